// vmx_api.cpp — implementation of the C ABI in include/vermilion_hip.h: the one host translation unit, made of the
// parts listed at its end (one per family of entries).
//
// Host orchestration only: BVH build (bvh_build.cpp), uploads, the pass loop
// of the wavefront pipeline, statistics.  All arithmetic that defines results
// runs in the gfx950 kernels (vmx_kernels.hip); there is no CPU rendering
// path here — without a HIP device every compute entry point fails.
#include "../../include/vermilion_hip.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "bvh_build.h"
#include "vmx_device.h"
#include "vmx_kernels.h"
#include "pixel_claim.h"  // kListWords
#include "pass_schedule.h"  // plan_pass, pass_form: the pure decisions of render_pass

#ifndef VMX_LDS_PRIMARY
#define VMX_LDS_PRIMARY 8  // LDS stack levels of the camera-ray kernel (A/B builds: make EXTRA=-DVMX_LDS_PRIMARY=n)
#endif

using namespace vmx;

// The parts, one per family of entries:
#include "vmx_host.h"          // shared: error reporting, the owners of device resources, the scene and its workspace, frame set-up
#include "api_ab.inc"          // what only the A/B library runs, behind ab_* hooks (the host side's one VMX_AB_KERNELS conditional)
#include "api_guide.inc"       // the guided bounce generation; vmx_guide_rays, vmx_guide_fused_rays, vmx_guide_list_entries, vmx_guide_trace*
#include "api_claims.inc"      // per-pixel claims and list claims; vmx_pixel_claims, vmx_pixel_claim_lists, vmx_list_settled_rays, vmx_fused_camera_paths
#include "api_render.inc"      // the pass loop by form (its schedule: pass_schedule.h); vmx_render*, vmx_local_rows
#include "api_nee.inc"         // light sampling: the emitter table, vmx_render_nee*, vmx_radiance_nee
#include "api_bruteforce.inc"  // BruteForceTracer: vmx_render_bruteforce*
#include "api_scene.inc"       // vmx_scene_create / destroy / bind_texture / describe / timings / bvh
#include "api_query.inc"       // vmx_trace, vmx_raycast*, vmx_query*, vmx_primary_ids, vmx_radiance, vmx_trig
#include "api_image.inc"       // shared by the image-space entries below: handle, overlap and params checks; vmx_variance_default_params
#include "api_filter.inc"      // vmx_filter_*
#include "api_upsample.inc"    // vmx_upsample_*
#include "api_albedo.inc"      // vmx_albedo_camera_device
#include "api_temporal.inc"    // vmx_temporal_*
#include "api_motion.inc"      // vmx_motion_device, vmx_motion_spheres_device
#include "api_progressive.inc" // vmx_progressive_*
#include "api_sampling.inc"    // adaptive sampling: vmx_progressive_state / step_selected / error / select / step_adaptive, vmx_sampling_default_params
#include "api_multi.inc"       // vmx_multi_*, vmx_assemble_device, vmx_quantize_device
#include "api_update.inc"      // vmx_scene_update*, vmx_multi_update, vmx_scene_set_spheres, vmx_multi_set_spheres, vmx_scene_set_emitters, vmx_scene_emitters
