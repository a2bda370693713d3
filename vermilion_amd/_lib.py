"""ctypes binding of the C ABI declared in include/vermilion_hip.h.

The shared library is the product; this module only loads it and declares
argument types.  There is no CPU fallback: if ``libvermilion_hip.so`` is
missing or cannot be loaded, importing the package fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VMX_LIB") or os.path.join(_HERE, "libvermilion_hip.so")  # VMX_LIB: A/B builds

VMX_OK = 0
VMX_ERR_INVALID = 1
VMX_ERR_NO_DEVICE = 2
VMX_ERR_HIP = 3
VMX_ERR_DEPTH = 4
VMX_ERR_NOMEM = 5

VMX_SPHERE_EMIT = 1
VMX_SAMPLING_PARITY = 0
VMX_SAMPLING_CORRECTED = 1
VMX_SAMPLING_LIBM_DOUBLE = 0x100
VMX_SAMPLING_ELIDE_DEAD = 0x200
VMX_BVH_REFERENCE = 0
VMX_BVH_SAH = 1
VMX_BVH_LBVH = 2
VMX_BVH_PLOC = 3
VMX_BF_ABS_INT = 1
VMX_ROTATION_DEGREES = 0
VMX_ROTATION_RADIANS = 1
VMX_QUERY_NEAREST = 0
VMX_QUERY_ANY = 1
VMX_QUERY_COLLISION = 2
VMX_QUERY_FETCH_PER_LANE = 0x100
VMX_ALBEDO_FLOOR = 2.0 ** -10  # the demodulated filter's lower clamp of an albedo channel
VMX_TEMPORAL_MOMENTS = 1  # vmx_temporal_create_ex: the handle keeps luminance moments (vmx_temporal_accumulate_variance_device)
VMX_PROGRESSIVE_MOMENTS = 1  # vmx_progressive_begin_ex: the handle keeps the sum of squared sample luminances (adaptive sampling)
VMX_VARIANCE_EPS = 1e-10  # the variance-guided filter's floor of sigma_luminance^2 * variance
VMX_SIGMA_LUMINANCE_DEFAULT = 4.0
VMX_ADAPTIVE_EPS = 1e-10  # the adaptive accumulation's floor of the window mean's squared standard error
VMX_UPDATE_REFIT = 0
VMX_UPDATE_REBUILD = 1
VMX_MAX_EMITTERS = 65536


class Sphere(C.Structure):
    _fields_ = [
        ("centre", C.c_float * 3),
        ("radius", C.c_float),
        ("colour", C.c_float * 3),
        ("flags", C.c_uint32),
        ("normal_centre", C.c_float * 3),
        ("normal_sign", C.c_float),
    ]


class Emitter(C.Structure):
    _fields_ = [("tri_id", C.c_uint32), ("radiance", C.c_float * 3)]


class EmitterInfo(C.Structure):
    _fields_ = [("tri_id", C.c_uint32), ("radiance", C.c_float * 3), ("area", C.c_double), ("weight", C.c_double),
                ("cdf", C.c_double)]


class CameraDesc(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("rotation_deg", C.c_float * 3),
        ("back_distance", C.c_float),
        ("back_size", C.c_float * 2),
        ("image_res", C.c_uint32 * 2),
        ("rays_per_pixel", C.c_uint32),
        ("rotation_units", C.c_uint32),
        ("rotation_rad", C.c_float * 3),
    ]


class Opts(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64),
        ("early_stop", C.c_uint32),
        ("sampling", C.c_uint32),
        ("rank", C.c_uint32),
        ("world", C.c_uint32),
        ("stripe_rows", C.c_uint32),
        ("samples_per_batch", C.c_uint32),
        ("collect_counters", C.c_uint32),
        ("reserved", C.c_uint32 * 7),
    ]


class StageStats(C.Structure):
    _fields_ = [
        ("rays", C.c_uint64),
        ("inner_visits", C.c_uint64),
        ("tri_tests", C.c_uint64),
        ("tri_hits", C.c_uint64),
        ("continued", C.c_uint64),
        ("launches", C.c_uint64),
        ("ms", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Stats(C.Structure):
    _fields_ = [
        ("rays_primary", C.c_uint64),
        ("rays_secondary", C.c_uint64),
        ("samples", C.c_uint64),
        ("samples_discarded", C.c_uint64),
        ("passes", C.c_uint64),
        ("kernel_launches", C.c_uint64),
        ("ms_total", C.c_double),
        ("ms_device", C.c_double),
        ("primary", StageStats),
        ("bounce", StageStats),
        ("shade", StageStats),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("primary", "bounce", "shade")}
        d["primary"] = self.primary.as_dict()
        d["bounce"] = self.bounce.as_dict()
        d["shade"] = self.shade.as_dict()
        return d


class SceneDesc(C.Structure):
    _fields_ = [
        ("ntris", C.c_uint32),
        ("nspheres", C.c_uint32),
        ("leaf_size", C.c_uint32),
        ("n_nodes", C.c_uint32),
        ("n_leaves", C.c_uint32),
        ("n_inner", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("stack_entries", C.c_uint32),
        ("device_bytes", C.c_uint64),
        ("device", C.c_int32),
        ("pad", C.c_uint32),
    ]


K_NAMES = ["raygen", "trace_camera", "shade_camera", "trace_bounce", "shade_bounce", "tail", "fused", "resolve",
           "bruteforce", "other"]  # VMX_K_* of vermilion_hip.h


class Timings(C.Structure):
    _fields_ = [("ms", C.c_double * 10), ("longest_ms", C.c_double * 10), ("launches", C.c_uint64 * 10)]

    def as_dict(self):
        return {n: {"ms": self.ms[i], "longest_ms": self.longest_ms[i], "launches": self.launches[i]}
                for i, n in enumerate(K_NAMES)}


class MultiTimes(C.Structure):
    _fields_ = [("slowest_render_ms", C.c_double), ("gather_ms", C.c_double), ("gather_sum_ms", C.c_double),
                ("assemble_ms", C.c_double), ("wall_ms", C.c_double), ("world", C.c_uint32), ("pad", C.c_uint32)]


class RayHit(C.Structure):
    _fields_ = [
        ("location", C.c_float * 3),
        ("distance", C.c_float),
        ("normal", C.c_float * 3),
        ("tri_id", C.c_int32),
        ("uv", C.c_float * 2),
        ("tri_t", C.c_float),
        ("flags", C.c_uint32),
        ("colour", C.c_float * 3),
        ("pad", C.c_uint32),
    ]


class ProgressiveInfo(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("rows", C.c_uint32),
        ("kmax", C.c_uint32),
        ("pixels_active", C.c_uint32),
        ("samples", C.c_uint64),
        ("passes", C.c_uint64),
        ("steps", C.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FilterParams(C.Structure):
    _fields_ = [
        ("iterations", C.c_uint32),
        ("normal_squarings", C.c_uint32),
        ("sigma_colour", C.c_float),
        ("sigma_depth", C.c_float),
        ("reserved", C.c_uint32 * 4),
    ]

    def as_dict(self):
        return {"iterations": self.iterations, "normal_squarings": self.normal_squarings,
                "sigma_colour": self.sigma_colour, "sigma_depth": self.sigma_depth, "reserved": list(self.reserved)}


class Motion(C.Structure):
    _fields_ = [
        ("prev_location", C.c_float * 3),
        ("flags", C.c_uint32),
        ("prev_normal", C.c_float * 3),
        ("pad", C.c_uint32),
    ]


class TemporalParams(C.Structure):
    _fields_ = [
        ("normal_min", C.c_float),
        ("plane_tol", C.c_float),
        ("max_history", C.c_float),
        ("reserved", C.c_uint32 * 5),
    ]

    def as_dict(self):
        return {"normal_min": self.normal_min, "plane_tol": self.plane_tol, "max_history": self.max_history,
                "reserved": list(self.reserved)}


class VarianceParams(C.Structure):
    _fields_ = [
        ("min_history", C.c_float),
        ("normal_squarings", C.c_uint32),
        ("sigma_depth", C.c_float),
        ("reserved", C.c_uint32 * 5),
    ]

    def as_dict(self):
        return {"min_history": self.min_history, "normal_squarings": self.normal_squarings,
                "sigma_depth": self.sigma_depth, "reserved": list(self.reserved)}


class AdaptiveParams(C.Structure):
    _fields_ = [
        ("gamma", C.c_float),
        ("min_support", C.c_float),
        ("normal_squarings", C.c_uint32),
        ("sigma_depth", C.c_float),
        ("reserved", C.c_uint32 * 4),
    ]

    def as_dict(self):
        return {"gamma": self.gamma, "min_support": self.min_support, "normal_squarings": self.normal_squarings,
                "sigma_depth": self.sigma_depth, "reserved": list(self.reserved)}


class SamplingParams(C.Structure):
    _fields_ = [
        ("threshold", C.c_float),
        ("floor", C.c_float),
        ("min_samples", C.c_uint32),
        ("radius", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]

    def as_dict(self):
        return {"threshold": self.threshold, "floor": self.floor, "min_samples": self.min_samples, "radius": self.radius,
                "reserved": list(self.reserved)}


class SamplingBudgetParams(C.Structure):
    _fields_ = [
        ("select", SamplingParams),
        ("max_step", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]

    def as_dict(self):
        return {"select": self.select.as_dict(), "max_step": self.max_step, "reserved": list(self.reserved)}


class UpsampleParams(C.Structure):
    _fields_ = [
        ("normal_squarings", C.c_uint32),
        ("sigma_depth", C.c_float),
        ("reserved", C.c_uint32 * 6),
    ]

    def as_dict(self):
        return {"normal_squarings": self.normal_squarings, "sigma_depth": self.sigma_depth, "reserved": list(self.reserved)}


# every symbol include/vermilion_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "vmx_abi_version": (C.c_int, []),
    "vmx_last_error": (C.c_char_p, []),
    "vmx_device_count": (C.c_int, []),
    "vmx_default_spheres": (C.POINTER(Sphere), [C.POINTER(C.c_uint32)]),
    "vmx_scene_create": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "vmx_scene_create_ex": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                     C.POINTER(_P)]),
    "vmx_scene_destroy": (C.c_int, [_P]),
    "vmx_scene_bind_texture": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "vmx_scene_describe": (C.c_int, [_P, C.POINTER(SceneDesc)]),
    "vmx_scene_timings": (C.c_int, [_P, C.POINTER(Timings)]),
    "vmx_scene_compute_units": (C.c_uint32, [_P]),
    "vmx_scene_bvh": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "vmx_scene_update": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32]),
    "vmx_scene_update_device": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, _P]),
    "vmx_scene_set_spheres": (C.c_int, [_P, _P, C.c_uint32]),
    "vmx_trace": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P]),
    "vmx_raycast": (C.c_int, [_P, _P, _P, C.c_uint32, _P]),
    "vmx_query_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.c_uint32, _P, _P, _P, _P]),
    "vmx_query": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.c_uint32, _P, _P, _P]),
    "vmx_raycast_device": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, _P]),
    "vmx_raycast_camera_device": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), C.c_uint32, _P, C.c_uint32,
                                            _P]),
    "vmx_primary_ids": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), C.c_uint32, _P, _P]),
    "vmx_pixel_claims": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(C.c_uint32)]),
    "vmx_fused_camera_paths": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "vmx_pixel_claim_lists": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, _P, C.POINTER(C.c_uint32)]),
    "vmx_list_settled_rays": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "vmx_guide_rays": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vmx_guide_list_entries": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "vmx_guide_fused_rays": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vmx_guide_trace": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "vmx_guide_trace_visits": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P]),
    "vmx_radiance": (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(Opts), _P, C.POINTER(Stats)]),
    "vmx_trig": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_int]),
    "vmx_local_rows": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "vmx_render": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(Stats)]),
    "vmx_render_device": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, _P, C.POINTER(Stats)]),
    "vmx_progressive_begin": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(_P)]),
    "vmx_progressive_step": (C.c_int, [_P, C.c_uint32, C.POINTER(Stats)]),
    "vmx_progressive_info_get": (C.c_int, [_P, C.POINTER(ProgressiveInfo)]),
    "vmx_progressive_preview_device": (C.c_int, [_P, _P, _P]),
    "vmx_progressive_preview": (C.c_int, [_P, _P, _P]),
    "vmx_progressive_end": (C.c_int, [_P]),
    "vmx_progressive_begin_ex": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), C.c_uint32, _P, C.POINTER(_P)]),
    "vmx_progressive_state_device": (C.c_int, [_P, _P, _P]),
    "vmx_progressive_step_selected_device": (C.c_int, [_P, C.c_uint32, _P, C.POINTER(Stats), C.POINTER(C.c_uint32)]),
    "vmx_sampling_default_params": (C.c_int, [C.POINTER(SamplingParams)]),
    "vmx_progressive_error_device": (C.c_int, [_P, C.POINTER(SamplingParams), _P, _P]),
    "vmx_progressive_select_device": (C.c_int, [_P, C.POINTER(SamplingParams), _P, _P]),
    "vmx_progressive_step_adaptive": (C.c_int, [_P, C.c_uint32, C.POINTER(SamplingParams), C.POINTER(Stats),
                                                C.POINTER(C.c_uint32)]),
    "vmx_progressive_begin_nee": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), C.c_uint32, _P, C.POINTER(_P)]),
    "vmx_sampling_budget_default_params": (C.c_int, [C.POINTER(SamplingBudgetParams)]),
    "vmx_progressive_budget_device": (C.c_int, [_P, C.POINTER(SamplingBudgetParams), _P, _P]),
    "vmx_progressive_step_budget_device": (C.c_int, [_P, _P, C.POINTER(Stats), C.POINTER(C.c_uint32)]),
    "vmx_progressive_step_budgeted": (C.c_int, [_P, C.POINTER(SamplingBudgetParams), C.POINTER(Stats), C.POINTER(C.c_uint32)]),
    "vmx_filter_default_params": (C.c_int, [C.POINTER(FilterParams)]),
    "vmx_filter_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "vmx_filter_destroy": (C.c_int, [_P]),
    "vmx_filter_set_guide_device": (C.c_int, [_P, _P, _P]),
    "vmx_filter_apply_device": (C.c_int, [_P, _P, _P, _P, C.POINTER(FilterParams), _P]),
    "vmx_progressive_preview_filtered_device": (C.c_int, [_P, _P, _P, C.POINTER(FilterParams)]),
    "vmx_progressive_preview_filtered": (C.c_int, [_P, _P, _P, C.POINTER(FilterParams)]),
    "vmx_albedo_camera_device": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), C.c_uint32, C.c_uint32, _P, _P]),
    "vmx_filter_apply_demodulated_device": (C.c_int, [_P, _P, _P, _P, _P, C.POINTER(FilterParams), _P]),
    "vmx_progressive_preview_demodulated_device": (C.c_int, [_P, _P, _P, C.POINTER(FilterParams), C.c_uint32]),
    "vmx_progressive_preview_demodulated": (C.c_int, [_P, _P, _P, C.POINTER(FilterParams), C.c_uint32]),
    "vmx_temporal_default_params": (C.c_int, [C.POINTER(TemporalParams)]),
    "vmx_temporal_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "vmx_temporal_destroy": (C.c_int, [_P]),
    "vmx_temporal_reset": (C.c_int, [_P, _P]),
    "vmx_temporal_frames": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "vmx_temporal_accumulate_device": (C.c_int, [_P, C.POINTER(CameraDesc), _P, _P, _P, _P, _P, C.POINTER(TemporalParams),
                                                 _P]),
    "vmx_temporal_accumulate_motion_device": (C.c_int, [_P, C.POINTER(CameraDesc), _P, _P, _P, _P, _P, _P,
                                                        C.POINTER(TemporalParams), _P]),
    "vmx_motion_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.c_uint32, _P, C.c_int, _P]),
    "vmx_motion_spheres_device": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.c_uint32, _P, _P, _P]),
    "vmx_variance_default_params": (C.c_int, [C.POINTER(VarianceParams)]),
    "vmx_temporal_create_ex": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "vmx_temporal_accumulate_variance_device": (C.c_int, [_P, C.POINTER(CameraDesc), _P, _P, _P, _P, _P, _P, _P,
                                                          C.POINTER(TemporalParams), C.POINTER(VarianceParams), _P]),
    "vmx_filter_apply_variance_device": (C.c_int, [_P, _P, _P, _P, _P, _P, C.POINTER(FilterParams), C.c_float, _P]),
    "vmx_adaptive_default_params": (C.c_int, [C.POINTER(AdaptiveParams)]),
    "vmx_temporal_accumulate_adaptive_device": (C.c_int, [_P, C.POINTER(CameraDesc), _P, _P, _P, _P, _P, _P, _P, _P,
                                                          C.POINTER(TemporalParams), C.POINTER(VarianceParams),
                                                          C.POINTER(AdaptiveParams), _P]),
    "vmx_upsample_default_params": (C.c_int, [C.POINTER(UpsampleParams)]),
    "vmx_upsample_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "vmx_upsample_destroy": (C.c_int, [_P]),
    "vmx_upsample_set_guides_device": (C.c_int, [_P, _P, _P, _P]),
    "vmx_upsample_apply_device": (C.c_int, [_P, _P, _P, _P, C.POINTER(UpsampleParams), _P]),
    "vmx_render_bruteforce": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), C.c_uint32, _P, C.POINTER(Stats)]),
    "vmx_render_bruteforce_device": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), C.c_uint32, _P, _P,
                                              C.POINTER(Stats)]),
    "vmx_render_nee": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(Stats)]),
    "vmx_render_nee_device": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(Stats), _P]),
    "vmx_radiance_nee": (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(Opts), _P, C.POINTER(Stats)]),
    "vmx_render_nee_rank": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(Stats)]),
    "vmx_render_nee_rank_device": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(Stats), _P]),
    "vmx_radiance_nee_device": (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(Opts), _P, C.POINTER(Stats), _P]),
    "vmx_progressive_begin_nee_rank": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), C.c_uint32, _P, C.POINTER(_P)]),
    "vmx_multi_render_nee": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(Stats)]),
    "vmx_multi_render_nee_device": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(Stats)]),
    "vmx_multi_create": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int),
                                  C.c_uint32, C.POINTER(_P)]),
    "vmx_multi_destroy": (C.c_int, [_P]),
    "vmx_multi_world": (C.c_uint32, [_P]),
    "vmx_multi_routes": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vmx_multi_timings": (C.c_int, [_P, C.POINTER(MultiTimes), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vmx_multi_bind_texture": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "vmx_multi_update": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32]),
    "vmx_multi_set_spheres": (C.c_int, [_P, _P, C.c_uint32]),
    "vmx_scene_set_emitters": (C.c_int, [_P, _P, C.c_uint32]),
    "vmx_scene_emitters": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "vmx_multi_set_emitters": (C.c_int, [_P, _P, C.c_uint32]),
    "vmx_emitters_check": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "vmx_multi_render": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(Stats)]),
    "vmx_multi_render_device": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), _P, C.POINTER(Stats)]),
    "vmx_multi_render_bruteforce": (C.c_int, [_P, C.POINTER(CameraDesc), C.POINTER(Opts), C.c_uint32, _P,
                                             C.POINTER(Stats)]),
    "vmx_quantize_device": (C.c_int, [_P, C.c_uint64, _P, _P, C.c_int, _P]),
    "vmx_assemble_device": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_int, _P]),
}


def load(path=None):
    """Load the HIP library and declare its prototypes.  Raises if it is absent."""
    path = path or LIB_PATH
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7.
    # If torch is importable, load it first so this library binds to the same
    # runtime (two runtimes in one process cannot both open the GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  vermilion_amd has no CPU fallback."
        )
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


class VmxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"vermilion_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load()
    return _lib


def check(code):
    if code != VMX_OK:
        raise VmxError(code, lib().vmx_last_error().decode("utf-8", "replace"))
