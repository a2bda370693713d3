"""vermilion_amd — MI355X-native hot path of the Vermilion path tracer.

The product is ``libvermilion_hip.so`` (hand-written gfx950 kernels behind the
C ABI of ``include/vermilion_hip.h``).  This package is the host-side mirror of
the reference's Integrator plugin surface plus synthetic scene generators.
Importing `vermilion_amd` does not need a GPU; creating a Scene does.
"""
from . import _lib
from ._lib import (VMX_SAMPLING_CORRECTED, VMX_SAMPLING_ELIDE_DEAD, VMX_SAMPLING_LIBM_DOUBLE, VMX_SAMPLING_PARITY, VmxError)
from ._lib import VMX_ADAPTIVE_EPS as ADAPTIVE_EPS
from ._lib import VMX_ALBEDO_FLOOR as ALBEDO_FLOOR
from ._lib import VMX_SIGMA_LUMINANCE_DEFAULT as SIGMA_LUMINANCE_DEFAULT
from ._lib import VMX_VARIANCE_EPS as VARIANCE_EPS
from .scene import (MOTION_DTYPE, MultiScene, Progressive, Scene, default_spheres,
                    local_row_indices, local_rows, low_camera, make_adaptive_params, make_camera, make_filter_params, make_opts,
                    make_sampling_budget_params, make_sampling_params, make_temporal_params, make_upsample_params, make_variance_params, motion_vectors, sphere_motion_vectors,
                    spheres_array)
from .image import Filter, Temporal, Upsample
from .api import (Camera, Integrator, MeshEngine, PathTracer, RenderEngine, cameraSettings, float3,
                  pixelValue, vermRenderMode)
from . import scenes

__all__ = [
    "Scene", "MultiScene", "Progressive", "Filter", "make_filter_params", "Upsample", "make_upsample_params", "low_camera", "Temporal", "make_temporal_params", "make_variance_params", "make_adaptive_params", "make_sampling_params", "make_sampling_budget_params", "ADAPTIVE_EPS", "VARIANCE_EPS", "SIGMA_LUMINANCE_DEFAULT", "motion_vectors", "sphere_motion_vectors", "MOTION_DTYPE", "ALBEDO_FLOOR", "make_camera", "make_opts", "spheres_array", "default_spheres", "local_rows",
    "local_row_indices", "Camera", "Integrator", "MeshEngine", "PathTracer", "RenderEngine",
    "cameraSettings", "float3", "pixelValue", "vermRenderMode", "scenes", "VmxError",
    "VMX_SAMPLING_PARITY", "VMX_SAMPLING_CORRECTED", "VMX_SAMPLING_LIBM_DOUBLE", "VMX_SAMPLING_ELIDE_DEAD",
]
