"""Thin object wrapper over the C ABI: one `Scene` = one `vmx_scene*`.

numpy arrays in, numpy arrays out; all compute happens in libvermilion_hip.so.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def _is_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _f32(a, shape_last=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape_last is not None and (a.ndim == 0 or a.shape[-1] != shape_last):
        a = a.reshape(-1, shape_last)
    return a


def _device_rays(x, name):
    """a ray array as the device entries take it (contiguous float32 [n, 3] tensor), or a ValueError"""
    import torch
    if not _is_tensor(x):
        raise ValueError(f"{name}: mix of torch tensors and other arrays")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{name} must be [n, 3]")
    if x.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 (got {x.dtype})")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return x


class _SideStream:
    """The stream a device entry runs on: `stream` (default: the current stream).  torch's default stream is the
    legacy NULL stream, which the ABI reads as "the scene's own stream": then a side stream ordered after it, and it
    after the side stream (as Scene.query)"""

    def __init__(self, dev, stream):
        import torch
        self.s = stream if stream is not None else torch.cuda.current_stream(dev)
        self.side = torch.cuda.Stream(dev) if self.s.cuda_stream == 0 else None

    def __enter__(self):
        if self.side is not None:
            self.side.wait_stream(self.s)
            return self.side
        return self.s

    def __exit__(self, *exc):
        if self.side is not None:
            self.s.wait_stream(self.side)


def _rayhit_views(raw):
    """named views over [..., 16] float32 vmx_rayhit records (RAYHIT_DTYPE's fields; tri_id / flags as int32)"""
    import torch
    words = raw.view(torch.int32)
    return {"location": raw[..., 0:3], "distance": raw[..., 3], "normal": raw[..., 4:7], "tri_id": words[..., 7],
            "uv": raw[..., 8:10], "tri_t": raw[..., 10], "flags": words[..., 11], "colour": raw[..., 12:15], "raw": raw}


def make_camera(position, rotation_deg, width, height, spp, back_distance=6.0, back_size=(3.6, 2.4), rotation_rad=None):
    """cameraSettings subset (core/camera/camera.h:32-47); defaults follow
    RenderEngine::CreateInternalDefaultCamera (core/engines/renderEngine.cpp:135-139).
    rotation_rad: Camera::mRotation itself (radians, x and y already negated, camera.cpp:43-47) instead of the
    settings' degrees — what an Integrator holds (VMX_ROTATION_RADIANS)."""
    c = L.CameraDesc()
    c.position[:] = [float(v) for v in position]
    if rotation_rad is not None:
        c.rotation_units = L.VMX_ROTATION_RADIANS
        c.rotation_rad[:] = [float(v) for v in rotation_rad]
    else:
        c.rotation_deg[:] = [float(v) for v in rotation_deg]
    c.back_distance = float(back_distance)
    c.back_size[:] = [float(back_size[0]), float(back_size[1])]
    c.image_res[:] = [int(width), int(height)]
    c.rays_per_pixel = int(spp)
    return c


def make_opts(seed=1, early_stop=True, sampling=L.VMX_SAMPLING_PARITY, rank=0, world=1, stripe_rows=16,
              samples_per_batch=0, collect_counters=False, pipeline=0, max_paths=0, tail_threshold=0,
              refill_min=0, shade_min=0, reorder=0, lds_entries=0):
    o = L.Opts()
    o.seed = int(seed)
    o.early_stop = 1 if early_stop else 0
    o.sampling = int(sampling)
    o.rank, o.world, o.stripe_rows = int(rank), int(world), int(stripe_rows)
    o.samples_per_batch = int(samples_per_batch)
    o.collect_counters = 1 if collect_counters else 0
    o.reserved[0] = int(pipeline)      # 0 default routing, 1 fused kernel for every pass, 4 split wavefront for every pass; 2/3 first-generation kernels (A/B library only); | 0x100 one-phase shading, | 0x200 two-phase shading (k_shade_ends) instead of sorted rays, | 0x800 no per-pixel claims, | 0x1000 claimed pixels are not fused into the shading kernel, | 0x2000 no list claims, | 0x4000 no guide tree for the bounce rays
    o.reserved[1] = int(max_paths)     # paths in flight per pass (0 -> 16M)
    o.reserved[2] = int(tail_threshold)
    o.reserved[3] = int(refill_min)    # k_paths: refill when this many lanes idle (0 -> 16)
    o.reserved[4] = int(shade_min)     # k_paths: shade when this many lanes finished (0 -> 16)
    o.reserved[5] = int(reorder)       # bounce reordering key (vmx_host.h: Tuning::sort_mode); 0 = the library's default
    o.reserved[6] = int(lds_entries)   # stack levels kept in LDS, all kernels (0 -> 8 camera / 13 bounce / 10 fused); deeper ones spill to HBM
    return o


def make_filter_params(iterations=None, normal_squarings=None, sigma_colour=None, sigma_depth=None):
    """vmx_filter_params: the library's defaults (vmx_filter_default_params) with the given fields replaced"""
    p = L.FilterParams()
    L.check(L.lib().vmx_filter_default_params(C.byref(p)))
    if iterations is not None:
        p.iterations = int(iterations)
    if normal_squarings is not None:
        p.normal_squarings = int(normal_squarings)
    if sigma_colour is not None:
        p.sigma_colour = float(sigma_colour)
    if sigma_depth is not None:
        p.sigma_depth = float(sigma_depth)
    return p


def make_temporal_params(normal_min=None, plane_tol=None, max_history=None):
    """vmx_temporal_params: the library's defaults (vmx_temporal_default_params) with the given fields replaced"""
    p = L.TemporalParams()
    L.check(L.lib().vmx_temporal_default_params(C.byref(p)))
    if normal_min is not None:
        p.normal_min = float(normal_min)
    if plane_tol is not None:
        p.plane_tol = float(plane_tol)
    if max_history is not None:
        p.max_history = float(max_history)
    return p


def make_variance_params(min_history=None, normal_squarings=None, sigma_depth=None):
    """vmx_variance_params: the library's defaults (vmx_variance_default_params) with the given fields replaced"""
    p = L.VarianceParams()
    L.check(L.lib().vmx_variance_default_params(C.byref(p)))
    if min_history is not None:
        p.min_history = float(min_history)
    if normal_squarings is not None:
        p.normal_squarings = int(normal_squarings)
    if sigma_depth is not None:
        p.sigma_depth = float(sigma_depth)
    return p


def make_adaptive_params(gamma=None, min_support=None, normal_squarings=None, sigma_depth=None):
    """vmx_adaptive_params: the library's defaults (vmx_adaptive_default_params) with the given fields replaced"""
    p = L.AdaptiveParams()
    L.check(L.lib().vmx_adaptive_default_params(C.byref(p)))
    if gamma is not None:
        p.gamma = float(gamma)
    if min_support is not None:
        p.min_support = float(min_support)
    if normal_squarings is not None:
        p.normal_squarings = int(normal_squarings)
    if sigma_depth is not None:
        p.sigma_depth = float(sigma_depth)
    return p


def make_sampling_params(threshold=None, floor=None, min_samples=None, radius=None):
    """vmx_sampling_params: the library's defaults (vmx_sampling_default_params) with the given fields replaced"""
    p = L.SamplingParams()
    L.check(L.lib().vmx_sampling_default_params(C.byref(p)))
    if threshold is not None:
        p.threshold = float(threshold)
    if floor is not None:
        p.floor = float(floor)
    if min_samples is not None:
        p.min_samples = int(min_samples)
    if radius is not None:
        p.radius = int(radius)
    return p


def make_sampling_budget_params(threshold=None, floor=None, min_samples=None, radius=None, max_step=None):
    """vmx_sampling_budget_params: the library's defaults (vmx_sampling_budget_default_params) with the given fields
    replaced; threshold, floor, min_samples and radius are its `select` member's"""
    p = L.SamplingBudgetParams()
    L.check(L.lib().vmx_sampling_budget_default_params(C.byref(p)))
    if threshold is not None:
        p.select.threshold = float(threshold)
    if floor is not None:
        p.select.floor = float(floor)
    if min_samples is not None:
        p.select.min_samples = int(min_samples)
    if radius is not None:
        p.select.radius = int(radius)
    if max_step is not None:
        p.max_step = int(max_step)
    return p


def make_upsample_params(normal_squarings=None, sigma_depth=None):
    """vmx_upsample_params: the library's defaults (vmx_upsample_default_params) with the given fields replaced"""
    p = L.UpsampleParams()
    L.check(L.lib().vmx_upsample_default_params(C.byref(p)))
    if normal_squarings is not None:
        p.normal_squarings = int(normal_squarings)
    if sigma_depth is not None:
        p.sigma_depth = float(sigma_depth)
    return p


def low_camera(cam, low_width, low_height):
    """a copy of the CameraDesc `cam` with image_res replaced: the same field of view on fewer pixels, what a frame for
    Upsample is rendered and ray-cast with"""
    c = L.CameraDesc()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(L.CameraDesc))
    c.image_res[:] = [int(low_width), int(low_height)]
    return c


def _frame_tensor(x, name, dtype, shape, dev):
    """an output or input of the device filter / previews as the ABI takes it, or a ValueError"""
    if not _is_tensor(x):
        raise ValueError(f"{name} must be a torch tensor")
    if x.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {x.dtype})")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)} (got {list(x.shape)})")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if x.device != dev:
        raise ValueError(f"{name} must be on {dev} (got {x.device})")
    return x


def _albedo_tensor(x, name, shape, dev):
    """an albedo plane as the ABI takes it (contiguous float32 [height, width, 4] on dev, 16-byte aligned), or a ValueError"""
    import torch
    _frame_tensor(x, name, torch.float32, tuple(shape) + (4,), dev)
    if x.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")
    return x


def motion_vectors(raw, pos_now, pos_prev, nrm_prev=None, out=None, stream=None):
    """vmx_motion_device: the motion records of a G-buffer after a geometry update, for Temporal.accumulate(motion=...).
    `raw` is the ["raw"] tensor of Scene.raycast_camera on the updated scene (float32 [..., 16]); `pos_now` and `pos_prev`
    the [ntris, 9] positions after and before the update (what Scene.update took); `nrm_prev` the [ntris, 9] normals
    before it, or None (right for translations).  Returns `out`, float32 [..., 8] words (MOTION_DTYPE's fields), made
    if not given.  All are contiguous float32 torch tensors on raw's device: anything else is a ValueError, never a
    copy through the host.  Enqueued on `stream` (default torch.cuda.current_stream()), nothing synchronised."""
    import torch
    if not _is_tensor(raw):
        raise ValueError("raw must be a torch tensor")
    if raw.dtype != torch.float32:
        raise ValueError(f"raw must be {torch.float32} (got {raw.dtype})")
    if len(raw.shape) < 1 or raw.shape[-1] != 16:
        raise ValueError(f"raw must be [..., 16] (got {list(raw.shape)})")
    if not raw.is_contiguous():
        raise ValueError("raw must be contiguous")
    dev = raw.device
    if dev.type != "cuda":
        raise ValueError(f"raw must be on cuda (got {dev})")
    if not _is_tensor(pos_now):
        raise ValueError("pos_now must be a torch tensor")
    if len(pos_now.shape) != 2 or pos_now.shape[0] == 0:
        raise ValueError(f"pos_now must be [ntris, 9] (got {list(pos_now.shape)})")
    ntris = int(pos_now.shape[0])
    _frame_tensor(pos_now, "pos_now", torch.float32, (ntris, 9), dev)
    _frame_tensor(pos_prev, "pos_prev", torch.float32, (ntris, 9), dev)
    if nrm_prev is not None:
        _frame_tensor(nrm_prev, "nrm_prev", torch.float32, (ntris, 9), dev)
    lead = tuple(raw.shape[:-1])
    n = 1
    for d in lead:
        n *= int(d)
    if out is None:
        out = torch.empty(lead + (8,), dtype=torch.float32, device=dev)
    else:
        _frame_tensor(out, "out", torch.float32, lead + (8,), dev)
    if n == 0:
        return out
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    with _SideStream(dev, stream) as run:
        L.check(L.lib().vmx_motion_device(ptr(raw), n, ptr(pos_now), ptr(pos_prev), ptr(nrm_prev), ntris, ptr(out),
                                          dev.index if dev.index is not None else torch.cuda.current_device(),
                                          C.c_void_p(run.cuda_stream)))
    return out


def _sphere_table(spheres, name):
    """(address, count) of a sphere table as Scene(...) takes it: None (NULL, 0: the reference's table) or a ctypes array of
    vmx_sphere (spheres_array / default_spheres; an empty one means no spheres at all)"""
    if spheres is None:
        return None, 0
    if not (isinstance(spheres, C.Array) and spheres._type_ is L.Sphere):
        raise ValueError(f"{name} must be None or a ctypes array of vmx_sphere (spheres_array, default_spheres)")
    return C.addressof(spheres), len(spheres)


def sphere_motion_vectors(raw, origin, spheres_now, spheres_prev, motion=None, out=None, stream=None):
    """vmx_motion_spheres_device: the motion records of a G-buffer's pixels that lie on a sphere which Scene.set_spheres
    moved, for Temporal.accumulate(motion=...).  `raw` is the ["raw"] tensor of Scene.raycast_camera on the scene as it is
    now (float32 [..., 16]); `origin` its rays' common origin, the camera's position (three floats); `spheres_now` and
    `spheres_prev` the table now and before, ctypes arrays of vmx_sphere of one length (None: the reference's table).
    `motion`: the records of motion_vectors for the same G-buffer, float32 [..., 8], or None; every pixel that is not on a
    moved sphere leaves as it is there.  Returns `out`, float32 [..., 8], made if not given; out may be `motion` itself.
    Tensors are contiguous float32 on raw's device: anything else is a ValueError, never a copy through the host.
    Enqueued on `stream` (default torch.cuda.current_stream()), nothing synchronised."""
    import torch
    if not _is_tensor(raw):
        raise ValueError("raw must be a torch tensor")
    if raw.dtype != torch.float32:
        raise ValueError(f"raw must be {torch.float32} (got {raw.dtype})")
    if len(raw.shape) < 1 or raw.shape[-1] != 16:
        raise ValueError(f"raw must be [..., 16] (got {list(raw.shape)})")
    if not raw.is_contiguous():
        raise ValueError("raw must be contiguous")
    dev = raw.device
    if dev.type != "cuda":
        raise ValueError(f"raw must be on cuda (got {dev})")
    o = np.ascontiguousarray(origin, dtype=np.float32).reshape(-1)
    if o.shape != (3,):
        raise ValueError(f"origin must be three floats (got {list(np.shape(origin))})")
    if spheres_now is None:
        spheres_now = default_spheres()
    if spheres_prev is None:
        spheres_prev = default_spheres()
    now, n_now = _sphere_table(spheres_now, "spheres_now")
    prev, n_prev = _sphere_table(spheres_prev, "spheres_prev")
    if n_now != n_prev:
        raise ValueError(f"spheres_now and spheres_prev must have one length (got {n_now} and {n_prev})")
    lead = tuple(raw.shape[:-1])
    n = 1
    for d in lead:
        n *= int(d)
    if motion is not None:
        _frame_tensor(motion, "motion", torch.float32, lead + (8,), dev)
    if out is None:
        out = torch.empty(lead + (8,), dtype=torch.float32, device=dev)
    else:
        _frame_tensor(out, "out", torch.float32, lead + (8,), dev)
    if n == 0:
        return out
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    with _SideStream(dev, stream) as run:
        L.check(L.lib().vmx_motion_spheres_device(ptr(raw), n, o.ctypes.data, now, prev, n_now, ptr(motion), ptr(out),
                                                  C.c_void_p(run.cuda_stream)))
    return out


def spheres_array(spheres):
    """list of dicts/tuples -> ctypes array of vmx_sphere"""
    arr = (L.Sphere * len(spheres))()
    for i, s in enumerate(spheres):
        arr[i].centre[:] = [float(v) for v in s["centre"]]
        arr[i].radius = float(s["radius"])
        arr[i].colour[:] = [float(v) for v in s.get("colour", (0, 0, 0))]
        arr[i].flags = L.VMX_SPHERE_EMIT if s.get("emit", False) else 0
        arr[i].normal_centre[:] = [float(v) for v in s.get("normal_centre", s["centre"])]
        arr[i].normal_sign = float(s.get("normal_sign", 1.0))
    return arr


def default_spheres():
    n = C.c_uint32(0)
    p = L.lib().vmx_default_spheres(C.byref(n))
    out = (L.Sphere * n.value)()
    for i in range(n.value):
        C.memmove(C.byref(out[i]), C.byref(p[i]), C.sizeof(L.Sphere))
    return out


class Scene:
    """Device-resident scene: replaces MeshEngine::createBVH + BVH for the HIP path."""

    def __init__(self, pos, nrm, uv=None, spheres=None, leaf_size=4, device=0, builder=L.VMX_BVH_REFERENCE, lib=None):
        """lib: a library object from _lib.load(path) — the tests' A/B library; default: the product library"""
        self._lib = lib if lib is not None else L.lib()
        pos = _f32(pos).reshape(-1, 9)
        nrm = _f32(nrm).reshape(-1, 9)
        if pos.shape != nrm.shape:
            raise ValueError("pos and nrm must both be [ntris, 9]")
        uvp = None
        if uv is not None:
            uv = _f32(uv).reshape(-1, 6)
            uvp = uv.ctypes.data
        self._spheres = spheres
        sp, nsp = (None, 0) if spheres is None else (C.addressof(spheres), len(spheres))
        h = C.c_void_p()
        self._check(self._lib.vmx_scene_create_ex(pos.ctypes.data, nrm.ctypes.data, uvp, pos.shape[0], sp, nsp,
                                            int(leaf_size), int(builder), int(device), C.byref(h)))
        self._h = h
        self.ntris = pos.shape[0]
        self.device = int(device)

    def _check(self, code):
        if code != L.VMX_OK:
            raise L.VmxError(code, self._lib.vmx_last_error().decode("utf-8", "replace"))

    def close(self):
        """vmx_scene_destroy; raises (and keeps the scene) while a progressive render of it is open"""
        if getattr(self, "_h", None):
            self._check(self._lib.vmx_scene_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def bind_texture(self, data):
        """MeshEngine::bindTexture (meshEngine.cpp:74-93): float image [H, W] or [H, W, C], C <= 4.
        Only the first bound texture is sampled (pathtracer.cpp:65)."""
        data = np.ascontiguousarray(data, dtype=np.float32)
        if data.ndim not in (2, 3):
            raise ValueError("texture must be [H, W] or [H, W, C]")
        c = 1 if data.ndim == 2 else data.shape[2]
        self._check(self._lib.vmx_scene_bind_texture(self._h, data.ctypes.data, data.shape[1], data.shape[0], c))
        return True

    # -- introspection ----------------------------------------------------
    def describe(self):
        d = L.SceneDesc()
        self._check(self._lib.vmx_scene_describe(self._h, C.byref(d)))
        return {k: getattr(d, k) for k, _ in d._fields_ if k != "pad"}

    def timings(self):
        """per-kernel device time of the last render on this scene (vmx_timings)"""
        t = L.Timings()
        self._check(self._lib.vmx_scene_timings(self._h, C.byref(t)))
        return t.as_dict()

    @property
    def compute_units(self):
        """the compute units the scene sizes its launches for: the device's, or fewer under VMX_CU_LIMIT"""
        return int(self._lib.vmx_scene_compute_units(self._h))

    def bvh(self):
        n = self.describe()["n_nodes"]
        start = np.zeros(n, np.uint32)
        nprims = np.zeros(n, np.uint32)
        roff = np.zeros(n, np.uint32)
        bbox = np.zeros((n, 6), np.float32)
        order = np.zeros(self.ntris, np.uint32)
        self._check(self._lib.vmx_scene_bvh(self._h, start.ctypes.data, nprims.ctypes.data, roff.ctypes.data,
                                      bbox.ctypes.data, order.ctypes.data))
        return {"start": start, "nprims": nprims, "right_offset": roff, "bbox": bbox, "prim_order": order}

    # -- parity hooks -------------------------------------------------------
    def trace(self, origin, direction):
        o, d = _f32(origin, 3), _f32(direction, 3)
        n = o.shape[0]
        tri = np.empty(n, np.int32)
        t = np.empty(n, np.float32)
        self._check(self._lib.vmx_trace(self._h, o.ctypes.data, d.ctypes.data, n, tri.ctypes.data, t.ctypes.data))
        return tri, t

    def raycast(self, origin, direction, stream=None, per_lane_fetch=False):
        """MeshEngine::RayCast (meshEngine.cpp:239-509) of a batch.

        numpy in -> vmx_raycast (host buffers, synchronous), a RAYHIT_DTYPE array out.  torch tensors on this scene's
        device in -> vmx_raycast_device on `stream` (default torch.cuda.current_stream()), nothing synchronised; out: a
        dict of views over one [n, 16] float32 tensor ("raw") — location [n, 3], distance [n], normal [n, 3], tri_id [n]
        (int32), uv [n, 2], tri_t [n], flags [n] (int32), colour [n, 3].  Device rays must be contiguous float32 [n, 3]:
        anything else is a ValueError, never a copy through the host.  per_lane_fetch: VMX_QUERY_FETCH_PER_LANE."""
        if _is_tensor(origin) or _is_tensor(direction):
            return self._raycast_device(origin, direction, stream, per_lane_fetch)
        o, d = _f32(origin, 3), _f32(direction, 3)
        n = o.shape[0]
        out = np.zeros(n, dtype=RAYHIT_DTYPE)
        self._check(self._lib.vmx_raycast(self._h, o.ctypes.data, d.ctypes.data, n, out.ctypes.data))
        return out

    def _raycast_device(self, origin, direction, stream, per_lane_fetch):
        import torch
        dev = torch.device("cuda", self.device)
        o, d = _device_rays(origin, "origin"), _device_rays(direction, "direction")
        if o.shape != d.shape:
            raise ValueError("origin and direction must both be [n, 3]")
        for x, name in ((o, "origin"), (d, "direction")):
            if x.device != dev:
                raise ValueError(f"{name} must be on {dev} (got {x.device})")
        n = o.shape[0]
        raw = torch.empty((n, 16), dtype=torch.float32, device=dev)
        if n:
            flags = L.VMX_QUERY_FETCH_PER_LANE if per_lane_fetch else 0
            with _SideStream(dev, stream) as run:
                self._check(self._lib.vmx_raycast_device(self._h, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                                         n, C.c_void_p(raw.data_ptr()), flags,
                                                         C.c_void_p(run.cuda_stream)))
        return _rayhit_views(raw)

    def raycast_camera(self, cam, opts, k=0, stream=None, per_lane_fetch=False):
        """vmx_raycast_camera_device: Scene.raycast's device record for sample k's camera ray of every pixel (the ray
        vmx_render traces and primary_ids reports), as a dict of [H, W, ...] views over one [H, W, 16] float32 tensor
        on this scene's device, computed on `stream` (default torch.cuda.current_stream()), nothing synchronised."""
        import torch
        dev = torch.device("cuda", self.device)
        W, H = int(cam.image_res[0]), int(cam.image_res[1])
        raw = torch.empty((H, W, 16), dtype=torch.float32, device=dev)
        flags = L.VMX_QUERY_FETCH_PER_LANE if per_lane_fetch else 0
        with _SideStream(dev, stream) as run:
            self._check(self._lib.vmx_raycast_camera_device(self._h, C.byref(cam), C.byref(opts), int(k),
                                                            C.c_void_p(raw.data_ptr()), flags,
                                                            C.c_void_p(run.cuda_stream)))
        return _rayhit_views(raw)

    def albedo_camera(self, cam, opts, samples=4, first=0, out=None, stream=None):
        """vmx_albedo_camera_device: the camera's albedo plane, float32 [H, W, 4] on this scene's device — per pixel the
        mean over samples first .. first + samples - 1 of what the integrator multiplies a camera path's throughput by
        at its first hit (the bound texture's texel, (1, 1, 1) off the mesh or without a texture), and in .w the
        fraction of those rays that hit the mesh.  `out`: a contiguous, 16-byte aligned float32 [H, W, 4] tensor on
        the scene's device to fill instead of a new one — anything else is a ValueError.  Computed on `stream`
        (default torch.cuda.current_stream()), nothing synchronised."""
        import torch
        dev = torch.device("cuda", self.device)
        W, H = int(cam.image_res[0]), int(cam.image_res[1])
        if int(samples) < 1:
            raise ValueError("samples must be at least 1")
        if int(first) < 0:
            raise ValueError("first must not be negative")
        if out is None:
            out = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        _albedo_tensor(out, "out", (H, W), dev)
        with _SideStream(dev, stream) as run:
            self._check(self._lib.vmx_albedo_camera_device(self._h, C.byref(cam), C.byref(opts), int(first), int(samples),
                                                           C.c_void_p(out.data_ptr()), C.c_void_p(run.cuda_stream)))
        return out

    # -- ray queries -----------------------------------------------------------
    QUERY_MODES = {"nearest": L.VMX_QUERY_NEAREST, "any": L.VMX_QUERY_ANY, "collision": L.VMX_QUERY_COLLISION}

    def query(self, origin, direction, tmax=None, mode="nearest", stream=None, per_lane_fetch=False):
        """Ray queries of a batch (vmx_query / vmx_query_device; semantics in include/vermilion_hip.h):
        "nearest" -> (tri_id, t, hit), "collision" -> (tri_id, t, hit) with hit = MeshEngine::RayCastCollision,
        "any" -> hit.  tmax: per-ray bound or None.

        numpy in -> the host entry, numpy out (int32, float32, bool).  torch tensors on this scene's device
        in -> the device entry on `stream` (default torch.cuda.current_stream()), tensors out (int32, float32,
        torch.bool), nothing synchronised.  Device rays must be contiguous float32 [n, 3] (tmax [n]): anything
        else is a ValueError, never a copy through the host.  per_lane_fetch: VMX_QUERY_FETCH_PER_LANE (tuning)."""
        if mode not in self.QUERY_MODES:
            raise ValueError(f"mode must be one of {sorted(self.QUERY_MODES)}")
        m = self.QUERY_MODES[mode] | (L.VMX_QUERY_FETCH_PER_LANE if per_lane_fetch else 0)
        want_ids = mode != "any"
        if _is_tensor(origin) or _is_tensor(direction) or _is_tensor(tmax):
            return self._query_device(origin, direction, tmax, m, want_ids, stream)
        o, d = _f32(origin, 3), _f32(direction, 3)
        if o.shape != d.shape:
            raise ValueError("origin and direction must both be [n, 3]")
        n = o.shape[0]
        tm = None
        if tmax is not None:
            tm = np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
            if tm.shape[0] != n:
                raise ValueError("tmax must hold one value per ray")
        hit = np.zeros(n, np.uint8)
        tri = np.empty(n, np.int32) if want_ids else None
        t = np.empty(n, np.float32) if want_ids else None
        self._check(self._lib.vmx_query(self._h, m, o.ctypes.data, d.ctypes.data, None if tm is None else tm.ctypes.data,
                                        n, None if tri is None else tri.ctypes.data, None if t is None else t.ctypes.data,
                                        hit.ctypes.data))
        hit = hit.view(np.bool_)
        return (tri, t, hit) if want_ids else hit

    def _query_device(self, origin, direction, tmax, m, want_ids, stream):
        import torch
        dev = torch.device("cuda", self.device)

        def rays(x, name, last):
            if not _is_tensor(x):
                raise ValueError(f"{name}: mix of torch tensors and other arrays")
            if x.device != dev:
                raise ValueError(f"{name} must be on {dev} (got {x.device})")
            if x.dtype != torch.float32:
                raise ValueError(f"{name} must be float32 (got {x.dtype})")
            if not x.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if last and (x.dim() != 2 or x.shape[1] != 3):
                raise ValueError(f"{name} must be [n, 3]")
            return x

        o, d = rays(origin, "origin", True), rays(direction, "direction", True)
        if o.shape != d.shape:
            raise ValueError("origin and direction must both be [n, 3]")
        n = o.shape[0]
        tm = None
        if tmax is not None:
            tm = rays(tmax, "tmax", False)
            if tm.dim() != 1 or tm.shape[0] != n:
                raise ValueError("tmax must be [n]")
        hit = torch.empty(n, dtype=torch.bool, device=dev)
        tri = torch.empty(n, dtype=torch.int32, device=dev) if want_ids else None
        t = torch.empty(n, dtype=torch.float32, device=dev) if want_ids else None
        if n:
            s = stream if stream is not None else torch.cuda.current_stream(dev)
            # torch's default stream is the legacy NULL stream, which the ABI reads as "the scene's own stream": run
            # the query on a side stream ordered after `s`, and `s` after it
            side = torch.cuda.Stream(dev) if s.cuda_stream == 0 else None
            run = side if side is not None else s
            if side is not None:
                side.wait_stream(s)
            ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
            self._check(self._lib.vmx_query_device(self._h, m, ptr(o), ptr(d), ptr(tm), n, ptr(tri), ptr(t), ptr(hit),
                                                   C.c_void_p(run.cuda_stream)))
            if side is not None:
                s.wait_stream(side)
        return (tri, t, hit) if want_ids else hit

    # -- changing lights ----------------------------------------------------------
    def set_spheres(self, spheres=None):
        """vmx_scene_set_spheres: replaces the sphere table of the live scene — what Scene(...) takes for it: None (the
        reference's table) or a ctypes array of vmx_sphere (spheres_array / default_spheres; an empty one: no spheres).
        Returns once the table is written; progressive renders begun before it refuse further steps."""
        sp, nsp = _sphere_table(spheres, "spheres")
        self._check(self._lib.vmx_scene_set_spheres(self._h, sp, nsp))
        self._spheres = spheres

    def set_emitters(self, ids=None, radiance=None):
        """vmx_scene_set_emitters: the scene's emissive triangles — ids [n] (createBVH-order triangle ids) and radiance
        [n, 3] (or one rgb for all of them); None or an empty list clears the table.  Only the light-sampled integrator
        (render_nee, radiance_nee, progressive_nee, ...) sees it; progressive renders begun before it refuse further steps."""
        tb, n = emitter_table(ids, radiance)
        self._check(self._lib.vmx_scene_set_emitters(self._h, tb, n))

    def emitters(self):
        """vmx_scene_emitters: the derived table as an EMITTER_DTYPE array (tri_id, radiance, area, weight, cdf), in the
        caller's order, from the scene's current triangle records"""
        n = C.c_uint32(0)
        self._check(self._lib.vmx_scene_emitters(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=EMITTER_DTYPE)
        if n.value:
            self._check(self._lib.vmx_scene_emitters(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    # -- moving geometry --------------------------------------------------------
    def update(self, pos=None, nrm=None, uv=None, rebuild=False, stream=None):
        """In-place update of the same triangles (vmx_scene_update / vmx_scene_update_device; semantics in
        include/vermilion_hip.h): pos / nrm [ntris, 9], uv [ntris, 6]; None keeps that attribute.  rebuild=False
        refits the tree (topology kept, boxes tight over the new positions), True runs the scene's builder again.

        numpy arrays (any float type, converted as at creation) -> the host entry, returns once the scene is updated.
        torch tensors on this scene's device ->
        the device entry on `stream` (default torch.cuda.current_stream()), not synchronised; they must be contiguous
        float32 of exactly those shapes: anything else is a ValueError, never a copy through the host."""
        arrays = {"pos": (pos, 9), "nrm": (nrm, 9), "uv": (uv, 6)}
        given = {k: v for k, v in arrays.items() if v[0] is not None}
        if not given:
            raise ValueError("nothing to update: pos, nrm and uv are all None")
        flags = L.VMX_UPDATE_REBUILD if rebuild else L.VMX_UPDATE_REFIT
        if any(_is_tensor(a) for a, _ in given.values()):
            return self._update_device(given, flags, stream)
        ptrs, keep = {}, []
        for k, (a, w) in given.items():
            a = _f32(a).reshape(-1, w)
            if a.shape[0] != self.ntris:
                raise ValueError(f"{k} must be [{self.ntris}, {w}] (got {list(a.shape)}): another count is a new scene")
            keep.append(a)
            ptrs[k] = a.ctypes.data
        self._check(self._lib.vmx_scene_update(self._h, ptrs.get("pos"), ptrs.get("nrm"), ptrs.get("uv"), self.ntris,
                                               flags))

    def _update_device(self, given, flags, stream):
        import torch
        dev = torch.device("cuda", self.device)
        ptrs = {}
        for k, (a, w) in given.items():
            if not _is_tensor(a):
                raise ValueError(f"{k}: mix of torch tensors and other arrays")
            if a.device != dev:
                raise ValueError(f"{k} must be on {dev} (got {a.device})")
            if a.dtype != torch.float32:
                raise ValueError(f"{k} must be float32 (got {a.dtype})")
            if not a.is_contiguous():
                raise ValueError(f"{k} must be contiguous")
            if tuple(a.shape) != (self.ntris, w):
                raise ValueError(f"{k} must be [{self.ntris}, {w}] (got {list(a.shape)})")
            ptrs[k] = C.c_void_p(a.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        # torch's default stream is the legacy NULL stream, which the ABI reads as "the scene's own stream": run the
        # update on a side stream ordered after `s`, and `s` after it (as Scene.query)
        side = torch.cuda.Stream(dev) if s.cuda_stream == 0 else None
        run = side if side is not None else s
        if side is not None:
            side.wait_stream(s)
        self._check(self._lib.vmx_scene_update_device(self._h, ptrs.get("pos"), ptrs.get("nrm"), ptrs.get("uv"),
                                                      self.ntris, flags, C.c_void_p(run.cuda_stream)))
        if side is not None:
            s.wait_stream(side)

    def primary_ids(self, cam, opts, k=0):
        n = cam.image_res[0] * cam.image_res[1]
        tri = np.empty(n, np.int32)
        t = np.empty(n, np.float32)
        self._check(self._lib.vmx_primary_ids(self._h, C.byref(cam), C.byref(opts), int(k), tri.ctypes.data,
                                        t.ctypes.data))
        return tri, t

    def radiance(self, origin, direction, opts):
        o, d = _f32(origin, 3), _f32(direction, 3)
        n = o.shape[0]
        out = np.empty((n, 4), np.float32)
        st = L.Stats()
        self._check(self._lib.vmx_radiance(self._h, o.ctypes.data, d.ctypes.data, n, C.byref(opts), out.ctypes.data,
                                     C.byref(st)))
        return out, st.as_dict()

    # -- render ---------------------------------------------------------------
    def pixel_claims(self, cam, opts):
        """vmx_pixel_claims: (claims uint32 [local_rows, W], number of claimed pixels) of this camera — per pixel
        0xFFFFFFFF none, 0xFFFFFFFE "no camera ray hits a triangle", else the leaf-order slot of the one triangle every
        camera ray of the pixel hits"""
        rows = local_rows(cam.image_res[1], opts.stripe_rows, opts.rank, opts.world)
        out = np.empty((rows, cam.image_res[0]), np.uint32)
        n = C.c_uint32(0)
        self._check(self._lib.vmx_pixel_claims(self._h, C.byref(cam), C.byref(opts), out.ctypes.data, C.byref(n)))
        return out, int(n.value)

    def fused_camera_paths(self):
        """vmx_fused_camera_paths: the camera paths of the last render on this scene whose rays the shading kernel
        formed and tested itself (claimed pixels of a fused pass)"""
        n = C.c_uint64(0)
        self._check(self._lib.vmx_fused_camera_paths(self._h, C.byref(n)))
        return int(n.value)

    def pixel_claim_lists(self, cam, opts):
        """vmx_pixel_claim_lists: (claims [local_rows, W], list records uint32 [local_rows, W, 4], number of claimed pixels):
        for a pixel without a claim up to four leaf-order slots, padded with 0xFFFFFFFF"""
        rows = local_rows(cam.image_res[1], opts.stripe_rows, opts.rank, opts.world)
        out = np.empty((rows, cam.image_res[0]), np.uint32)
        lists = np.empty((rows, cam.image_res[0], 4), np.uint32)
        n = C.c_uint32(0)
        self._check(self._lib.vmx_pixel_claim_lists(self._h, C.byref(cam), C.byref(opts), out.ctypes.data, lists.ctypes.data,
                                                    C.byref(n)))
        return out, lists, int(n.value)

    def list_settled_rays(self):
        """vmx_list_settled_rays: the camera rays of the last render on this scene that a list claim settled"""
        n = C.c_uint64(0)
        self._check(self._lib.vmx_list_settled_rays(self._h, C.byref(n)))
        return int(n.value)

    def guide_rays(self):
        """vmx_guide_rays: (settled, fallback) bounce rays of the last render on this scene that walked its guide tree"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.vmx_guide_rays(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def guide_fused_rays(self):
        """vmx_guide_fused_rays: (settled, fallback) traversals of the last render's fused launches, whose rays walk the guide tree"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.vmx_guide_fused_rays(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def guide_list_entries(self):
        """vmx_guide_list_entries: entries of the bounce lists the last render handed to the guide form of the trace kernel"""
        n = C.c_uint64(0)
        self._check(self._lib.vmx_guide_list_entries(self._h, C.byref(n)))
        return int(n.value)

    def guide_trace(self, origin, direction, opts=None, records=False, complete=False, grid_blocks=0):
        """vmx_guide_trace (debug entry): the guide form of the bounce traversal kernel on explicit rays.  Returns
        (settled uint8 [n], slot uint32 [n], t float32 [n]): settled 1 where the guided launch settled the ray, slot the
        leaf slot in the scene's tree (bvh()'s prim_order index, 0xFFFFFFFF: no hit).  records: the form that hands the
        rays on as dense records; complete: the launch over the fallback list follows, so every ray has its answer
        (else a fallback ray has slot 0xFFFFFFFF, t 0); grid_blocks: cap of the guided launch's blocks (0: a render's)."""
        o, d = _f32(origin, 3), _f32(direction, 3)
        n = o.shape[0]
        if opts is None:
            opts = make_opts()
        settled = np.zeros(n, np.uint8)
        slot = np.full(n, 0xFFFFFFFF, np.uint32)
        t = np.zeros(n, np.float32)
        flags = (1 if records else 0) | (2 if complete else 0)
        self._check(self._lib.vmx_guide_trace(self._h, o.ctypes.data, d.ctypes.data, n, C.byref(opts), flags, int(grid_blocks),
                                              settled.ctypes.data, slot.ctypes.data, t.ctypes.data))
        return settled, slot, t

    def guide_trace_visits(self, origin, direction, opts=None, complete=False, grid_blocks=0):
        """vmx_guide_trace_visits (debug entry): guide_trace through the kernel's counting form.  Returns (settled, slot, t,
        inner_visits uint32 [n], tri_tests uint32 [n]): the inner records and triangle tests of every ray's guide walk."""
        o, d = _f32(origin, 3), _f32(direction, 3)
        n = o.shape[0]
        if opts is None:
            opts = make_opts()
        settled = np.zeros(n, np.uint8)
        slot = np.full(n, 0xFFFFFFFF, np.uint32)
        t = np.zeros(n, np.float32)
        nv, nt = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._check(self._lib.vmx_guide_trace_visits(self._h, o.ctypes.data, d.ctypes.data, n, C.byref(opts), 2 if complete else 0,
                                                     int(grid_blocks), settled.ctypes.data, slot.ctypes.data, t.ctypes.data,
                                                     nv.ctypes.data, nt.ctypes.data))
        return settled, slot, t, nv, nt

    def render(self, cam, opts):
        """PathTracer::Render into a host array [local_rows, W, 5] (RGBAZ)."""
        rows = local_rows(cam.image_res[1], opts.stripe_rows, opts.rank, opts.world)
        out = np.empty((rows, cam.image_res[0], 5), np.float32)
        st = L.Stats()
        self._check(self._lib.vmx_render(self._h, C.byref(cam), C.byref(opts), out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def progressive(self, cam, opts, stream=None, moments=False):
        """vmx_progressive_begin: the frame `render(cam, opts)` returns, rendered in resumable steps with previews in
        between (a context-managed Progressive).  stream: a torch stream the passes and previews run on (default: the
        scene's own stream).  moments (vmx_progressive_begin_ex, VMX_PROGRESSIVE_MOMENTS): the handle also keeps the
        second moment of every pixel's luminance, which `error_device`, `select_device` and `step_adaptive` need."""
        return Progressive(self, cam, opts, stream, moments)

    def render_bruteforce(self, cam, opts, flags=0):
        """BruteForceTracer::Render (core/integrators/integrators.cpp:9-186) into a host array
        [local_rows, W, 5]: r, g, b, alpha = hit fraction, depth = last sample's hit distance."""
        rows = local_rows(cam.image_res[1], opts.stripe_rows, opts.rank, opts.world)
        out = np.empty((rows, cam.image_res[0], 5), np.float32)
        st = L.Stats()
        self._check(self._lib.vmx_render_bruteforce(self._h, C.byref(cam), C.byref(opts), int(flags), out.ctypes.data,
                                              C.byref(st)))
        return out, st.as_dict()

    def render_device(self, cam, opts, d_out_ptr, stream_ptr=None):
        """Same, into device memory (e.g. a torch tensor's data_ptr()) on `stream_ptr`."""
        st = L.Stats()
        self._check(self._lib.vmx_render_device(self._h, C.byref(cam), C.byref(opts), C.c_void_p(d_out_ptr),
                                          C.c_void_p(stream_ptr or 0), C.byref(st)))
        return st.as_dict()

    # -- light sampling -----------------------------------------------------------
    def render_nee(self, cam, opts):
        """vmx_render_nee: the path integrator with next-event estimation (opts.sampling: VMX_SAMPLING_CORRECTED, no
        early stop) into a host array [H, W, 5] (RGBAZ, the fifth float the sample count)."""
        out = np.empty((cam.image_res[1], cam.image_res[0], 5), np.float32)
        st = L.Stats()
        self._check(self._lib.vmx_render_nee(self._h, C.byref(cam), C.byref(opts), out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def progressive_nee(self, cam, opts, stream=None, moments=False, rank=False):
        """vmx_progressive_begin_nee: the frame `render_nee(cam, opts)` returns, rendered in resumable steps (a
        context-managed Progressive whose passes run the light-sampling integrator).  Every method of Progressive works on
        it; `budget_device`, `step_budget` and `step_budgeted` work on such a handle only.  rank
        (vmx_progressive_begin_nee_rank): opts.world > 1 is accepted and the handle holds `render_nee_rank`'s rows; its
        planes, maps and budgets are indexed by local pixel and their windows stop at the rank's own rows."""
        return Progressive(self, cam, opts, stream, moments, nee=True, rank=rank)

    def render_nee_device(self, cam, opts, d_out_ptr, stream_ptr=None):
        """Same, into device memory (e.g. a torch tensor's data_ptr()) on `stream_ptr`."""
        st = L.Stats()
        self._check(self._lib.vmx_render_nee_device(self._h, C.byref(cam), C.byref(opts), C.c_void_p(d_out_ptr), C.byref(st),
                                                    C.c_void_p(stream_ptr or 0)))
        return st.as_dict()

    def radiance_nee(self, origin, direction, opts):
        """vmx_radiance_nee: light-sampled Radiance of explicit camera rays, ray i on stream (seed, i, 0): unclamped
        accumColour [n, 4] (w: the primary hit distance) and the call's statistics."""
        o, d = _f32(origin, 3), _f32(direction, 3)
        n = o.shape[0]
        out = np.empty((n, 4), np.float32)
        st = L.Stats()
        self._check(self._lib.vmx_radiance_nee(self._h, o.ctypes.data, d.ctypes.data, n, C.byref(opts), out.ctypes.data,
                                               C.byref(st)))
        return out, st.as_dict()

    def radiance_nee_device(self, d_origin_ptr, d_dir_ptr, n, opts, d_out4_ptr, stream_ptr=None):
        """vmx_radiance_nee_device: `radiance_nee` on device arrays of the scene's device (n x 3 floats each, the result
        n x 4 floats, 16-byte aligned), enqueued on `stream_ptr` (default: the scene's stream); blocks until the batch is
        done and returns its statistics."""
        st = L.Stats()
        self._check(self._lib.vmx_radiance_nee_device(self._h, C.c_void_p(d_origin_ptr), C.c_void_p(d_dir_ptr), int(n),
                                                      C.byref(opts), C.c_void_p(d_out4_ptr), C.byref(st),
                                                      C.c_void_p(stream_ptr or 0)))
        return st.as_dict()

    def render_nee_rank(self, cam, opts):
        """vmx_render_nee_rank: the rows of `render_nee`'s frame that (opts.rank, opts.world, opts.stripe_rows) owns, packed in
        ascending order into a host array [local_rows, W, 5]; the statistics cover those pixels only."""
        rows = local_rows(cam.image_res[1], opts.stripe_rows, opts.rank, opts.world)
        n = rows * cam.image_res[0] * 5
        buf = np.empty(max(n, 1), np.float32)  # (a rank without rows still hands the entry a pointer)
        st = L.Stats()
        self._check(self._lib.vmx_render_nee_rank(self._h, C.byref(cam), C.byref(opts), buf.ctypes.data, C.byref(st)))
        return buf[:n].reshape(rows, cam.image_res[0], 5), st.as_dict()

    def render_nee_rank_device(self, cam, opts, d_out_ptr, stream_ptr=None):
        """Same, into device memory (local_rows * W * 5 floats) on `stream_ptr`; a rank that owns no row writes nothing."""
        st = L.Stats()
        self._check(self._lib.vmx_render_nee_rank_device(self._h, C.byref(cam), C.byref(opts), C.c_void_p(d_out_ptr),
                                                         C.byref(st), C.c_void_p(stream_ptr or 0)))
        return st.as_dict()


class Progressive:
    """One vmx_progressive handle: `step` issues samples, `preview` shows the frame so far, and the frame a completed
    handle previews is `Scene.render`'s, bit for bit, whatever the steps were."""

    def __init__(self, scene, cam, opts, stream=None, moments=False, nee=False, rank=False):
        self._scene = scene  # (keeps the scene alive: it cannot be destroyed before its handles)
        self.moments = bool(moments)
        self.nee = bool(nee)
        self._lib = scene._lib
        self._h = None
        self.device = scene.device
        self._stream = stream
        rows = local_rows(cam.image_res[1], opts.stripe_rows, opts.rank, opts.world)
        self.shape = (rows, int(cam.image_res[0]))
        h = C.c_void_p()
        sptr = C.c_void_p(stream.cuda_stream if stream is not None else 0)
        if rank and not nee:
            raise ValueError("rank=True is the light-sampled handle's rank form: a plain handle takes opts.world > 1 as it is")
        if nee:
            begin = self._lib.vmx_progressive_begin_nee_rank if rank else self._lib.vmx_progressive_begin_nee
            scene._check(begin(scene._h, C.byref(cam), C.byref(opts), L.VMX_PROGRESSIVE_MOMENTS if moments else 0, sptr,
                               C.byref(h)))
        elif moments:
            scene._check(self._lib.vmx_progressive_begin_ex(scene._h, C.byref(cam), C.byref(opts), L.VMX_PROGRESSIVE_MOMENTS,
                                                            sptr, C.byref(h)))
        else:
            scene._check(self._lib.vmx_progressive_begin(scene._h, C.byref(cam), C.byref(opts), sptr, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._scene._check(self._lib.vmx_progressive_end(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def step(self, samples=0):
        """up to `samples` more samples per pixel (0: run to completion); blocks; this step's vmx_stats as a dict"""
        st = L.Stats()
        self._scene._check(self._lib.vmx_progressive_step(self._h, int(samples), C.byref(st)))
        return st.as_dict()

    def _plane(self, x, name, dtype, last=None):
        """a torch tensor of the handle's local image ([rows, W] or [rows, W, last]) on its device, or a ValueError"""
        import torch
        return _frame_tensor(x, name, dtype, self.shape + (() if last is None else (last,)), torch.device("cuda", self.device))

    def state_device(self, sums=None, counts=None):
        """vmx_progressive_state_device: the raw per-pixel state into torch tensors on the scene's device — sums float32
        [local_rows, W, 4] (r, g, b sums; w = the sum of squared luminances on a moments handle, else 0) and / or counts
        int32 [local_rows, W].  Enqueued on the handle's stream, nothing synchronised; returns (sums, counts)."""
        import torch
        if sums is None and counts is None:
            raise ValueError("no output: sums and counts are both None")
        if sums is not None:
            self._plane(sums, "sums", torch.float32, 4)
        if counts is not None:
            self._plane(counts, "counts", torch.int32)
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        self._scene._check(self._lib.vmx_progressive_state_device(self._h, ptr(sums), ptr(counts)))
        return sums, counts

    def step_selected(self, samples, select):
        """vmx_progressive_step_selected_device: a step in which only the pixels with select != 0 take samples (select: a
        torch uint8 or bool tensor [local_rows, W] on the scene's device; 0 samples: the selected pixels run to kmax).
        Blocks; returns (this step's vmx_stats as a dict, the number of pixels that took samples)."""
        import torch
        self._plane(select, "select", torch.bool if select is not None and _is_tensor(select) and select.dtype == torch.bool else torch.uint8)
        st, n = L.Stats(), C.c_uint32(0)
        self._scene._check(self._lib.vmx_progressive_step_selected_device(self._h, int(samples), C.c_void_p(select.data_ptr()),
                                                                          C.byref(st), C.byref(n)))
        return st.as_dict(), int(n.value)

    def error_device(self, error=None, variance=None, params=None):
        """vmx_progressive_error_device (a moments handle): the relative standard error of every pixel's mean luminance
        and / or the variance of that mean — what Filter.apply(variance=...) reads — into float32 tensors [local_rows, W].
        params: make_sampling_params(...), default the library's (only `floor` matters here).  Returns (error, variance)."""
        import torch
        if error is None and variance is None:
            raise ValueError("no output: error and variance are both None")
        if error is not None:
            self._plane(error, "error", torch.float32)
        if variance is not None:
            self._plane(variance, "variance", torch.float32)
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        prm = None if params is None else C.byref(params)
        self._scene._check(self._lib.vmx_progressive_error_device(self._h, prm, ptr(error), ptr(variance)))
        return error, variance

    def select_device(self, select, count=None, params=None):
        """vmx_progressive_select_device (a moments handle): select[p] = 1 where pixel p is unfinished and has fewer than
        min_samples samples or an error above the threshold within `radius` pixels, else 0 (uint8 [local_rows, W]); count:
        an int32 tensor of one element that receives the number of selected pixels.  Returns (select, count)."""
        import torch
        self._plane(select, "select", torch.uint8)
        if count is not None:
            _frame_tensor(count, "count", torch.int32, (1,), torch.device("cuda", self.device))
        prm = None if params is None else C.byref(params)
        self._scene._check(self._lib.vmx_progressive_select_device(self._h, prm, C.c_void_p(select.data_ptr()),
                                                                   None if count is None else C.c_void_p(count.data_ptr())))
        return select, count

    def step_adaptive(self, samples, params=None):
        """vmx_progressive_step_adaptive (a moments handle): `select_device` into a map of the handle's, then
        `step_selected` with it.  Blocks; returns (this step's vmx_stats as a dict, the number of pixels that took samples)."""
        st, n = L.Stats(), C.c_uint32(0)
        prm = None if params is None else C.byref(params)
        self._scene._check(self._lib.vmx_progressive_step_adaptive(self._h, int(samples), prm, C.byref(st), C.byref(n)))
        return st.as_dict(), int(n.value)

    def budget_device(self, budget, total=None, params=None):
        """vmx_progressive_budget_device (a light-sampled moments handle): budget[p] = the samples pixel p's error asks
        for (int32 [local_rows, W], read as uint32); total: an int64 tensor of one element that receives their sum.
        params: make_sampling_budget_params(...).  Enqueued on the handle's stream; returns (budget, total)."""
        import torch
        self._plane(budget, "budget", torch.int32)
        if total is not None:
            _frame_tensor(total, "total", torch.int64, (1,), torch.device("cuda", self.device))
        prm = None if params is None else C.byref(params)
        self._scene._check(self._lib.vmx_progressive_budget_device(self._h, prm, C.c_void_p(budget.data_ptr()),
                                                                   None if total is None else C.c_void_p(total.data_ptr())))
        return budget, total

    def step_budget(self, budget):
        """vmx_progressive_step_budget_device (a light-sampled handle): every active pixel p takes min(budget[p], samples
        per batch, kmax - its count) samples in one pass (budget: int32 [local_rows, W] on the scene's device).  Blocks;
        returns (this step's vmx_stats as a dict, the number of pixels that took samples)."""
        import torch
        self._plane(budget, "budget", torch.int32)
        st, n = L.Stats(), C.c_uint32(0)
        self._scene._check(self._lib.vmx_progressive_step_budget_device(self._h, C.c_void_p(budget.data_ptr()), C.byref(st),
                                                                        C.byref(n)))
        return st.as_dict(), int(n.value)

    def step_budgeted(self, params=None):
        """vmx_progressive_step_budgeted (a light-sampled moments handle): `budget_device` into a plane of the handle's,
        then `step_budget` with it.  Blocks; returns (this step's vmx_stats as a dict, the pixels that took samples)."""
        st, n = L.Stats(), C.c_uint32(0)
        prm = None if params is None else C.byref(params)
        self._scene._check(self._lib.vmx_progressive_step_budgeted(self._h, prm, C.byref(st), C.byref(n)))
        return st.as_dict(), int(n.value)

    def info(self):
        i = L.ProgressiveInfo()
        self._scene._check(self._lib.vmx_progressive_info_get(self._h, C.byref(i)))
        return i.as_dict()

    def preview(self, rgba8=False):
        """the frame so far as a host array [local_rows, W, 5] (RGBAZ, depth = samples taken); rgba8=True: also its
        [local_rows, W, 4] uint8 form, from the same launch"""
        out = np.empty(self.shape + (5,), np.float32)
        q = np.empty(self.shape + (4,), np.uint8) if rgba8 else None
        self._scene._check(self._lib.vmx_progressive_preview(self._h, out.ctypes.data, None if q is None else q.ctypes.data))
        return (out, q) if rgba8 else out

    def preview_device(self, rgbaz=None, rgba8=None):
        """vmx_progressive_preview_device into torch tensors on the scene's device: rgbaz float32 [local_rows, W, 5]
        and / or rgba8 uint8 [local_rows, W, 4], contiguous — anything else is a ValueError, never a copy through the
        host.  Enqueued on the handle's stream, nothing synchronised; returns (rgbaz, rgba8)."""
        import torch
        if rgbaz is None and rgba8 is None:
            raise ValueError("no output: rgbaz and rgba8 are both None")
        dev = torch.device("cuda", self.device)
        for x, name, dtype, last in ((rgbaz, "rgbaz", torch.float32, 5), (rgba8, "rgba8", torch.uint8, 4)):
            if x is None:
                continue
            if not _is_tensor(x):
                raise ValueError(f"{name} must be a torch tensor")
            if x.dtype != dtype:
                raise ValueError(f"{name} must be {dtype} (got {x.dtype})")
            if tuple(x.shape) != self.shape + (last,):
                raise ValueError(f"{name} must be {list(self.shape + (last,))} (got {list(x.shape)})")
            if not x.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if x.device != dev:
                raise ValueError(f"{name} must be on {dev} (got {x.device})")
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        self._scene._check(self._lib.vmx_progressive_preview_device(self._h, ptr(rgbaz), ptr(rgba8)))
        return rgbaz, rgba8

    def preview_filtered(self, rgba8=False, params=None, albedo_samples=None):
        """vmx_progressive_preview_filtered: `preview`'s frame pushed through the G-buffer-guided filter (guide: sample
        0's camera ray of every pixel, built on the first call), as host arrays like `preview`'s.  params:
        make_filter_params(...), default the library's.  albedo_samples (vmx_progressive_preview_demodulated): filter
        colour / albedo and multiply the albedo back, with the handle's albedo plane of that many samples (built on
        the first such call, again when the number changes); None is the call without."""
        if albedo_samples is not None and int(albedo_samples) < 1:
            raise ValueError("albedo_samples must be at least 1")
        out = np.empty(self.shape + (5,), np.float32)
        q = np.empty(self.shape + (4,), np.uint8) if rgba8 else None
        prm = None if params is None else C.byref(params)
        if albedo_samples is None:
            self._scene._check(self._lib.vmx_progressive_preview_filtered(self._h, out.ctypes.data,
                                                                          None if q is None else q.ctypes.data, prm))
        else:
            self._scene._check(self._lib.vmx_progressive_preview_demodulated(self._h, out.ctypes.data,
                                                                             None if q is None else q.ctypes.data, prm,
                                                                             int(albedo_samples)))
        return (out, q) if rgba8 else out

    def preview_filtered_device(self, rgbaz=None, rgba8=None, params=None, albedo_samples=None):
        """vmx_progressive_preview_filtered_device into torch tensors, checked as `preview_device` checks its own.
        Enqueued on the handle's stream, nothing synchronised (but the first filtered preview of a handle builds its
        guide and blocks until that is done); returns (rgbaz, rgba8).  albedo_samples: as in `preview_filtered`
        (vmx_progressive_preview_demodulated_device)."""
        import torch
        if albedo_samples is not None and int(albedo_samples) < 1:
            raise ValueError("albedo_samples must be at least 1")
        if rgbaz is None and rgba8 is None:
            raise ValueError("no output: rgbaz and rgba8 are both None")
        dev = torch.device("cuda", self.device)
        if rgbaz is not None:
            _frame_tensor(rgbaz, "rgbaz", torch.float32, self.shape + (5,), dev)
        if rgba8 is not None:
            _frame_tensor(rgba8, "rgba8", torch.uint8, self.shape + (4,), dev)
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        prm = None if params is None else C.byref(params)
        if albedo_samples is None:
            self._scene._check(self._lib.vmx_progressive_preview_filtered_device(self._h, ptr(rgbaz), ptr(rgba8), prm))
        else:
            self._scene._check(self._lib.vmx_progressive_preview_demodulated_device(self._h, ptr(rgbaz), ptr(rgba8), prm,
                                                                                    int(albedo_samples)))
        return rgbaz, rgba8


class MultiScene:
    """One process, several devices (vmx_multi_*): scene replicas render interleaved stripes, the packed
    stripes are gathered device-to-device on devices[0] and de-interleaved there."""

    def __init__(self, pos, nrm, uv=None, devices=(0,), spheres=None, leaf_size=4, builder=L.VMX_BVH_REFERENCE):
        pos = _f32(pos).reshape(-1, 9)
        nrm = _f32(nrm).reshape(-1, 9)
        uvp = None
        if uv is not None:
            uv = _f32(uv).reshape(-1, 6)
            uvp = uv.ctypes.data
        self._spheres = spheres
        sp, nsp = (None, 0) if spheres is None else (C.addressof(spheres), len(spheres))
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        L.check(L.lib().vmx_multi_create(pos.ctypes.data, nrm.ctypes.data, uvp, pos.shape[0], sp, nsp, int(leaf_size),
                                         int(builder), devs, len(devices), C.byref(h)))
        self._h = h
        self.ntris = pos.shape[0]
        self.world = L.lib().vmx_multi_world(h)

    def close(self):
        if getattr(self, "_h", None):
            L.lib().vmx_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def routes(self):
        """[(device, route)] per replica: route 2 = the root's own device, 1 = direct peer copy, 0 = staged through the host"""
        d, r = (C.c_int * self.world)(), (C.c_int * self.world)()
        L.check(L.lib().vmx_multi_routes(self._h, d, r))
        return list(zip(list(d), list(r)))

    def timings(self):
        """the exchange step of the last render, timed apart from the rendering (vmx_multi_timings)"""
        t = L.MultiTimes()
        r, c = (C.c_double * self.world)(), (C.c_double * self.world)()
        L.check(L.lib().vmx_multi_timings(self._h, C.byref(t), r, c))
        d = {k: getattr(t, k) for k, _ in t._fields_ if k != "pad"}
        d["render_ms"], d["copy_ms"] = list(r), list(c)
        return d

    def bind_texture(self, data):
        data = np.ascontiguousarray(data, dtype=np.float32)
        c = 1 if data.ndim == 2 else data.shape[2]
        L.check(L.lib().vmx_multi_bind_texture(self._h, data.ctypes.data, data.shape[1], data.shape[0], c))

    def set_emitters(self, ids=None, radiance=None):
        """vmx_multi_set_emitters: Scene.set_emitters on every replica"""
        tb, n = emitter_table(ids, radiance)
        L.check(L.lib().vmx_multi_set_emitters(self._h, tb, n))

    def set_spheres(self, spheres=None):
        """vmx_multi_set_spheres: Scene.set_spheres on every replica"""
        sp, nsp = _sphere_table(spheres, "spheres")
        L.check(L.lib().vmx_multi_set_spheres(self._h, sp, nsp))
        self._spheres = spheres

    def update(self, pos=None, nrm=None, uv=None, rebuild=False):
        """vmx_multi_update: Scene.update's host entry on every replica (numpy arrays; None keeps that attribute)"""
        ptrs, keep = {}, []
        for k, a, w in (("pos", pos, 9), ("nrm", nrm, 9), ("uv", uv, 6)):
            if a is None:
                continue
            a = _f32(a).reshape(-1, w)
            if a.shape[0] != self.ntris:
                raise ValueError(f"{k} must be [{self.ntris}, {w}] (got {list(a.shape)}): another count is a new scene")
            keep.append(a)
            ptrs[k] = a.ctypes.data
        if not ptrs:
            raise ValueError("nothing to update: pos, nrm and uv are all None")
        L.check(L.lib().vmx_multi_update(self._h, ptrs.get("pos"), ptrs.get("nrm"), ptrs.get("uv"), self.ntris,
                                         L.VMX_UPDATE_REBUILD if rebuild else L.VMX_UPDATE_REFIT))

    def render(self, cam, opts):
        out = np.empty((cam.image_res[1], cam.image_res[0], 5), np.float32)
        st = L.Stats()
        L.check(L.lib().vmx_multi_render(self._h, C.byref(cam), C.byref(opts), out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def render_device(self, cam, opts, d_out_ptr):
        st = L.Stats()
        L.check(L.lib().vmx_multi_render_device(self._h, C.byref(cam), C.byref(opts), C.c_void_p(d_out_ptr), C.byref(st)))
        return st.as_dict()

    def render_bruteforce(self, cam, opts, flags=0):
        out = np.empty((cam.image_res[1], cam.image_res[0], 5), np.float32)
        st = L.Stats()
        L.check(L.lib().vmx_multi_render_bruteforce(self._h, C.byref(cam), C.byref(opts), int(flags), out.ctypes.data,
                                                    C.byref(st)))
        return out, st.as_dict()

    def render_nee(self, cam, opts):
        """vmx_multi_render_nee: `Scene.render_nee`'s frame, each replica rendering its stripes; opts.world must be 0 or 1"""
        out = np.empty((cam.image_res[1], cam.image_res[0], 5), np.float32)
        st = L.Stats()
        L.check(L.lib().vmx_multi_render_nee(self._h, C.byref(cam), C.byref(opts), out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def render_nee_device(self, cam, opts, d_out_ptr):
        """Same, into device memory on devices[0]"""
        st = L.Stats()
        L.check(L.lib().vmx_multi_render_nee_device(self._h, C.byref(cam), C.byref(opts), C.c_void_p(d_out_ptr), C.byref(st)))
        return st.as_dict()


EMITTER_DTYPE = np.dtype([("tri_id", np.uint32), ("radiance", np.float32, 3), ("area", np.float64), ("weight", np.float64),
                          ("cdf", np.float64)])
assert EMITTER_DTYPE.itemsize == C.sizeof(L.EmitterInfo) == 40


def emitter_table(ids, radiance):
    """(ctypes array of vmx_emitter or None, n) from ids [n] and radiance [n, 3] or [3]"""
    if ids is None or len(ids) == 0:
        return None, 0
    ids = np.asarray(ids, np.int64).reshape(-1)
    rad = np.broadcast_to(np.asarray(radiance, np.float32).reshape(-1, 3), (ids.size, 3))
    if ids.min() < 0 or ids.max() > 0xFFFFFFFF:
        raise ValueError("emitter ids must be triangle ids")
    rec = np.empty(ids.size, dtype=[("tri_id", np.uint32), ("radiance", np.float32, 3)])
    rec["tri_id"], rec["radiance"] = ids, rad
    return (L.Emitter * ids.size).from_buffer_copy(rec.tobytes()), ids.size


RAYHIT_DTYPE = np.dtype([
    ("location", np.float32, 3), ("distance", np.float32), ("normal", np.float32, 3), ("tri_id", np.int32),
    ("uv", np.float32, 2), ("tri_t", np.float32), ("flags", np.uint32), ("colour", np.float32, 3),
    ("pad", np.uint32),
])
assert RAYHIT_DTYPE.itemsize == 64

MOTION_DTYPE = np.dtype([
    ("prev_location", np.float32, 3), ("flags", np.uint32), ("prev_normal", np.float32, 3), ("pad", np.uint32),
])
assert MOTION_DTYPE.itemsize == 32


def local_rows(height, stripe_rows, rank, world):
    r = C.c_uint32(0)
    L.check(L.lib().vmx_local_rows(int(height), int(stripe_rows), int(rank), int(world), C.byref(r)))
    return r.value


def local_row_indices(height, stripe_rows, rank, world):
    """global row index of every local row of (rank, world) — pure host logic"""
    stripe_rows = stripe_rows or 16
    if world <= 1:
        return np.arange(height)
    rows = []
    n_stripes = (height + stripe_rows - 1) // stripe_rows
    for s in range(rank, n_stripes, world):
        rows.extend(range(s * stripe_rows, min((s + 1) * stripe_rows, height)))
    return np.asarray(rows, dtype=np.int64)


from .image import Filter, Temporal, Upsample  # noqa: E402,F401  (they import this module's helpers: after them)
