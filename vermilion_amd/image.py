"""The image-space passes over the C ABI: `Filter` (vmx_filter_*), `Upsample` (vmx_upsample_*) and `Temporal`
(vmx_temporal_*), one handle each.

torch tensors on the handle's device in and out; all compute happens in libvermilion_hip.so.
"""
import ctypes as C

from . import _lib as L
from .scene import _SideStream, _albedo_tensor, _frame_tensor


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _out_pair(out, rgba8, shape, dev):
    """the `out` (float32 shape + [5]) / `rgba8` (uint8 shape + [4]) pair of an apply or accumulate as the ABI takes it,
    or a ValueError; with neither given, a new `out` is made"""
    import torch
    if out is None and rgba8 is None:
        out = torch.empty(shape + (5,), dtype=torch.float32, device=dev)
    if out is not None:
        _frame_tensor(out, "out", torch.float32, shape + (5,), dev)
    if rgba8 is not None:
        _frame_tensor(rgba8, "rgba8", torch.uint8, shape + (4,), dev)
    return out, rgba8


class _Handle:
    """One handle of the C ABI on `device`: `_h` from the subclass's create entry, given back to `_destroy` (the destroy
    entry's name) by `close`, by leaving a `with` block, or when the object dies."""
    _destroy = None

    def __init__(self, device, lib):
        self._lib = lib if lib is not None else L.lib()
        self._h = None
        self.device = int(device)

    def _check(self, code):
        if code != L.VMX_OK:
            raise L.VmxError(code, self._lib.vmx_last_error().decode("utf-8", "replace"))

    def close(self):
        if getattr(self, "_h", None):
            self._check(getattr(self._lib, self._destroy)(self._h))
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


class Filter(_Handle):
    """One vmx_filter handle: the G-buffer-guided a-trous filter (include/vermilion_hip.h) for [height, width] frames on
    `device`.  `set_guide` takes a camera raycast's records, `apply` filters RGBAZ frames with it."""
    _destroy = "vmx_filter_destroy"

    def __init__(self, width, height, device=0, lib=None):
        super().__init__(device, lib)
        self.shape = (int(height), int(width))
        h = C.c_void_p()
        self._check(self._lib.vmx_filter_create(self.device, int(width), int(height), C.byref(h)))
        self._h = h

    def set_guide(self, raw, stream=None):
        """vmx_filter_set_guide_device: `raw` is the ["raw"] tensor of Scene.raycast_camera, or any contiguous float32
        [height, width, 16] tensor of vmx_rayhit records on the filter's device — anything else is a ValueError.
        Enqueued on `stream` (default torch.cuda.current_stream()), nothing synchronised."""
        import torch
        dev = torch.device("cuda", self.device)
        _frame_tensor(raw, "raw", torch.float32, self.shape + (16,), dev)
        with _SideStream(dev, stream) as run:
            self._check(self._lib.vmx_filter_set_guide_device(self._h, C.c_void_p(raw.data_ptr()),
                                                              C.c_void_p(run.cuda_stream)))

    def apply(self, rgbaz, out=None, rgba8=None, params=None, stream=None, albedo=None, variance=None,
              sigma_luminance=L.VMX_SIGMA_LUMINANCE_DEFAULT):
        """vmx_filter_apply_device: filters the float32 [height, width, 5] frame `rgbaz` into `out` (same shape; may be
        `rgbaz` itself) and / or `rgba8` (uint8 [height, width, 4]); with neither given, a new `out` is made.  All are
        contiguous torch tensors on the filter's device: anything else is a ValueError, never a copy through the host.
        params: make_filter_params(...), default the library's.  `albedo` (vmx_filter_apply_demodulated_device): what
        Scene.albedo_camera made for the frame's camera, float32 [height, width, 4], 16-byte aligned, read only — the
        filter then works on colour / albedo and multiplies the albedo back, so textures survive; None is the call
        without.  `variance` (vmx_filter_apply_variance_device): what Temporal.accumulate(..., variance=...) wrote for this
        frame, float32 [height, width], read only — the colour stop is then the luminance difference in standard
        deviations, `sigma_luminance` of them (params.sigma_colour is not used); it composes with `albedo`.
        Enqueued on `stream` (default torch.cuda.current_stream()), nothing synchronised; returns (out, rgba8)."""
        import torch
        dev = torch.device("cuda", self.device)
        _frame_tensor(rgbaz, "rgbaz", torch.float32, self.shape + (5,), dev)
        if albedo is not None:
            _albedo_tensor(albedo, "albedo", self.shape, dev)
        if variance is not None:
            _frame_tensor(variance, "variance", torch.float32, self.shape, dev)
            sigma_luminance = float(sigma_luminance)
            if not (0.0 < sigma_luminance < float("inf")):
                raise ValueError("sigma_luminance must be finite and > 0")
        out, rgba8 = _out_pair(out, rgba8, self.shape, dev)
        with _SideStream(dev, stream) as run:
            prm, s = None if params is None else C.byref(params), C.c_void_p(run.cuda_stream)
            if variance is not None:
                self._check(self._lib.vmx_filter_apply_variance_device(self._h, _ptr(rgbaz), _ptr(variance), _ptr(albedo),
                                                                       _ptr(out), _ptr(rgba8), prm, sigma_luminance, s))
            elif albedo is None:
                self._check(self._lib.vmx_filter_apply_device(self._h, _ptr(rgbaz), _ptr(out), _ptr(rgba8), prm, s))
            else:
                self._check(self._lib.vmx_filter_apply_demodulated_device(self._h, _ptr(rgbaz), _ptr(albedo), _ptr(out),
                                                                          _ptr(rgba8), prm, s))
        return out, rgba8


class Upsample(_Handle):
    """One vmx_upsample handle: G-buffer-guided upsampling (include/vermilion_hip.h) of [low_height, low_width] frames to
    [height, width] frames on `device`.  `set_guides` takes the camera raycasts' records of both sizes, `apply`
    reconstructs RGBAZ frames with them."""
    _destroy = "vmx_upsample_destroy"

    def __init__(self, low_width, low_height, width, height, device=0, lib=None):
        super().__init__(device, lib)
        self.low_shape = (int(low_height), int(low_width))
        self.shape = (int(height), int(width))
        h = C.c_void_p()
        self._check(self._lib.vmx_upsample_create(self.device, int(low_width), int(low_height), int(width), int(height),
                                                  C.byref(h)))
        self._h = h

    def set_guides(self, raw_low, raw_full, stream=None):
        """vmx_upsample_set_guides_device: the ["raw"] tensors of Scene.raycast_camera for low_camera(cam, ...) and for
        cam, or any contiguous float32 [low_height, low_width, 16] and [height, width, 16] tensors of vmx_rayhit records
        on the handle's device — anything else is a ValueError.  Enqueued on `stream` (default
        torch.cuda.current_stream()), nothing synchronised."""
        import torch
        dev = torch.device("cuda", self.device)
        _frame_tensor(raw_low, "raw_low", torch.float32, self.low_shape + (16,), dev)
        _frame_tensor(raw_full, "raw_full", torch.float32, self.shape + (16,), dev)
        with _SideStream(dev, stream) as run:
            self._check(self._lib.vmx_upsample_set_guides_device(self._h, C.c_void_p(raw_low.data_ptr()),
                                                                 C.c_void_p(raw_full.data_ptr()),
                                                                 C.c_void_p(run.cuda_stream)))

    def apply(self, frame_low, out=None, rgba8=None, params=None, stream=None):
        """vmx_upsample_apply_device: reconstructs the float32 [low_height, low_width, 5] frame `frame_low` into `out`
        (float32 [height, width, 5]) and / or `rgba8` (uint8 [height, width, 4]); with neither given, a new `out` is
        made.  All are contiguous torch tensors on the handle's device: anything else is a ValueError, never a copy
        through the host.  params: make_upsample_params(...), default the library's.  Enqueued on `stream` (default
        torch.cuda.current_stream()), nothing synchronised; returns `out` (None where only `rgba8` was asked for)."""
        import torch
        dev = torch.device("cuda", self.device)
        _frame_tensor(frame_low, "frame_low", torch.float32, self.low_shape + (5,), dev)
        out, rgba8 = _out_pair(out, rgba8, self.shape, dev)
        with _SideStream(dev, stream) as run:
            self._check(self._lib.vmx_upsample_apply_device(self._h, _ptr(frame_low), _ptr(out), _ptr(rgba8),
                                                            None if params is None else C.byref(params),
                                                            C.c_void_p(run.cuda_stream)))
        return out


class Temporal(_Handle):
    """One vmx_temporal handle: temporal accumulation (include/vermilion_hip.h) of [height, width] frames on `device`.
    `accumulate` reprojects the frames accumulated so far into the new camera through the new frame's G-buffer and
    blends the new frame in; `reset` forgets them.  moments=True (vmx_temporal_create_ex with VMX_TEMPORAL_MOMENTS): the
    handle also carries the luminance's first and second moment, and every `accumulate` writes a per-pixel variance."""
    _destroy = "vmx_temporal_destroy"

    def __init__(self, width, height, device=0, lib=None, moments=False):
        super().__init__(device, lib)
        self.shape = (int(height), int(width))
        self.moments = bool(moments)
        h = C.c_void_p()
        if self.moments:
            self._check(self._lib.vmx_temporal_create_ex(self.device, int(width), int(height), L.VMX_TEMPORAL_MOMENTS,
                                                         C.byref(h)))
        else:
            self._check(self._lib.vmx_temporal_create(self.device, int(width), int(height), C.byref(h)))
        self._h = h

    def accumulate(self, cam, raw, rgbaz, out=None, rgba8=None, history=None, params=None, stream=None, motion=None,
                   variance=None, variance_params=None, adaptive=None, change=None):
        """vmx_temporal_accumulate_device: one frame.  `cam` is that frame's camera (make_camera), `raw` its G-buffer —
        the ["raw"] tensor of Scene.raycast_camera(cam, opts, 0), float32 [height, width, 16] — and `rgbaz` the float32
        [height, width, 5] frame.  The accumulated frame goes to `out` (same shape; may be `rgbaz` itself) and / or
        `rgba8` (uint8 [height, width, 4]); with neither given, a new `out` is made.  `history` (float32 [height, width])
        receives each pixel's history length.  All are contiguous torch tensors on the handle's device: anything else is
        a ValueError, never a copy through the host.  params: make_temporal_params(...), default the library's.
        `motion` (vmx_temporal_accumulate_motion_device): what motion_vectors made of `raw` after a geometry update,
        float32 [height, width, 8], read only — moved surfaces then keep their history; None is the call without.
        `variance` (vmx_temporal_accumulate_variance_device): float32 [height, width], receives the variance of each
        pixel's luminance, for Filter.apply(..., variance=...); required on a handle made with moments=True and refused
        on any other.  variance_params: make_variance_params(...), default the library's.
        `adaptive` (vmx_temporal_accumulate_adaptive_device): True, or make_adaptive_params(...) — the history is cut
        where the lighting changed (on either kind of handle, with or without `motion`); None or False is the call
        without.  `change`: float32 [height, width], receives each pixel's change ratio r (0 without support); it
        needs `adaptive`.
        Enqueued on `stream` (default torch.cuda.current_stream()), nothing synchronised; returns (out, rgba8)."""
        import torch
        dev = torch.device("cuda", self.device)
        moments = getattr(self, "moments", False)
        if moments and variance is None:
            raise ValueError("variance is required: the handle was made with moments=True")
        if not moments and (variance is not None or variance_params is not None):
            raise ValueError("variance needs a handle made with moments=True")
        if adaptive is False:
            adaptive = None
        if adaptive is not None and adaptive is not True and not isinstance(adaptive, L.AdaptiveParams):
            raise ValueError("adaptive must be None, True or make_adaptive_params(...)")
        if change is not None and adaptive is None:
            raise ValueError("change needs adaptive")
        _frame_tensor(raw, "raw", torch.float32, self.shape + (16,), dev)
        _frame_tensor(rgbaz, "rgbaz", torch.float32, self.shape + (5,), dev)
        if variance is not None:
            _frame_tensor(variance, "variance", torch.float32, self.shape, dev)
        if change is not None:
            _frame_tensor(change, "change", torch.float32, self.shape, dev)
        if motion is not None:
            _frame_tensor(motion, "motion", torch.float32, self.shape + (8,), dev)
        out, rgba8 = _out_pair(out, rgba8, self.shape, dev)
        if history is not None:
            _frame_tensor(history, "history", torch.float32, self.shape, dev)
        with _SideStream(dev, stream) as run:
            prm, s = None if params is None else C.byref(params), C.c_void_p(run.cuda_stream)
            if adaptive is not None:
                vprm = None if variance_params is None else C.byref(variance_params)
                aprm = None if adaptive is True else C.byref(adaptive)
                self._check(self._lib.vmx_temporal_accumulate_adaptive_device(self._h, C.byref(cam), _ptr(raw), _ptr(motion),
                                                                              _ptr(rgbaz), _ptr(out), _ptr(rgba8), _ptr(history),
                                                                              _ptr(variance), _ptr(change), prm, vprm, aprm, s))
            elif moments:
                vprm = None if variance_params is None else C.byref(variance_params)
                self._check(self._lib.vmx_temporal_accumulate_variance_device(self._h, C.byref(cam), _ptr(raw), _ptr(motion),
                                                                              _ptr(rgbaz), _ptr(out), _ptr(rgba8), _ptr(history),
                                                                              _ptr(variance), prm, vprm, s))
            elif motion is None:
                self._check(self._lib.vmx_temporal_accumulate_device(self._h, C.byref(cam), _ptr(raw), _ptr(rgbaz), _ptr(out),
                                                                     _ptr(rgba8), _ptr(history), prm, s))
            else:
                self._check(self._lib.vmx_temporal_accumulate_motion_device(self._h, C.byref(cam), _ptr(raw), _ptr(motion),
                                                                            _ptr(rgbaz), _ptr(out), _ptr(rgba8), _ptr(history),
                                                                            prm, s))
        return out, rgba8

    def reset(self, stream=None):
        """vmx_temporal_reset: forgets the history; the next `accumulate` is a first call"""
        self._check(self._lib.vmx_temporal_reset(self._h, None if stream is None else C.c_void_p(stream.cuda_stream)))

    def frames(self):
        """vmx_temporal_frames: calls of `accumulate` since the handle was made or reset"""
        n = C.c_uint64(0)
        self._check(self._lib.vmx_temporal_frames(self._h, C.byref(n)))
        return n.value
