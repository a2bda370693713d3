"""Albedo-demodulated denoising (include/vermilion_hip.h, "albedo-demodulated denoising") restated in numpy float32: what
vmx_albedo_camera_device (vermilion_amd/csrc/vmx_albedo.inc) and the DEMOD instantiations of k_atrous
(vmx_filter.inc) are held to, bit for bit.  A helper, not a test.

Every array and every scalar is float32, so each written operation rounds once to float32, in the order written.
Where it pays: resolved textures on surfaces wider than the filter's footprint.  Thin bars with a minified texture (the
lattice) are the known limit — there demodulation is no better than the plain filter (tests/test_demod_abi.py)."""
import numpy as np

import filter_spec as FS
import oracle_lib as O

F = np.float32
ALBEDO_FLOOR = F(2.0 ** -10)  # VMX_ALBEDO_FLOOR
FLT_MAX = F(3.402823466e+38)


def albedo_plane(osc, tex, cam, opts, first, n):
    """[H, W, 4] float32: per pixel the mean over samples first .. first + n - 1 of what the integrator multiplies a camera
    path's throughput by at its first hit, and in .w the fraction of those rays with the material bit.  osc: the
    OracleScene; tex: the texture bound to the scene under test ([H, W(, C)] float) or None"""
    W, H = int(cam.image_res[0]), int(cam.image_res[1])
    total = np.zeros((W * H, 3), np.float32)
    cnt = np.zeros(W * H, np.uint32)
    for k in range(first, first + n):
        o, d = O.primary_rays(cam, opts, k)
        r = osc.raycast(o, d)
        mat = (r["flags"] & 2) != 0
        t = np.ones((W * H, 3), np.float32)
        if tex is not None and mat.any():
            t[mat] = O.texture_sample(tex, r["uv"][mat])[:, :3]
        total = total + t
        cnt = cnt + mat.astype(np.uint32)
    fn = F(n)
    out = np.empty((W * H, 4), np.float32)
    out[:, :3] = total / fn
    out[:, 3] = cnt.astype(np.float32) / fn
    assert total.dtype == np.float32
    return out.reshape(H, W, 4)


def clamped_albedo(albedo):
    """am of the demodulated filter: each channel of albedo[..., :3], or the floor unless above it and finite"""
    a = np.ascontiguousarray(albedo, np.float32)[..., :3]
    with np.errstate(all="ignore"):
        ok = (a > ALBEDO_FLOOR) & (a <= FLT_MAX)
    return np.where(ok, a, ALBEDO_FLOOR).astype(np.float32)


def demodulated_frame(frame, n, z, albedo, params=None):
    """the RGBAZ frame [H, W, 5] through the demodulated filter: divide, FS.filtered_frame, multiply"""
    am = clamped_albedo(albedo)
    f = np.array(frame, np.float32)
    with np.errstate(all="ignore"):
        f[..., :3] = f[..., :3] / am
        out = FS.filtered_frame(f, n, z, params)
        out[..., :3] = out[..., :3] * am
    assert out.dtype == np.float32
    return out
