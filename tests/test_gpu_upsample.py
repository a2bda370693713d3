"""G-buffer-guided upsampling on the device (vmx_upsample_*): every output is compared as uint32 bits with the float32
restatement (tests/upsample_spec.py), every pixel; NaN may appear only where the restatement has NaN.

Shapes (W, H, lw, lh): 1x1 from 1x1; 7x5 from 2x2 (ratio below 1/2, not an integer); 9x4 from 9x4 (ratio 1); 65x33 from
17x9 (about 1/4, three blocks across and five down, the last of each one pixel wide / high); 130x3 from 33x1 (a single
low row, five blocks across); 72x40 from 36x20 (1/2); 70x41 from 47x28 (about 2/3: a block's low footprint starts and ends
between low pixels).  A block is 32 x 8 full pixels, a wave two rows of 32."""
import ctypes as C
import functools

import numpy as np
import pytest

import filter_spec as FS
import oracle_lib as O
import upsample_spec as US
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1, 1), (7, 5, 2, 2), (9, 4, 9, 4), (65, 33, 17, 9), (130, 3, 33, 1), (72, 40, 36, 20), (70, 41, 47, 28)]
PARAMS = [None, dict(normal_squarings=0, sigma_depth=10.0), dict(normal_squarings=8, sigma_depth=1e-3)]
ODD = np.array([0x7FC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF], np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cached cases are read-only)


def _records(rng, h, w):
    """vmx_rayhit records [h, w, 16]: unit normals scattered around +z, depths in [5, 6), a band of columns that miss,
    and — where the image has the pixels for them — a zero normal, a NaN normal and a depth of 1e-40"""
    raw = np.zeros((h, w, 16), np.float32)
    nrm = np.float32([0, 0, 1]) + 0.4 * rng.normal(size=(h, w, 3))
    raw[..., 4:7] = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    raw[..., 3] = rng.uniform(5, 6, (h, w)).astype(np.float32)
    hit = np.ones((h, w), bool)
    hit[:, w // 3:w // 3 + max(1, w // 8)] = False
    raw[..., 3][~hit] = np.inf  # (a miss's record: distance INFINITY, a stale normal)
    raw.view(np.uint32)[..., 11] = np.where(hit, 3, 2)
    flat = raw.reshape(-1, 16)
    live = np.flatnonzero(hit.reshape(-1))
    if len(live) >= 4:
        a, b, c = live[len(live) // 5], live[len(live) // 2], live[(4 * len(live)) // 5]
        flat[a, 4:7] = 0.0
        flat[b, 4:7] = np.nan
        flat[c, 3] = np.float32(1e-40)
    return raw


@functools.lru_cache(maxsize=None)
def case(W, H, lw, lh):
    """(low frame [lh, lw, 5], low records, full records) from a seeded RandomState, computed once, never written to"""
    rng = np.random.RandomState(W * 1000003 + H * 1009 + lw * 31 + lh)
    lo = rng.uniform(0, 1, (lh, lw, 5)).astype(np.float32)
    flat = lo.reshape(-1, 5)
    n = flat.shape[0]
    for k, v in enumerate(ODD):  # NaN, +inf, -inf and denormal colours (a 1 x 1 image keeps the last of them)
        flat[(k * 7 + 1) % n, k % 3] = v
    flat[(3 * n) // 4, 3:] = ODD[:2]  # ... and an odd alpha and depth
    raw_lo, raw_hi = _records(rng, lh, lw), _records(rng, H, W)
    for a in (lo, raw_lo, raw_hi):
        a.setflags(write=False)
    return lo, raw_lo, raw_hi


@functools.lru_cache(maxsize=None)
def want_of(shape, kw):
    lo, raw_lo, raw_hi = case(*shape)
    out = US.upsample(lo, *FS.guide_of(raw_lo), *FS.guide_of(raw_hi), US.params_of(**dict(kw)))
    out.setflags(write=False)
    return out


def params_of(kw):
    return None if kw is None else va.make_upsample_params(**kw)


def key(kw):
    return tuple(sorted((kw or {}).items()))


def quantized_on_device(frame):
    """vmx_quantize_device of a [H, W, 5] device tensor -> uint8 [H, W, 4] (host)"""
    import torch
    h, w = frame.shape[:2]
    q = torch.empty((h, w, 4), dtype=torch.uint8, device=frame.device)
    torch.cuda.synchronize()
    L.check(L.lib().vmx_quantize_device(C.c_void_p(frame.data_ptr()), h * w, C.c_void_p(q.data_ptr()), None, 0, None))
    return q.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_from_%dx%d" % s)
def test_apply_is_the_restatement_bit_for_bit(shape):
    """the defaults (the kernel's constant form of normal_squarings) and two further parameter sets (its general form),
    with both outputs, with RGBAZ only and with rgba8 only; rgba8 is vmx_quantize_device of the RGBAZ output; the input
    is left alone"""
    import torch
    W, H, lw, lh = shape
    lo, raw_lo, raw_hi = case(*shape)
    src = dev(lo)
    with va.Upsample(lw, lh, W, H) as u:
        u.set_guides(dev(raw_lo), dev(raw_hi))
        for kw in PARAMS:
            want = want_of(shape, key(kw))
            prm = params_of(kw)
            out = torch.full((H, W, 5), -7.0, dtype=torch.float32, device="cuda")
            q = torch.full((H, W, 4), 99, dtype=torch.uint8, device="cuda")
            got = u.apply(src, out=out, rgba8=q, params=prm)
            assert got is out
            diff = (bits(out.cpu().numpy()) != bits(want)).any(axis=-1)
            assert FS.same_bits(out.cpu().numpy(), want), (shape, kw, int(diff.sum()), "pixels differ", np.argwhere(diff)[:4])
            assert np.array_equal(q.cpu().numpy(), quantized_on_device(out)), (shape, kw)
            only5 = u.apply(src, params=prm)
            assert np.array_equal(bits(only5.cpu().numpy()), bits(out.cpu().numpy())), (shape, kw)
            only4 = torch.full_like(q, 99)
            assert u.apply(src, rgba8=only4, params=prm) is None
            assert torch.equal(only4, q), (shape, kw)
            assert np.array_equal(bits(src.cpu().numpy()), bits(lo))  # the input is left alone
        if shape == (72, 40, 36, 20):
            outs = [want_of(shape, key(kw)) for kw in PARAMS]
            assert not FS.same_bits(outs[0], outs[1]) or not FS.same_bits(outs[0], outs[2])  # (the parameters matter)


def test_the_planted_oddities_reach_the_output():
    """the cases above are not all-finite by accident: NaN and infinite colours, the fallback and misses all occur"""
    shape = (72, 40, 36, 20)
    lo, raw_lo, raw_hi = case(*shape)
    out, fell, _ = US.upsample(lo, *FS.guide_of(raw_lo), *FS.guide_of(raw_hi), details=True)
    assert np.isnan(out[..., :3]).any() and np.isinf(out[..., :3]).any()
    n_hi, z_hi = FS.guide_of(raw_hi)
    assert 0 < fell.sum() < fell.size // 4 and (z_hi < 0).any() and np.isnan(n_hi).any()
    assert fell[(z_hi >= 0) & (z_hi < 1e-30)].all() and fell[np.isnan(n_hi).any(axis=-1)].all()


def test_refusals_leave_the_outputs_alone():
    import torch
    shape = (70, 41, 47, 28)
    W, H, lw, lh = shape
    lo, raw_lo, raw_hi = case(*shape)
    want = want_of(shape, key(None))
    src = dev(lo)

    def refused(call, match):
        with pytest.raises(va.VmxError, match=match) as e:
            call()
        assert e.value.code == L.VMX_ERR_INVALID

    with va.Upsample(lw, lh, W, H) as u:
        refused(lambda: u.apply(src), "no guides")
        u.set_guides(dev(raw_lo), dev(raw_hi))

        def still_works():
            assert FS.same_bits(u.apply(src).cpu().numpy(), want)

        still_works()
        for kw in (dict(normal_squarings=9), dict(sigma_depth=0.0), dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf"))):
            refused(lambda: u.apply(src, params=va.make_upsample_params(**kw)), "vmx_upsample_params")
        prm = va.make_upsample_params()
        prm.reserved[5] = 7
        refused(lambda: u.apply(src, params=prm), "reserved")
        still_works()
        # overlaps, with device pointers, refused before any launch: one buffer holds a low frame and, five floats into
        # it, a full frame; an rgba8 inside the input; an rgba8 inside the RGBAZ output
        nlo, nhi = lw * lh * 5, W * H * 5
        buf = torch.zeros(5 + nhi, dtype=torch.float32, device="cuda")
        a, b = buf[:nlo].view(lh, lw, 5), buf[5:].view(H, W, 5)
        a.copy_(src)
        before = buf.clone()
        refused(lambda: u.apply(a, out=b), "overlap")
        tail = buf[nlo - W * H:nlo].view(torch.uint8).view(H, W, 4)  # (the last W*H words of the input)
        refused(lambda: u.apply(a, rgba8=tail), "overlap")
        full = torch.zeros(nhi, dtype=torch.float32, device="cuda")
        refused(lambda: u.apply(src, out=full.view(H, W, 5), rgba8=full[8:8 + W * H].view(torch.uint8).view(H, W, 4)), "overlap")
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32)) and not full.any()  # nothing was written
        # buffers that only touch are fine: the full frame right after the low one
        buf2 = torch.zeros(nlo + nhi, dtype=torch.float32, device="cuda")
        a2, b2 = buf2[:nlo].view(lh, lw, 5), buf2[nlo:].view(H, W, 5)
        a2.copy_(src)
        assert FS.same_bits(u.apply(a2, out=b2).cpu().numpy(), want)
        # host pointers, straight through the C ABI (the Python layer would refuse them itself)
        host = np.array(lo)
        hout = np.zeros((H, W, 5), np.float32)
        out = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        lib = u._lib
        for args in ((C.c_void_p(host.ctypes.data), P(out), None), (P(src), C.c_void_p(hout.ctypes.data), None),
                     (P(src), None, C.c_void_p(hout.ctypes.data))):
            assert lib.vmx_upsample_apply_device(u._h, *args, None, None) == L.VMX_ERR_INVALID
            assert "not device memory" in lib.vmx_last_error().decode()
        hraw = np.array(raw_lo)
        d_hi = dev(raw_hi)
        assert lib.vmx_upsample_set_guides_device(u._h, C.c_void_p(hraw.ctypes.data + (-hraw.ctypes.data % 16)), P(d_hi),
                                                  None) == L.VMX_ERR_INVALID
        assert "not device memory" in lib.vmx_last_error().decode()
        assert lib.vmx_upsample_apply_device(u._h, P(src), None, None, None, None) == L.VMX_ERR_INVALID
        assert "no output" in lib.vmx_last_error().decode()
        still_works()
    for bad in ((lw, lh, lw - 1, H), (lw, lh, 4 * lw + 1, H), (0, lh, W, H)):
        with pytest.raises(va.VmxError) as e:
            va.Upsample(*bad)
        assert e.value.code == L.VMX_ERR_INVALID


def test_two_streams_with_new_guides_in_between():
    """apply on one stream, new guides and apply on another, and so on: the handle orders them by enqueue, so each call
    gives the result of the guides set before it"""
    import torch
    shape = (72, 40, 36, 20)
    W, H, lw, lh = shape
    lo, raw_lo, raw_hi = case(*shape)
    rng = np.random.RandomState(12)
    raw_lo2, raw_hi2 = _records(rng, lh, lw), _records(rng, H, W)
    want = [want_of(shape, key(None)), US.upsample(lo, *FS.guide_of(raw_lo2), *FS.guide_of(raw_hi2))]
    assert not FS.same_bits(want[0], want[1])
    src = dev(lo)
    guides = [(dev(raw_lo), dev(raw_hi)), (dev(raw_lo2), dev(raw_hi2))]
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    with va.Upsample(lw, lh, W, H) as u:
        for i in range(6):
            u.set_guides(*guides[i % 2], stream=s[i % 2])
            outs.append(u.apply(src, out=torch.empty((H, W, 5), dtype=torch.float32, device="cuda"), stream=s[(i + 1) % 2]))
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert FS.same_bits(o.cpu().numpy(), want[i % 2]), i


def test_whole_chain_on_the_device_is_the_oracle_chain():
    """cornell8, 72x40 from 36x20, seed 3, corrected sampling, early stop off: Scene.render_device at the low size with
    64 spp, both G-buffers from raycast_camera, va.Filter at the low size, va.Upsample — against the oracle's render and
    camera rays pushed through filter_spec and upsample_spec, bit for bit at every stage"""
    import torch
    pos, nrm, uv = scenes.cornell8()
    c = scenes.cornell_camera()
    W, H, lw, lh = 72, 40, 36, 20
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 16)
    lcam = va.low_camera(va.make_camera(c["position"], c["rotation_deg"], W, H, 64), lw, lh)
    opts = va.make_opts(seed=3, early_stop=False, sampling=va.VMX_SAMPLING_CORRECTED)
    osc = O.OracleScene(pos, nrm, uv)
    low, _ = osc.render(lcam, opts)
    rec_lo = osc.raycast(*O.primary_rays(lcam, opts, 0)).reshape(lh, lw)
    rec_hi = osc.raycast(*O.primary_rays(cam, opts, 0)).reshape(H, W)
    osc.close()
    n_lo, z_lo = FS.guide_of(rec_lo)
    n_hi, z_hi = FS.guide_of(rec_hi)
    low_f = FS.filtered_frame(low, n_lo, z_lo)
    want = US.upsample(low_f, n_lo, z_lo, n_hi, z_hi)
    with va.Scene(pos, nrm, uv) as sc, va.Filter(lw, lh) as f, va.Upsample(lw, lh, W, H) as u:
        d_low = torch.empty((lh, lw, 5), dtype=torch.float32, device="cuda")
        sc.render_device(lcam, opts, d_low.data_ptr())
        raw_lo = sc.raycast_camera(lcam, opts, 0)["raw"]
        raw_hi = sc.raycast_camera(cam, opts, 0)["raw"]
        f.set_guide(raw_lo)
        d_f, _ = f.apply(d_low)
        u.set_guides(raw_lo, raw_hi)
        q = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        got = u.apply(d_f, out=torch.empty((H, W, 5), dtype=torch.float32, device="cuda"), rgba8=q)
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_low.cpu().numpy()), bits(low)), "the low frame differs from the oracle's"
        for mine, theirs in ((raw_lo, (n_lo, z_lo)), (raw_hi, (n_hi, z_hi))):
            n, z = FS.guide_of(mine.cpu().numpy())
            assert FS.same_bits(n, theirs[0]) and FS.same_bits(z, theirs[1]), "a guide differs from the oracle's"
        assert FS.same_bits(d_f.cpu().numpy(), low_f), "the filtered low frame differs"
        assert FS.same_bits(got.cpu().numpy(), want), "the upsampled frame differs"
        assert np.array_equal(q.cpu().numpy().reshape(-1, 4), O.quantize(want)[0])  # (an all-finite frame in [0, 1])
    assert np.isfinite(want).all() and want[..., :3].min() >= 0 and want[..., :3].max() <= 1


def test_upsample_through_python():
    """out= and rgba8= tensors are reused and returned, a closed handle raises, the context manager closes"""
    import torch
    shape = (65, 33, 17, 9)
    W, H, lw, lh = shape
    lo, raw_lo, raw_hi = case(*shape)
    want = want_of(shape, key(None))
    src = dev(lo)
    out = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
    q = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    with va.Upsample(lw, lh, W, H) as u:
        assert u.shape == (H, W) and u.low_shape == (lh, lw)
        u.set_guides(dev(raw_lo), dev(raw_hi))
        for _ in range(2):
            out.fill_(-1.0), q.fill_(7)
            ptr5, ptr4 = out.data_ptr(), q.data_ptr()
            got = u.apply(src, out=out, rgba8=q)
            assert got is out and (out.data_ptr(), q.data_ptr()) == (ptr5, ptr4)
            assert FS.same_bits(out.cpu().numpy(), want)
        made = u.apply(src)
        assert made is not out and tuple(made.shape) == (H, W, 5) and FS.same_bits(made.cpu().numpy(), want)
        with pytest.raises(ValueError, match=r"\[33, 65, 5\]"):
            u.apply(src, out=torch.empty((lh, lw, 5), dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError, match="uint8"):
            u.apply(src, rgba8=torch.empty((H, W, 4), dtype=torch.float32, device="cuda"))
        handle = u
    assert handle._h is None  # the context manager closed it
    with pytest.raises(va.VmxError, match="NULL handle"):
        handle.apply(src)
    handle.close()  # closing twice is fine
    u2 = va.Upsample(lw, lh, W, H)
    u2.close()
    with pytest.raises(va.VmxError, match="NULL handle"):
        u2.set_guides(dev(raw_lo), dev(raw_hi))
