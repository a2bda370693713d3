"""Variance-guided denoising on the device (vmx_temporal_accumulate_variance_device, vmx_filter_apply_variance_device):
every output — the accumulated frame, the history lengths, the variance, the filtered frame, the rgba8 form — is compared
with the float32 restatement (tests/variance_spec.py) fed the same sequence of calls, as uint32 bits, every pixel; NaN may
appear only where the restatement has NaN.

Shapes, the smallest at which the kernels can go wrong: 70x41 and 33x9 (partial blocks in both directions, a second block
row of one line), 1x1, and 12x9 (step 16 exceeds the image at iteration 5, and the 7x7 window exceeds it in y)."""
import ctypes as C

import numpy as np
import pytest

import demod_spec as DS
import filter_spec as FS
import motion_spec as MS
import oracle_lib as O
import temporal_spec as TS
import test_temporal_abi as TT
import variance_spec as VS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
W, H = 70, 41
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def words(rec):
    """[H, W, 16] float32 words of records"""
    return MS.words_of(rec).view(np.float32)


@pytest.fixture(scope="module")
def cornell():
    """four 16-spp oracle frames of the Cornell set at 70x41, computed once, never written to: [(cam, frame, records
    [H, W, 16], motion [H, W, 8] or None)].  Frames 0 and 1: one camera, one geometry (a first call, a static second
    call); frames 2 and 3: the block moved (case D of tests/motion_spec.py: turned and shifted under a stepping camera),
    with motion records"""
    pos0, nrm0, uv = scenes.cornell8()
    c = scenes.cornell_camera()
    shift, angle, cam_step = MS.CASES["D"]
    out, prev = [], None
    for i, k in enumerate((0, 0, 1, 2)):
        pos, nrm = MS.moved_block(pos0, nrm0, shift, angle, k)
        p, r = c["position"], c["rotation_deg"]
        cam = va.make_camera((p[0] + cam_step[0] * k, p[1], p[2]), (r[0], r[1] + cam_step[1] * k, r[2]), W, H, 16)
        opts = va.make_opts(seed=3 + i, early_stop=False, sampling=va.VMX_SAMPLING_CORRECTED)
        osc = O.OracleScene(pos, nrm, uv)
        img, _ = osc.render(cam, opts)
        o, d = O.primary_rays(cam, opts, 0)
        raw = np.array(words(osc.raycast(o, d).reshape(H, W)))
        osc.close()
        mv = None
        if k:
            mv = MS.motion(raw, pos, prev[0], prev[1])
            assert (bits(mv)[..., 3] & 1).any()
            mv.setflags(write=False)
        img = np.array(img)
        img.setflags(write=False), raw.setflags(write=False)
        out.append((cam, img, raw, mv))
        prev = (pos, nrm)
    return out


def planes(w, h, pos_x, seed):
    """w x h records in the manner of test_temporal_abi._two_planes (the plane z = -4, one world unit per pixel, the left
    half with normal +z and the right half with normal +x) for any size, with a few pixels spoilt where there is room: a
    miss, a zero normal, a NaN normal; and a random frame"""
    cam = va.make_camera((pos_x, 0, 0), (0, 0, 0), w, h, 16, back_distance=1.0, back_size=(w / 4.0, h / 4.0))
    rec = np.zeros((h, w, 16), np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rec[..., 0] = pos_x + (xs + 0.5 - w / 2)
    rec[..., 1] = -(ys + 0.5 - h / 2)
    rec[..., 2] = -4.0
    rec[..., 3] = np.sqrt((rec[..., 0] - pos_x) ** 2 + rec[..., 1] ** 2 + 16.0)
    rec[:, :(w + 1) // 2, 6] = 1.0
    rec[:, (w + 1) // 2:, 4] = 1.0
    rec.view(np.uint32)[..., 11] = 3
    if w >= 8 and h >= 8:
        rec.view(np.uint32)[2, 3, 11] = 2
        rec[2, 3, 3] = np.inf
        rec[4, 2, 4:7] = 0.0
        rec[5, w - 2, 5] = np.nan
    frame = np.random.RandomState(seed).uniform(0, 1, (h, w, 5)).astype(np.float32)
    return cam, frame, rec


class Pair:
    """a moments handle and the restatement, fed the same calls: `step` makes one on both and compares every output"""

    def __init__(self, w, h):
        self.t = va.Temporal(w, h, moments=True)
        self.w, self.h = w, h
        self.state = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.t.close()

    def reset(self):
        self.t.reset()
        self.state = None

    def step(self, cam, frame, raw, mv=None, vparams=None, tag=None, in_place=False, variance_only=False):
        import torch
        want, self.state, want_n = VS.step(self.state, frame, raw, cam, mv)
        want_var = VS.variance(self.state, vparams)
        # (one word more than the image on either side: nothing may be written there)
        vbuf = torch.full((self.h * self.w + 2,), -7.0, dtype=torch.float32, device="cuda")
        var = vbuf[1:-1].view(self.h, self.w)
        src, d_raw = dev(frame), dev(raw)
        d_mv = None if mv is None else dev(mv)
        vprm = None if vparams is None else va.make_variance_params(**vparams)
        if variance_only:  # through the C ABI itself: the variance counts as an output
            lib = L.lib()
            L.check(lib.vmx_temporal_accumulate_variance_device(
                self.t._h, C.byref(cam), C.c_void_p(d_raw.data_ptr()), None if d_mv is None else C.c_void_p(d_mv.data_ptr()),
                C.c_void_p(src.data_ptr()), None, None, None, C.c_void_p(var.data_ptr()), None,
                None if vprm is None else C.byref(vprm), None))
            torch.cuda.synchronize()
        else:
            hist = torch.empty((self.h, self.w), dtype=torch.float32, device="cuda")
            q = torch.empty((self.h, self.w, 4), dtype=torch.uint8, device="cuda")
            dst = src if in_place else torch.empty((self.h, self.w, 5), device="cuda")
            out, q = self.t.accumulate(cam, d_raw, src, rgba8=q, out=dst, history=hist, motion=d_mv, variance=var,
                                       variance_params=vprm)
            assert out is dst
            got = out.cpu().numpy()
            assert FS.same_bits(got, want), (tag, int((bits(got) != bits(want)).any(axis=-1).sum()), "pixels differ")
            assert FS.same_bits(hist.cpu().numpy(), want_n), (tag, "history lengths differ")
            ok = np.all(np.isfinite(want[..., :4]) & (want[..., :4] >= 0) & (want[..., :4] <= 1), axis=-1)
            assert np.array_equal(q.cpu().numpy()[ok], O.quantize(want)[0].reshape(self.h, self.w, 4)[ok]), (tag, "rgba8")
        got_var = var.cpu().numpy()
        assert FS.same_bits(got_var, want_var), (tag, int((bits(got_var) != bits(want_var)).sum()), "variances differ")
        assert vbuf[0].item() == -7.0 and vbuf[-1].item() == -7.0, (tag, "written outside the variance")
        if not in_place:
            assert np.array_equal(bits(src.cpu().numpy()), bits(frame))  # the input is left alone
        return want, want_n, want_var


@pytest.mark.parametrize("min_history", [1.0, 4.0, 64.0])
def test_cornell_sequence_is_the_restatement_bit_for_bit(cornell, min_history):
    """a first call, a static second call, two calls with motion records on the moved block, then two further calls (the
    carried state: colour, history and moments of everything before), with min_history 1, 4 and 64 — no pixel, some pixels
    and all pixels take the window"""
    vp = dict(min_history=min_history)
    with Pair(W, H) as p:
        taken = []
        for i, (cam, img, raw, mv) in enumerate(cornell + [cornell[3][:3] + (None,)] * 2):
            _, n, _ = p.step(cam, img, raw, mv, vp, tag=("cornell", min_history, i), in_place=i == 3)
            taken.append(float(np.mean(n < min_history)))
        assert p.t.frames() == 6
    if min_history == 1.0:
        assert max(taken) == 0
    elif min_history == 64.0:
        assert min(taken) == 1
    else:
        assert taken[0] == 1 and 0 < taken[3] < 1, taken
    # without motion records on the same frames the moved block restarts: another state, the same agreement
    with Pair(W, H) as p:
        for i, (cam, img, raw, _) in enumerate(cornell):
            p.step(cam, img, raw, None, vp, tag=("cornell, no records", min_history, i))


@pytest.mark.parametrize("shape", [(33, 9), (1, 1), (12, 9), (70, 41)], ids=lambda s: "%dx%d" % s)
def test_two_planes_pan_is_the_restatement_bit_for_bit(shape):
    """two planes under a camera that pans by one pixel and then by a quarter, spoilt records among them (a miss, a zero
    normal, a NaN normal): the first call, a static second call, the pans, and a call that asks for the variance alone;
    12 x 9 is test_temporal_abi._two_planes itself.  min_history 1, 4, 64 and normal_squarings 5 and 3."""
    w, h = shape
    path = (-1.0, -1.0, 0.0, 0.25, 0.25)
    for vp in (None, dict(min_history=1.0), dict(min_history=64.0, normal_squarings=3), dict(min_history=2.0, sigma_depth=0.01,
                                                                                           normal_squarings=0)):
        with Pair(w, h) as p:
            for i, x in enumerate(path):
                cam, frame, rec = planes(w, h, x, 40 + i)
                if shape == (12, 9):
                    cam, rec = TT._two_planes(x)
                _, n, var = p.step(cam, frame, rec, None, vp, tag=(shape, vp, i), variance_only=i == 4)
            if vp is None and w >= 8:
                assert n.max() >= 3 and np.any(n < 4) and np.any(var > 0)
            # reset: the next call is a first call again, on a moments handle too
            p.reset()
            assert p.t.frames() == 0
            cam, frame, rec = planes(w, h, 0.0, 50)
            _, n, var = p.step(cam, frame, rec, None, vp, tag=(shape, vp, "after reset"))
            assert np.all(n == 1)


def poisoned_variance(h, w, seed):
    """a variance plane of plausible size with 0, +inf, NaN, denormals and a negative value in a few pixels"""
    v = (np.random.RandomState(seed).uniform(0, 0.02, (h, w)) ** 2).astype(np.float32)
    flat = v.reshape(-1)
    odd = np.array([0.0, np.inf, np.nan, 1e-42, 1.4e-45, -0.01, 3e38], np.float32)
    idx = np.linspace(0, flat.size - 1, len(odd)).astype(int) if flat.size >= len(odd) else np.arange(flat.size)
    flat[idx] = odd[:len(idx)]
    return v


def filter_inputs(cornell, shape, seed=9):
    """(frame, records, variance, albedo) for a shape: the Cornell oracle frame with the variance of its own accumulation at
    70x41, two planes and a random frame elsewhere; a few pixels of the variance and of the guide spoilt"""
    w, h = shape
    if shape == (W, H):
        state = None
        for cam, img, raw, mv in cornell[:2]:
            _, state, _ = VS.step(state, img, raw, cam)
        frame, rec, var = np.array(img), np.array(raw), np.array(VS.variance(state))
        flat = var.reshape(-1)
        flat[[5, 700, 1500, 2000, 2869]] = np.array([np.inf, np.nan, 0.0, 1e-42, -1.0], np.float32)
        rec[7, 9, 4:7] = 0.0
        rec[30, 60, 4] = np.nan
    else:
        _, frame, rec = planes(w, h, 0.0, seed)
        var = poisoned_variance(h, w, seed)
    rng = np.random.RandomState(seed + 1)
    albedo = rng.uniform(0.05, 1.0, (h, w, 4)).astype(np.float32)
    albedo.reshape(-1, 4)[0, :3] = (0.0, np.nan, -1.0)  # (these take the floor)
    return frame, rec, var, albedo


CASES = [  # (shape, iterations, normal_squarings, albedo)
    ((W, H), 1, 5, False), ((W, H), 2, 5, True), ((W, H), 5, 5, False), ((W, H), 5, 5, True), ((W, H), 10, 3, False),
    ((W, H), 5, 3, True), ((W, H), 1, 3, True),
    ((33, 9), 5, 5, False), ((33, 9), 2, 3, True), ((1, 1), 1, 5, False), ((1, 1), 5, 5, True), ((12, 9), 5, 5, False),
    ((12, 9), 10, 5, True), ((12, 9), 1, 3, False),
]


@pytest.mark.parametrize("shape,iterations,squarings,with_albedo", CASES,
                         ids=["%dx%d-it%d-m%d-%s" % (c[0] + (c[1], c[2], "albedo" if c[3] else "plain")) for c in CASES])
def test_filter_is_the_restatement_bit_for_bit(cornell, shape, iterations, squarings, with_albedo):
    """out of place, in place and rgba8 only; the variance plane holds 0, +inf, NaN, denormals and a negative value in a
    few pixels, the guide a zero and a NaN normal; sigma_luminance 4 (the default) and 0.5"""
    import torch
    w, h = shape
    frame, rec, var, albedo = filter_inputs(cornell, shape)
    n, z = FS.guide_of(rec)
    prm = FS.params_of(iterations=iterations, normal_squarings=squarings)
    lp = va.make_filter_params(iterations=iterations, normal_squarings=squarings)
    d_alb = dev(albedo) if with_albedo else None
    with va.Filter(w, h) as f:
        f.set_guide(dev(rec))
        for sl in (4.0, 0.5):
            want = VS.filtered_frame(frame, var, n, z, prm, sl, albedo if with_albedo else None)
            d_var, src = dev(var), dev(frame)
            q = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
            out, q = f.apply(src, rgba8=q, out=torch.empty_like(src), params=lp, albedo=d_alb, variance=d_var,
                             sigma_luminance=sl)
            got = out.cpu().numpy()
            assert FS.same_bits(got, want), (sl, int((bits(got) != bits(want)).any(axis=-1).sum()), "pixels differ")
            ok = np.all(np.isfinite(want[..., :4]) & (want[..., :4] >= 0) & (want[..., :4] <= 1), axis=-1)
            assert np.array_equal(q.cpu().numpy()[ok], O.quantize(want)[0].reshape(h, w, 4)[ok])
            assert np.array_equal(bits(src.cpu().numpy()), bits(frame))
            assert FS.same_bits(d_var.cpu().numpy(), var)  # read only
            # in place, and rgba8 alone
            same, _ = f.apply(src, out=src, params=lp, albedo=d_alb, variance=d_var, sigma_luminance=sl)
            assert same is src and FS.same_bits(src.cpu().numpy(), want), (sl, "in place")
            q2 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            none, q2 = f.apply(dev(frame), rgba8=q2, params=lp, albedo=d_alb, variance=d_var, sigma_luminance=sl)
            assert none is None and torch.equal(q2, q)
        # the default sigma_luminance is 4
        out, _ = f.apply(dev(frame), params=lp, albedo=d_alb, variance=dev(var))
        assert FS.same_bits(out.cpu().numpy(), VS.filtered_frame(frame, var, n, z, prm, 4.0, albedo if with_albedo else None))


@pytest.mark.parametrize("iterations", [1, 5])
def test_infinite_variance_is_the_plain_call_on_the_device(cornell, iterations):
    """test_variance_abi's condition (b) between two device calls: d_variance = +inf everywhere against
    vmx_filter_apply_device with sigma_colour = 1e19, bit for bit"""
    import torch
    cam, img, raw, _ = cornell[0]
    with va.Filter(W, H) as f:
        f.set_guide(dev(raw))
        inf = torch.full((H, W), float("inf"), dtype=torch.float32, device="cuda")
        got, _ = f.apply(dev(img), params=va.make_filter_params(iterations=iterations), variance=inf)
        want, _ = f.apply(dev(img), params=va.make_filter_params(iterations=iterations, sigma_colour=1e19))
        assert not torch.isnan(got).any() and torch.equal(got.view(torch.int32), want.view(torch.int32))
        plain, _ = f.apply(dev(img), params=va.make_filter_params(iterations=iterations))
        assert not torch.equal(got, plain)


def test_refusals_that_need_a_handle(cornell):
    """the kind of handle, and d_variance's overlaps: before any launch, the handle's state untouched"""
    import torch
    lib = L.lib()
    cam, img, raw, _ = cornell[0]
    npix = W * H
    d_raw, d_in, d_out = dev(raw), dev(img), torch.empty((H, W, 5), device="cuda")
    d_var, d_hist, d_q = torch.empty((H, W), device="cuda"), torch.empty((H, W), device="cuda"), \
        torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    d_mv = torch.zeros((H, W, 8), device="cuda")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    err = lambda: lib.vmx_last_error().decode()  # noqa: E731
    with va.Temporal(W, H) as plain, va.Temporal(W, H, moments=True) as mom:
        accv, acc, accm = (lib.vmx_temporal_accumulate_variance_device, lib.vmx_temporal_accumulate_device,
                           lib.vmx_temporal_accumulate_motion_device)
        assert accv(plain._h, C.byref(cam), P(d_raw), None, P(d_in), P(d_out), None, None, P(d_var), None, None, None) \
            == L.VMX_ERR_INVALID and "VMX_TEMPORAL_MOMENTS" in err()
        assert acc(mom._h, C.byref(cam), P(d_raw), P(d_in), P(d_out), None, None, None, None) == L.VMX_ERR_INVALID
        assert "moments stale" in err()
        assert accm(mom._h, C.byref(cam), P(d_raw), P(d_mv), P(d_in), P(d_out), None, None, None, None) == L.VMX_ERR_INVALID
        assert "moments stale" in err()
        with pytest.raises(ValueError, match="moments=True"):
            plain.accumulate(cam, d_raw, d_in, variance=d_var)
        with pytest.raises(ValueError, match="variance is required"):
            mom.accumulate(cam, d_raw, d_in)
        # d_variance may meet no other buffer of the call: each of them in turn, from either side
        big = torch.empty((npix * 16 + npix,), device="cuda")
        for name, args in (
                ("d_rayhit", dict(raw=P(big), var=P(big, npix * 64 - 4))),
                ("d_in_rgbaz", dict(src=P(big), var=P(big, npix * 20 - 4))),
                ("d_in_rgbaz", dict(src=P(big, npix * 4 - 4), var=P(big))),
                ("d_out_rgbaz", dict(out=P(big), var=P(big))),
                ("d_rgba8", dict(q=P(big), var=P(big, npix * 4 - 4))),
                ("d_history_len", dict(hist=P(big, 4), var=P(big))),
                ("d_motion", dict(mv=P(big), var=P(big, npix * 32 - 4)))):
            a = dict(raw=P(d_raw), mv=None, src=P(d_in), out=P(d_out), q=P(d_q), hist=P(d_hist), var=P(d_var))
            a.update(args)
            assert accv(mom._h, C.byref(cam), a["raw"], a["mv"], a["src"], a["out"], a["q"], a["hist"], a["var"], None, None,
                        None) == L.VMX_ERR_INVALID, name
            assert "d_variance overlaps" in err(), (name, err())
        # a buffer that ends where the variance begins does not overlap it
        assert accv(mom._h, C.byref(cam), P(d_raw), None, P(big), None, None, None, P(big, npix * 20), None, None, None) == L.VMX_OK
        assert mom.frames() == 1 and plain.frames() == 0  # (every refused call left the handles as they were)
        # host memory is no device memory
        host = np.zeros(npix, np.float32)
        assert accv(mom._h, C.byref(cam), P(d_raw), None, P(d_in), P(d_out), None, None, C.c_void_p(host.ctypes.data), None,
                    None, None) == L.VMX_ERR_INVALID and "d_variance" in err()
        mom.reset()
        assert mom.frames() == 0
    with va.Filter(W, H) as f:
        app = lib.vmx_filter_apply_variance_device
        # before any guide was set, as the plain call
        assert app(f._h, P(d_in), P(d_var), None, P(d_out), None, None, 4.0, None) == L.VMX_ERR_INVALID and "no guide" in err()
        f.set_guide(d_raw)
        big = torch.empty((npix * 6,), device="cuda")
        assert app(f._h, P(d_in), P(big, npix * 20 - 4), None, P(big), None, None, 4.0, None) == L.VMX_ERR_INVALID
        assert "d_variance overlaps" in err()
        assert app(f._h, P(d_in), P(big), None, None, P(big, npix * 4 - 4), None, 4.0, None) == L.VMX_ERR_INVALID
        assert "d_variance overlaps" in err()
        assert app(f._h, P(d_in), C.c_void_p(host.ctypes.data), None, P(d_out), None, None, 4.0, None) == L.VMX_ERR_INVALID
        assert "d_variance" in err()
        # the variance may share memory with the input frame (both are read only) and end where an output begins
        d_var.fill_(0.01)
        assert app(f._h, P(d_in), P(d_var), None, P(d_out), None, None, 4.0, None) == L.VMX_OK
        big[:npix] = 0.01
        assert app(f._h, P(d_in), P(big), None, P(big, npix * 4), None, None, 4.0, None) == L.VMX_OK
        torch.cuda.synchronize()
        assert torch.equal(big[npix:npix * 6].view(H, W, 5).view(torch.int32), d_out.view(torch.int32))


def test_plain_calls_are_unchanged_after_variance_calls(cornell):
    """a plain handle and the plain and the demodulated filter calls give temporal_spec's and filter_spec's bits, in a
    process in which the variance calls have run (and run between them)"""
    import torch
    frame, rec, var, albedo = filter_inputs(cornell, (W, H))
    n, z = FS.guide_of(rec)
    with va.Temporal(W, H) as plain, Pair(W, H) as p, va.Filter(W, H) as f:
        state = None
        for i, (cam, img, raw, mv) in enumerate(cornell):
            p.step(cam, img, raw, mv, tag=("moments", i))
            want, state, want_n = TS.step(state, img, raw, cam) if mv is None else MS.step(state, img, raw, cam, mv)
            hist = torch.empty((H, W), device="cuda")
            out, _ = plain.accumulate(cam, dev(raw), dev(img), history=hist, motion=None if mv is None else dev(mv))
            assert FS.same_bits(out.cpu().numpy(), want) and FS.same_bits(hist.cpu().numpy(), want_n), i
        f.set_guide(dev(rec))
        guided, _ = f.apply(dev(frame), variance=dev(var))
        out, _ = f.apply(dev(frame))
        assert FS.same_bits(out.cpu().numpy(), FS.filtered_frame(frame, n, z))
        guided2, _ = f.apply(dev(frame), variance=dev(var), albedo=dev(albedo))
        out, _ = f.apply(dev(frame), albedo=dev(albedo))
        assert FS.same_bits(out.cpu().numpy(), DS.demodulated_frame(frame, n, z, albedo))
        assert not torch.equal(guided, guided2)
