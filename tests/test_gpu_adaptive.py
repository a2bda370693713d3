"""Adaptive temporal accumulation on the device (vmx_temporal_accumulate_adaptive_device): every output — the accumulated
frame, its rgba8 form, the history lengths, the change ratios, the variance — is compared with the float32 restatement
(tests/adaptive_spec.py) fed the same sequence of calls, as uint32 bits, every pixel; the next call's outputs pin the state.

The G-buffers are the device's own (vmx_raycast_camera_device on the Cornell set under a stepping camera, the block
refitted between frames and followed by motion records); the frames are synthetic, noise around a value that steps at
frame 2, so that some windows cut and some do not.  Sizes: 70x41 (ragged in both tile dimensions), 33x9 (one pixel past a
tile each way), 5x3 (smaller than the window), 1x1."""
import ctypes as C

import numpy as np
import pytest

import adaptive_spec as AS
import filter_spec as FS
import motion_spec as MS
import oracle_lib as O
import temporal_spec as TS
import variance_spec as VS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [(70, 41), (33, 9), (5, 3), (1, 1)]
IDS = ["%dx%d" % s for s in SIZES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def stepped_frames(w, h, seed, n=4):
    """n frames [h, w, 5]: per channel a level (0.5, 0.4, 0.3 before frame 2; 0.12, 0.3, 0.31 from it on: a clear step, a
    small one and none) plus uniform noise of +-0.08, alpha and depth random"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        level = np.array([0.5, 0.4, 0.3] if i < 2 else [0.12, 0.3, 0.31])
        f = rng.uniform(0, 1, (h, w, 5)).astype(np.float32)
        f[..., :3] = (level + rng.uniform(-0.08, 0.08, (h, w, 3))).astype(np.float32)
        f.setflags(write=False)
        out.append(f)
    return out


@pytest.fixture(scope="module")
def sequences():
    """{(w, h): [(cam, frame, records [h, w, 16], motion [h, w, 8] or None)] x 4}, computed once, never written to: the
    Cornell set, case D of tests/motion_spec.py (the block turned and shifted under a stepping camera), the geometry
    refitted on the device, the records from vmx_raycast_camera_device and vmx_motion_device"""
    pos0, nrm0, uv = scenes.cornell8()
    c = scenes.cornell_camera()
    shift, angle, cam_step = MS.CASES["D"]
    out = {}
    for w, h in SIZES:
        frames, seq, prev = stepped_frames(w, h, 100 + w), [], None
        with va.Scene(pos0, nrm0, uv) as sc:
            for i in range(4):
                pos, nrm = MS.moved_block(pos0, nrm0, shift, angle, i)
                d_pos, d_nrm = dev(pos), dev(nrm)
                if i:
                    sc.update(pos=d_pos, nrm=d_nrm)
                p, r = c["position"], c["rotation_deg"]
                cam = va.make_camera((p[0] + cam_step[0] * i, p[1], p[2]), (r[0], r[1] + cam_step[1] * i, r[2]), w, h, 16)
                opts = va.make_opts(seed=3 + i, early_stop=False, sampling=va.VMX_SAMPLING_CORRECTED)
                d_raw = sc.raycast_camera(cam, opts, 0)["raw"]
                mv = None
                if prev is not None:
                    mv = va.motion_vectors(d_raw, d_pos, prev[0], prev[1]).cpu().numpy()
                    mv.setflags(write=False)
                raw = d_raw.cpu().numpy().reshape(h, w, 16)
                raw.setflags(write=False)
                seq.append((cam, frames[i], raw, mv))
                prev = (d_pos, d_nrm)
        out[w, h] = seq
    return out


class Pair:
    """a handle and the restatement, fed the same calls: `step` makes one adaptive call on both and compares every output"""

    def __init__(self, w, h, moments):
        self.t = va.Temporal(w, h, moments=moments)
        self.w, self.h, self.moments = w, h, moments
        self.state = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.t.close()

    def spec(self, cam, frame, raw, mv, aparams, adaptive=True):
        """the restatement's call: (frame, n', change, variance or None)"""
        if adaptive:
            want, self.state, n, chg = AS.step(self.state, frame, raw, cam, mv, aparams=aparams, moments=self.moments)
        else:
            want, self.state, n = (VS.step if self.moments else MS.step)(self.state, frame, raw, cam, mv)
            chg = None
        return want, n, chg, VS.variance(self.state) if self.moments else None

    def step(self, cam, frame, raw, mv=None, aparams=None, tag=None, form="both", change=True, stream=None):
        import torch
        h, w = self.h, self.w
        want, want_n, want_chg, want_var = self.spec(cam, frame, raw, mv, aparams)
        # (one word more than the image on either side of the planes the new kernels write: nothing may land there)
        cbuf = torch.full((h * w + 2,), -7.0, dtype=torch.float32, device="cuda")
        vbuf = torch.full((h * w + 2,), -7.0, dtype=torch.float32, device="cuda")
        chg = cbuf[1:-1].view(h, w) if change else None
        var = vbuf[1:-1].view(h, w) if self.moments else None
        src, d_raw = dev(frame), dev(raw)
        d_mv = None if mv is None else dev(mv)
        hist = torch.empty((h, w), dtype=torch.float32, device="cuda")
        q = None if form == "rgbaz" else torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        dst = None if form == "rgba8" else src if form == "in place" else torch.empty((h, w, 5), device="cuda")
        ap = True if aparams is None else va.make_adaptive_params(**aparams)
        out, q = self.t.accumulate(cam, d_raw, src, out=dst, rgba8=q, history=hist, motion=d_mv, variance=var, adaptive=ap,
                                   change=chg, stream=stream)
        torch.cuda.synchronize()
        assert out is dst
        if out is not None:
            got = out.cpu().numpy()
            assert FS.same_bits(got, want), (tag, int((bits(got) != bits(want)).any(axis=-1).sum()), "pixels differ")
        if q is not None:
            ok = np.all(np.isfinite(want[..., :4]) & (want[..., :4] >= 0) & (want[..., :4] <= 1), axis=-1)
            assert np.array_equal(q.cpu().numpy()[ok], O.quantize(want)[0].reshape(h, w, 4)[ok]), (tag, "rgba8")
        assert FS.same_bits(hist.cpu().numpy(), want_n), (tag, "history lengths differ")
        if change:
            got_chg = chg.cpu().numpy()
            assert FS.same_bits(got_chg, want_chg), (tag, int((bits(got_chg) != bits(want_chg)).sum()), "change ratios differ")
        assert cbuf[0].item() == -7.0 and cbuf[-1].item() == -7.0, (tag, "written outside the change plane")
        if self.moments:
            got_var = var.cpu().numpy()
            assert FS.same_bits(got_var, want_var), (tag, int((bits(got_var) != bits(want_var)).sum()), "variances differ")
            assert vbuf[0].item() == -7.0 and vbuf[-1].item() == -7.0, (tag, "written outside the variance")
        if form != "in place":
            assert np.array_equal(bits(src.cpu().numpy()), bits(frame))  # the input is left alone
        return want, want_n, want_chg


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_sequences_are_the_restatement_bit_for_bit(sequences, size, moments):
    """four frames with the value step at frame 2, with the motion records and without them, then two further calls on
    the last frame's records (the carried state); the forms in turn: both outputs, in place, rgba8 only, the frame only,
    d_change NULL"""
    w, h = size
    seq = sequences[size]
    forms = ("both", "both", "in place", "rgba8", "rgbaz", "both")
    for with_mv in (True, False):
        with Pair(w, h, moments) as p:
            cut = 0
            for i, (cam, frame, raw, mv) in enumerate(seq + [seq[3][:3] + (None,)] * 2):
                _, n, chg = p.step(cam, frame, raw, mv if with_mv else None, tag=(size, moments, with_mv, i), form=forms[i],
                                   change=i != 4)
                cut += int(np.sum(chg > 1))
                if i == 0:
                    assert np.all(chg == 0) and np.all(n == 1)
            assert p.t.frames() == 6
            if w >= 33:
                assert cut > 0 and n.max() > 1  # (some history was cut, some was kept)
    # other parameters: normal_squarings read from the pass, another gamma, sigma_depth and min_support
    ap = dict(gamma=1.5, min_support=2.0, normal_squarings=3, sigma_depth=0.03)
    with Pair(w, h, moments) as p:
        for i, (cam, frame, raw, mv) in enumerate(seq):
            p.step(cam, frame, raw, mv, ap, tag=(size, moments, ap, i), form="in place" if i == 3 else "both")


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_nan_and_inf_colours_follow_the_restatement(sequences, moments):
    """NaN and +-inf colours in the input of frames 1 and 2 (and, from there, in the history): the outputs are the
    restatement's bits, NaN included; a window that holds a NaN has r = NaN or the finite channels' and the NaN pixel
    itself is never cut"""
    w, h = 70, 41
    seq = sequences[w, h]
    with Pair(w, h, moments) as p:
        for i, (cam, frame, raw, mv) in enumerate(seq):
            f = np.array(frame)
            if i in (1, 2):
                f[5, 9, 0], f[20, 40, 1], f[30, 60, 2], f[12, 33, :3] = np.nan, np.inf, -np.inf, np.nan
            _, n, chg = p.step(cam, f, raw, mv, tag=("nan", moments, i))
            if i == 1:
                assert np.isnan(chg).any() and not np.any(chg[12, 33] > 1)


def test_without_a_cut_the_call_is_the_existing_one_on_the_device(sequences):
    """gamma = 3e38 (gamma*gamma = +inf) against the motion call and the variance call on a second handle, bit for bit:
    frame, rgba8, history lengths, variance; d_change is 0 or NaN"""
    import torch
    w, h = 70, 41
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda")  # noqa: E731
    off = va.make_adaptive_params(gamma=3e38)
    for moments in (False, True):
        with va.Temporal(w, h, moments=moments) as a, va.Temporal(w, h, moments=moments) as b:
            for i, (cam, frame, raw, mv) in enumerate(sequences[w, h]):
                d_raw, d_mv = dev(raw), None if mv is None else dev(mv)
                outs, chg = [], new(h, w)
                for t, kw in ((a, dict(adaptive=off, change=chg)), (b, {})):
                    hist, var = new(h, w), new(h, w) if moments else None
                    o, q = t.accumulate(cam, d_raw, dev(frame), out=new(h, w, 5), rgba8=new(h, w, 4, dtype=torch.uint8),
                                        history=hist, motion=d_mv, variance=var, **kw)
                    outs.append((o, q, hist, var))
                torch.cuda.synchronize()
                for x, y in zip(*outs):
                    if x is not None:
                        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                           y.view(torch.int32) if y.dtype == torch.float32 else y), (moments, i)
                assert torch.all((chg == 0) | torch.isnan(chg)), (moments, i)


def test_existing_and_adaptive_calls_alternate_on_one_handle(sequences):
    """the state layout is one: the motion (variance) call and the adaptive call frame by frame on one handle give the
    restatements' bits, whichever comes first"""
    import torch
    w, h = 70, 41
    seq = sequences[w, h] + [sequences[w, h][3][:3] + (None,)] * 2
    for moments in (False, True):
        for first_adaptive in (False, True):
            with Pair(w, h, moments) as p:
                for i, (cam, frame, raw, mv) in enumerate(seq):
                    if (i % 2 == 0) == first_adaptive:
                        p.step(cam, frame, raw, mv, tag=("alternating", moments, first_adaptive, i))
                        continue
                    want, want_n, _, want_var = p.spec(cam, frame, raw, mv, None, adaptive=False)
                    hist = torch.empty((h, w), device="cuda")
                    var = torch.empty((h, w), device="cuda") if moments else None
                    out, _ = p.t.accumulate(cam, dev(raw), dev(frame), history=hist, motion=None if mv is None else dev(mv),
                                            variance=var)
                    assert FS.same_bits(out.cpu().numpy(), want) and FS.same_bits(hist.cpu().numpy(), want_n), (moments, i)
                    if moments:
                        assert FS.same_bits(var.cpu().numpy(), want_var), i


def test_calls_on_two_streams_are_ordered_by_enqueue(sequences):
    """six adaptive calls alternate on two streams: ordered by enqueue on the handle, each result its own call's"""
    import torch
    w, h = 70, 41
    six = (sequences[w, h] + sequences[w, h][::-1])[:6]
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    for moments in (False, True):
        state, wants = None, []
        for cam, frame, raw, _ in six:
            want, state, n, chg = AS.step(state, frame, raw, cam, moments=moments)
            wants.append((want, n, chg, VS.variance(state) if moments else None))
        ins = [(cam, dev(raw), dev(frame)) for cam, frame, raw, _ in six]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with va.Temporal(w, h, moments=moments) as t:
            torch.cuda.synchronize()
            outs = []
            for i, (cam, raw, frame) in enumerate(ins):
                hist, chg, var = new(h, w), new(h, w), new(h, w) if moments else None
                o, _ = t.accumulate(cam, raw, frame, out=new(h, w, 5), history=hist, variance=var, adaptive=True, change=chg,
                                    stream=s2 if i % 2 else s1)
                outs.append((o, hist, chg, var))
            torch.cuda.synchronize()
            for i, got in enumerate(outs):
                for g, wnt in zip(got, wants[i]):
                    if g is not None:
                        assert FS.same_bits(g.cpu().numpy(), wnt), (moments, i)
            assert t.frames() == 6


def test_the_plane_is_allocated_by_the_first_adaptive_call_and_freed_by_destroy():
    """2048 x 1024: the state is 2 x 48 (56) B per pixel, the plane 16 (24).  Device memory falls by the state at create,
    stays through an existing call, falls by the plane at the first adaptive call, stays at the second, and is back after
    destroy (other users of the device: 8 MiB of slack either way)"""
    import torch
    w, h = 2048, 1024
    npix, slack = w * h, 8 << 20
    cam = va.make_camera((0, 0, 0), (0, 0, 0), w, h, 16)
    raw = torch.zeros((h, w, 16), device="cuda")  # (every pixel a miss)
    frame, out, var = torch.rand((h, w, 5), device="cuda"), torch.empty((h, w, 5), device="cuda"), torch.empty((h, w), device="cuda")
    free = lambda: (torch.cuda.synchronize(), torch.cuda.mem_get_info()[0])[1]  # noqa: E731
    for moments in (False, True):  # (whatever the runtime allocates at a kernel's first launch is allocated here)
        small = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 16)
        with va.Temporal(8, 8, moments=moments) as t:
            for adaptive in (None, True, True):
                t.accumulate(small, raw.view(-1)[:8 * 8 * 16].view(8, 8, 16), frame.view(-1)[:8 * 8 * 5].view(8, 8, 5),
                             variance=var.view(-1)[:64].view(8, 8) if moments else None, adaptive=adaptive)
    for moments in (False, True):
        kw = dict(variance=var) if moments else {}
        state, plane = 2 * (56 if moments else 48) * npix, (24 if moments else 16) * npix
        before = free()
        t = va.Temporal(w, h, moments=moments)
        created = free()
        assert abs((before - created) - state) <= slack, (moments, before - created, state)
        t.accumulate(cam, raw, frame, out=out, **kw)
        assert abs(free() - created) <= slack
        t.accumulate(cam, raw, frame, out=out, adaptive=True, **kw)
        first = free()
        assert abs((created - first) - plane) <= slack, (moments, created - first, plane)
        t.accumulate(cam, raw, frame, out=out, adaptive=True, **kw)
        assert abs(free() - first) <= slack
        assert torch.equal(out.view(torch.int32), frame.view(torch.int32))  # (misses: the input)
        t.close()
        assert abs(free() - before) <= slack, (moments, free() - before)


def test_refusals_that_need_a_handle(sequences):
    """the kind of handle, and d_change's overlaps: before any launch, the handle's state untouched"""
    import torch
    lib = L.lib()
    w, h = 70, 41
    cam, frame, raw, _ = sequences[w, h][0]
    npix = w * h
    d_raw, d_in, d_out = dev(raw), dev(frame), torch.empty((h, w, 5), device="cuda")
    d_var, d_chg, d_hist = (torch.empty((h, w), device="cuda") for _ in range(3))
    d_q = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    err = lambda: lib.vmx_last_error().decode()  # noqa: E731
    acc = lib.vmx_temporal_accumulate_adaptive_device
    with va.Temporal(w, h) as plain, va.Temporal(w, h, moments=True) as mom:
        cb = C.byref(cam)
        assert acc(mom._h, cb, P(d_raw), None, P(d_in), P(d_out), None, None, None, None, None, None, None, None) == L.VMX_ERR_INVALID
        assert "NULL d_variance" in err()
        assert acc(plain._h, cb, P(d_raw), None, P(d_in), P(d_out), None, None, P(d_var), None, None, None, None, None) \
            == L.VMX_ERR_INVALID and "keeps no moments" in err()
        vp = va.make_variance_params()
        assert acc(plain._h, cb, P(d_raw), None, P(d_in), P(d_out), None, None, None, None, None, C.byref(vp), None, None) \
            == L.VMX_ERR_INVALID and "keeps no moments" in err()
        # the existing calls stay refused on a moments handle, and the variance call on a plain one
        assert lib.vmx_temporal_accumulate_device(mom._h, cb, P(d_raw), P(d_in), P(d_out), None, None, None, None) == L.VMX_ERR_INVALID
        assert "moments stale" in err()
        assert lib.vmx_temporal_accumulate_variance_device(plain._h, cb, P(d_raw), None, P(d_in), P(d_out), None, None, P(d_var),
                                                           None, None, None) == L.VMX_ERR_INVALID and "VMX_TEMPORAL_MOMENTS" in err()
        # d_change may meet no other buffer of the call: each of them in turn
        big = torch.empty((npix * 16 + npix,), device="cuda")
        for name, args in (
                ("d_rayhit", dict(raw=P(big), chg=P(big, npix * 64 - 4))),
                ("d_in_rgbaz", dict(src=P(big), chg=P(big, npix * 20 - 4))),
                ("d_out_rgbaz", dict(out=P(big), chg=P(big))),
                ("d_rgba8", dict(q=P(big), chg=P(big, npix * 4 - 4))),
                ("d_history_len", dict(hist=P(big, 4), chg=P(big))),
                ("d_variance", dict(var=P(big), chg=P(big, npix * 4 - 4))),
                ("d_motion", dict(mv=P(big), chg=P(big, npix * 32 - 4)))):
            a = dict(raw=P(d_raw), mv=None, src=P(d_in), out=P(d_out), q=P(d_q), hist=P(d_hist), var=P(d_var), chg=P(d_chg))
            a.update(args)
            assert acc(mom._h, cb, a["raw"], a["mv"], a["src"], a["out"], a["q"], a["hist"], a["var"], a["chg"], None, None, None,
                       None) == L.VMX_ERR_INVALID, name
            assert "d_change overlaps" in err(), (name, err())
        host = np.zeros(npix, np.float32)
        assert acc(mom._h, cb, P(d_raw), None, P(d_in), P(d_out), None, None, P(d_var), C.c_void_p(host.ctypes.data), None, None,
                   None, None) == L.VMX_ERR_INVALID and "d_change" in err()
        assert mom.frames() == 0 and plain.frames() == 0  # (every refused call left the handles as they were)
        # a buffer that ends where the change plane begins does not overlap it
        assert acc(mom._h, cb, P(d_raw), None, P(d_in), P(d_out), None, None, P(big), P(big, npix * 4), None, None, None, None) == L.VMX_OK
        assert acc(plain._h, cb, P(d_raw), None, P(d_in), P(d_out), None, None, None, None, None, None, None, None) == L.VMX_OK
        torch.cuda.synchronize()
        assert mom.frames() == 1 and plain.frames() == 1
