"""Adaptive sampling on the device (vmx_progressive_begin_ex / state / step_selected / error / select / step_adaptive): a
handle whose pixels took different numbers of samples still ends at the oracle's frame, bit for bit; its previews are each
pixel's own prefix; the second moment, the error, the variance and the selection map are tests/sampling_spec.py's, bit
for bit; and what adaptive sampling buys in image error at equal samples is measured and pinned.

Shapes: those of test_gpu_progressive.py — the 8-triangle Cornell set at 70x41 (2,870 pixels: the last wave of every
pixel list is partial) at 16 and 64 spp, and the lattice at 64x48x16 for bounce generations that are not empty."""
import math
import os
import subprocess

import numpy as np
import pytest

import demod_spec as DS
import filter_spec as FS
import oracle_lib as O
import sampling_spec as SS
import variance_spec as VS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 70, 41
ELIDE = va.VMX_SAMPLING_ELIDE_DEAD
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cornell_cam(spp, w=W, h=H):
    c = scenes.cornell_camera()
    return va.make_camera(c["position"], c["rotation_deg"], w, h, spp)


def lattice_cam(spp, w=64, h=48):
    c = scenes.lattice_camera()
    return va.make_camera(c["position"], c["rotation_deg"], w, h, spp)


@pytest.fixture(scope="module")
def sc():
    with va.Scene(*scenes.cornell8()) as s:
        yield s


@pytest.fixture(scope="module")
def oracle():
    """oracle frames of the Cornell set, computed once per (camera, options) and never written to"""
    osc = O.OracleScene(*scenes.cornell8())
    cache = {}

    def render(spp, **kw):
        key = (spp, tuple(sorted(kw.items())))
        if key not in cache:
            img, st = osc.render(cornell_cam(spp), va.make_opts(**kw))
            img.setflags(write=False)
            cache[key] = (img, st)
        return cache[key]

    yield render
    osc.close()


def state(p):
    """(sums [rows, W, 4] float32, counts [rows, W] int32) of the handle, read back"""
    import torch
    sums = torch.empty(p.shape + (4,), dtype=torch.float32, device="cuda")
    counts = torch.empty(p.shape, dtype=torch.int32, device="cuda")
    p.state_device(sums, counts)
    p.preview()  # (the host entry synchronises the handle's stream)
    return sums.cpu().numpy(), counts.cpu().numpy()


# ---- selection maps and the host replay of a selected step ----------------------------------------------------------------
def make_map(name, n, kmax, rng):
    """a selection map [rows, W] uint8 by name; n: the counts so far.  Non-zero bytes of any value select."""
    rows, w = n.shape
    m = np.zeros((rows, w), np.uint8)
    active = np.flatnonzero(n.reshape(-1) < kmax)
    if name == "all":
        m[:] = 255
    elif name == "checker":
        yy, xx = np.mgrid[0:rows, 0:w]
        m[:] = ((xx + yy) & 1) * 3
    elif name == "one":
        m[rows // 2, w // 3] = 1
    elif name in ("n63", "n64", "n65"):
        m.reshape(-1)[rng.permutation(active)[:int(name[1:])]] = 1
    elif name == "random30":
        m[:] = rng.uniform(size=(rows, w)) < 0.3
    elif name == "finished":
        assert (n >= kmax).any(), "the map of finished pixels needs some"
        m[:] = n >= kmax
    else:
        assert name == "none", name
    return m


def replay(n, kmax, m, samples):
    """the counts after a selected step, the number of pixels that took samples, the samples taken"""
    take = np.where((n < kmax) & (m != 0), np.minimum(samples if samples else kmax, kmax - n), 0)
    return n + take, int((take > 0).sum()), int(take.sum())


SEQUENCES = {
    "A": [("checker", 3), ("n63", 5), ("none", 3)],
    "B": [("one", 0), ("finished", 5), ("n64", 3), ("all", 5)],
    "C": [("random30", 3), ("n65", 5), ("random30", 3)],
}


def ragged_then_complete(scene, cam, opts, ref, want, rays, tag, moments=False, sequences="ABC"):
    """selected steps by each sequence's maps, every one checked against the host replay, then step(0): the frame is `ref`,
    the summed samples are want["samples"] and (rays) the summed ray counters want's"""
    kmax = 4 * (cam.rays_per_pixel // 4)
    for name in sequences:
        rng = np.random.RandomState(ord(name))
        tot = dict(rays_primary=0, rays_secondary=0, samples=0, passes=0)
        with scene.progressive(cam, opts, moments=moments) as p:
            n = np.zeros(p.shape, np.int64)
            steps = 0
            for mname, samples in SEQUENCES[name]:
                m = make_map(mname, n, kmax, rng)
                st, nsel = p.step_selected(samples, dev(m))
                n, want_sel, want_samples = replay(n, kmax, m, samples)
                assert (nsel, st["samples"]) == (want_sel, want_samples), (tag, name, mname)
                steps += want_sel > 0
                info = p.info()
                assert info["pixels_active"] == int((n < kmax).sum()) and info["steps"] == steps, (tag, name, mname)
                assert np.array_equal(state(p)[1], n), (tag, name, mname)
                for k in tot:
                    tot[k] += st[k]
            st = p.step(0)
            for k in tot:
                tot[k] += st[k]
            info = p.info()
            img = p.preview()
            assert info["pixels_active"] == 0 and info["steps"] == steps + 1
            assert np.array_equal(bits(img), bits(ref)), (tag, name, int((bits(img) != bits(ref)).any(axis=2).sum()))
            assert tot["samples"] == want["samples"] == info["samples"] and tot["passes"] == info["passes"], (tag, name)
            if rays:
                assert tot["rays_primary"] == want["rays_primary"] and tot["rays_secondary"] == want["rays_secondary"], (tag, name)
            st, nsel = p.step_selected(3, dev(np.ones(p.shape, np.uint8)))
            assert nsel == 0 and st["samples"] == 0 and p.info() == info  # a selected step of a complete frame does nothing


# ---- a. ragged, then complete, is the oracle's frame ------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", [va.VMX_SAMPLING_PARITY, va.VMX_SAMPLING_CORRECTED, ELIDE], ids=["parity", "corrected", "elide"])
@pytest.mark.parametrize("spp", [16, 64])
def test_ragged_then_complete_is_the_oracles_frame(sc, oracle, spp, sampling):
    """Every map (none, all, a checkerboard, one pixel, exactly 63 / 64 / 65 pixels, a seeded 30 %, only finished pixels)
    in steps of 3, 5 and 0 samples, in the default routing and with every pass fused (1) or split (4), on plain and on
    moments handles.  Ray counters: the oracle's when every ray is traced; under VMX_SAMPLING_ELIDE_DEAD the counters hold
    the traced rays only, which the oracle does not model (test_gpu_progressive.py), so there only the samples are held."""
    cam = cornell_cam(spp)
    ref, ost = oracle(spp, seed=11, early_stop=False, sampling=sampling)
    for pipeline in (0, 1, 4):
        opts = va.make_opts(seed=11, early_stop=False, sampling=sampling, pipeline=pipeline)
        ragged_then_complete(sc, cam, opts, ref, ost, not (sampling & ELIDE), (spp, pipeline), moments=pipeline == 1)


def test_ragged_lattice_with_live_bounce_generations():
    pos, nrm, uv = scenes.lattice()
    cam = lattice_cam(16)
    osc = O.OracleScene(pos, nrm, uv)
    ref, ost = osc.render(cam, va.make_opts(seed=5, early_stop=False))
    osc.close()
    assert ost["rays_secondary"] > 0
    with va.Scene(pos, nrm, uv) as s:
        for pipeline in (0, 4):
            ragged_then_complete(s, cam, va.make_opts(seed=5, early_stop=False, pipeline=pipeline), ref, ost, True, ("lattice", pipeline),
                                 moments=pipeline == 4)


def test_ragged_stripes_of_one_rank(sc, oracle):
    """maps are indexed by local pixel: rank 1 of 3, stripes of 4 rows"""
    sub = dict(world=3, rank=1, stripe_rows=4)
    ref, ost = oracle(16, seed=4, early_stop=False, **sub)
    assert ref.shape == (va.local_rows(H, 4, 1, 3), W, 5)
    ragged_then_complete(sc, cornell_cam(16), va.make_opts(seed=4, early_stop=False, **sub), ref, ost, True, "stripes")


# ---- b, c. previews of a ragged handle; a plain step on it ------------------------------------------------------------------
@pytest.fixture(scope="module")
def prefix(sc):
    """a plain, never ragged handle (16 spp, seed 9) stepped one sample at a time: its preview (rgbaz, rgba8) and its raw
    state after every n = 0..16 — the frames of today's code that a ragged handle's pixels are held to"""
    cam, opts = cornell_cam(16), va.make_opts(seed=9, early_stop=False)
    prev, quant, sums = [], [], []
    with sc.progressive(cam, opts) as p:
        for n in range(17):
            if n:
                p.step(1)
            f, q = p.preview(rgba8=True)
            s, c = state(p)
            assert (c == n).all() and (s[..., 3] == 0).all()  # a plain handle's w reads 0
            prev.append(f), quant.append(q), sums.append(s)
    out = dict(cam=cam, opts=opts, prev=np.stack(prev), quant=np.stack(quant), sums=np.stack(sums))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def at_counts(rec, n):
    """rec [17, rows, W, ...] taken at each pixel's own count n [rows, W]"""
    yy, xx = np.mgrid[0:n.shape[0], 0:n.shape[1]]
    return rec[n, yy, xx]


def test_ragged_preview_is_each_pixels_own_prefix(sc, prefix):
    import torch
    kmax = 16
    rng = np.random.RandomState(2)
    with sc.progressive(prefix["cam"], prefix["opts"]) as p:
        n = np.zeros(p.shape, np.int64)
        before = p.preview()
        step = 0
        for mname, samples in SEQUENCES["A"] + SEQUENCES["B"] + SEQUENCES["C"]:
            m = make_map(mname, n, kmax, rng)
            _, nsel = p.step_selected(samples, dev(m))
            n2, want_sel, _ = replay(n, kmax, m, samples)
            cur, q = p.preview(rgba8=True)
            assert nsel == want_sel and p.info()["pixels_active"] == int((n2 < kmax).sum()), mname
            assert np.array_equal(cur[..., 4], n2.astype(F)), mname
            assert np.array_equal(bits(cur), bits(at_counts(prefix["prev"], n2))), mname
            assert np.array_equal(q, at_counts(prefix["quant"], n2)), mname
            same = n2 == n
            assert np.array_equal(bits(cur[same]), bits(before[same])), mname  # unselected pixels: bit for bit unchanged
            if step in (1, 5):
                d5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
                d4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
                p.preview_device(d5, d4)
                p.preview()
                assert np.array_equal(bits(d5.cpu().numpy()), bits(cur)) and np.array_equal(d4.cpu().numpy(), q)
            n, before, step = n2, cur, step + 1
        assert len(np.unique(n)) > 3  # the handle really is ragged


def test_plain_step_on_a_ragged_handle(sc, prefix):
    kmax = 16
    rng = np.random.RandomState(3)
    with sc.progressive(prefix["cam"], prefix["opts"]) as p:
        n = np.zeros(p.shape, np.int64)
        for mname, samples in SEQUENCES["C"] + [("one", 0)]:
            m = make_map(mname, n, kmax, rng)
            p.step_selected(samples, dev(m))
            n, _, _ = replay(n, kmax, m, samples)
        for samples in (3, 5):
            st = p.step(samples)
            got = state(p)[1]
            rise = got - n
            active = n < kmax
            assert rise[active].min() >= 1 and rise[active].max() <= samples and (rise[~active] == 0).all()
            assert np.array_equal(got, np.minimum(n + samples, kmax))  # ... in fact all it may
            assert st["samples"] == int(rise.sum()) and p.info()["pixels_active"] == int((got < kmax).sum())
            assert np.array_equal(bits(p.preview()), bits(at_counts(prefix["prev"], got)))
            n = got
        p.step(0)
        assert p.info()["pixels_active"] == 0
        assert np.array_equal(bits(p.preview()), bits(prefix["prev"][16]))


# ---- d. moments ---------------------------------------------------------------------------------------------------------------
def test_moments_handle_is_a_plain_handle_plus_m2(sc):
    cam = cornell_cam(16)
    w_by_form = []
    for pipeline in (0, 1, 4):
        opts = va.make_opts(seed=9, early_stop=False, pipeline=pipeline)
        with sc.progressive(cam, opts) as a, sc.progressive(cam, opts, moments=True) as b:
            for samples in (3, 5, 0):
                sa, sb = a.step(samples), b.step(samples)
                assert sa["samples"] == sb["samples"]
                (su_a, n_a), (su_b, n_b) = state(a), state(b)
                assert np.array_equal(bits(su_a[..., :3]), bits(su_b[..., :3])) and np.array_equal(n_a, n_b), (pipeline, samples)
                assert (bits(su_a[..., 3]) == 0).all() and (su_b[..., 3] >= 0).all() and su_b[..., 3].max() > 0
                pa, qa = a.preview(rgba8=True)
                pb, qb = b.preview(rgba8=True)
                assert np.array_equal(bits(pa), bits(pb)) and np.array_equal(qa, qb), (pipeline, samples)
            assert a.info() == b.info() and a.info()["pixels_active"] == 0
            w_by_form.append(su_b[..., 3])
    assert all(np.array_equal(bits(w), bits(w_by_form[0])) for w in w_by_form)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F)).astype(np.float64)


def test_m2_is_the_sum_of_squared_sample_luminances(sc, prefix):
    """The samples themselves are not readable, the partial sums of a handle stepped one sample at a time are (`prefix`).
    Exact class: a pixel with at most one nonzero difference among its first 16 has that sample exactly (its sums jump
    from 0), and m2 must be fl(l*l) of it, bit for bit.  With seed 9 on an MI355X that is 2,869 of the 2,870 pixels (nearly
    every path of this frame ends black under the reference's sampling); the assertion below requires at least 1 in 20.
    Other pixels: sample k is rebuilt in float64 as S_k - S_(k-1) per channel.  S_k = fl(S_(k-1) + x_k), so the rebuilt
    value is off by at most half an ulp of the larger partial sum, h_c; the luminance of the true sample, computed on the
    device with 5 roundings of values no larger than it, differs from the float64 luminance L_k of the rebuilt one by at
    most d_k = lum(h) + 2.5 ulp(L_k + lum(h)); its square by (2 L_k + d_k) d_k, plus half an ulp of the square for
    rounding it, plus half an ulp of m2's partial sum (which never exceeds the final m2, every term being >= 0) for the
    add.  The bound is the sum of these over the 16 samples — derived, not a constant."""
    with sc.progressive(prefix["cam"], prefix["opts"], moments=True) as p:
        p.step(0)
        sums, counts = state(p)
    assert (counts == 16).all() and np.array_equal(bits(sums[..., :3]), bits(prefix["sums"][16][..., :3]))
    m2 = sums[..., 3]
    S = prefix["sums"].astype(np.float64)[..., :3]      # [17, rows, W, 3]
    x = S[1:] - S[:-1]                                   # rebuilt samples
    nonzero = (x != 0).any(axis=-1).sum(axis=0)          # per pixel
    exact = nonzero <= 1
    share = float(exact.mean())
    print(f"exact class: {int(exact.sum())} of {exact.size} pixels ({share:.1%})")
    assert share >= 0.05, share
    only = x.sum(axis=0).astype(F)                       # the one nonzero sample (or 0), exactly
    l = SS.luminance(only[..., 0], only[..., 1], only[..., 2])
    want = (l * l).astype(F)
    assert np.array_equal(bits(m2[exact]), bits(want[exact])), int((bits(m2[exact]) != bits(want[exact])).sum())
    h = 0.5 * np.maximum(ulp32(S[1:]), ulp32(S[:-1]))
    wts = np.float64([F(0.2126), F(0.7152), F(0.0722)])
    Lk = (x * wts).sum(axis=-1)
    lum_h = (h * wts).sum(axis=-1)
    d = lum_h + 2.5 * ulp32(np.abs(Lk) + lum_h)
    bound = ((2 * np.abs(Lk) + d) * d + 0.5 * ulp32((np.abs(Lk) + d) ** 2)).sum(axis=0) + 16 * 0.5 * ulp32(m2)
    err = np.abs(m2.astype(np.float64) - (Lk * Lk).sum(axis=0))
    print(f"m2 against the float64 sum of squares: worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), (float(err.max()), int((err > bound).sum()))


# ---- e. error, variance and selection against the restatement -----------------------------------------------------------------
def check_against_spec(p, kmax, tag):
    import torch
    sums, counts = state(p)
    d_e = torch.empty(p.shape, dtype=torch.float32, device="cuda")
    d_v = torch.empty(p.shape, dtype=torch.float32, device="cuda")
    e = None
    for floor in (0.05, 0.01):
        prm = va.make_sampling_params(floor=floor)
        p.error_device(d_e, d_v, prm)
        p.preview()
        e, var = d_e.cpu().numpy(), d_v.cpu().numpy()
        we, wv = SS.error_variance(sums, counts, floor)
        assert np.array_equal(bits(e), bits(we)) and np.array_equal(bits(var), bits(wv)), (tag, floor)
        only_e, only_v = torch.empty_like(d_e), torch.empty_like(d_v)
        p.error_device(error=only_e, params=prm), p.error_device(variance=only_v, params=prm)
        p.preview()
        assert torch.equal(only_e, d_e) and torch.equal(only_v, d_v)
    # thresholds that straddle the observed errors (floor 0.01), one of them an observed e itself
    seen = np.sort(e[(counts >= 2) & (e > 0)])
    thresholds = [0.0, 3.0e38]
    if seen.size:
        thresholds += [float(seen[len(seen) // 4]), float(seen[len(seen) // 2]), float(np.nextafter(seen[len(seen) // 2], F(0))),
                       float(seen[-1])]
    d_m = torch.empty(p.shape, dtype=torch.uint8, device="cuda")
    d_c = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    popcounts = set()
    for radius in (0, 1, 3):
        for thr in thresholds:
            for min_samples in (2, 12):
                prm = va.make_sampling_params(threshold=thr, floor=0.01, min_samples=min_samples, radius=radius)
                p.select_device(d_m, d_c, prm)
                p.preview()
                got = d_m.cpu().numpy()
                want = SS.select(sums, counts, kmax, thr, 0.01, min_samples, radius)
                assert np.array_equal(got, want), (tag, radius, thr, min_samples, int((got != want).sum()))
                assert int(d_c.item()) == int(want.sum()), (tag, radius, thr, min_samples)
                popcounts.add(int(want.sum()))
    assert not seen.size or len(popcounts) >= 3, popcounts  # none, all and something in between
    sums2, counts2 = state(p)
    assert np.array_equal(bits(sums2), bits(sums)) and np.array_equal(counts2, counts)  # nothing here changes the state
    return e


@pytest.mark.parametrize("sampling", [va.VMX_SAMPLING_PARITY, va.VMX_SAMPLING_CORRECTED], ids=["parity", "corrected"])
def test_error_variance_and_select_are_the_restatement(sc, sampling):
    """The state before any sample, after 8 uniform samples, ragged, and with finished pixels.  Under the reference's
    sampling nearly every path of this frame is black — after 8 samples four pixels have a non-zero error — so the cases
    run under VMX_SAMPLING_CORRECTED too, where nearly every path goes on and the errors are spread out."""
    kmax = 64
    cam, opts = cornell_cam(64), va.make_opts(seed=9, early_stop=False, sampling=sampling)
    with sc.progressive(cam, opts, moments=True) as p:
        check_against_spec(p, kmax, "no sample")  # n < 2 everywhere: no estimate
        p.step(1)
        p.step(7)
        e = check_against_spec(p, kmax, "uniform 8")
        assert p.step_adaptive(1, va.make_sampling_params(threshold=3.0e38, min_samples=9))[1] == W * H  # fewer than min_samples: all
        prm = va.make_sampling_params(threshold=float(np.sort(e.reshape(-1))[int(0.7 * e.size)]), floor=0.01)
        for _ in range(2):
            assert 0 < p.step_adaptive(4, prm)[1] < W * H  # the pixels of the larger errors and their neighbours
        assert len(np.unique(state(p)[1])) >= 2
        check_against_spec(p, kmax, "ragged")
        yy, xx = np.mgrid[0:H, 0:W]
        p.step_selected(0, dev((((xx // 3) + (yy // 2)) % 3 == 0).astype(np.uint8)))
        assert (state(p)[1] == kmax).any() and p.info()["pixels_active"] > 0
        check_against_spec(p, kmax, "with finished pixels")


def test_select_on_one_rank_of_a_striped_frame(sc):
    """the window is taken in the rank's packed rows: the restatement on the local image"""
    opts = va.make_opts(seed=4, early_stop=False, world=3, rank=1, stripe_rows=4)
    with sc.progressive(cornell_cam(64), opts, moments=True) as p:
        assert p.shape == (va.local_rows(H, 4, 1, 3), W)
        p.step(8)
        p.step_adaptive(4, va.make_sampling_params(threshold=0.1, floor=0.01))
        check_against_spec(p, 64, "stripes")


# ---- f. step_adaptive is select + step_selected -----------------------------------------------------------------------------
def test_step_adaptive_is_select_then_step_selected(sc):
    import torch
    cam, opts = cornell_cam(64), va.make_opts(seed=9, early_stop=False)
    with sc.progressive(cam, opts, moments=True) as a, sc.progressive(cam, opts, moments=True) as b:
        a.step(8), b.step(8)
        e, _ = SS.error_variance(*state(a), floor=0.05)
        prm = va.make_sampling_params(threshold=float(np.sort(e.reshape(-1))[int(0.8 * e.size)]))
        d_m = torch.empty(b.shape, dtype=torch.uint8, device="cuda")
        for rnd in range(3):
            sa, na = a.step_adaptive(4, prm)
            b.select_device(d_m, params=prm)
            sb, nb = b.step_selected(4, d_m)
            assert na == nb and 0 < na < W * H and sa["samples"] == sb["samples"], rnd
            (su_a, n_a), (su_b, n_b) = state(a), state(b)
            assert np.array_equal(bits(su_a), bits(su_b)) and np.array_equal(n_a, n_b), rnd
        assert a.info() == b.info() and np.array_equal(bits(a.preview()), bits(b.preview()))
        # the library's default parameters: the same through both routes
        sa, na = a.step_adaptive(4)
        b.select_device(d_m)
        sb, nb = b.step_selected(4, d_m)
        assert na == nb and np.array_equal(bits(state(a)[0]), bits(state(b)[0]))


# ---- g. previews downstream -------------------------------------------------------------------------------------------------
def test_filtered_previews_of_a_ragged_moments_handle(sc):
    import torch
    cam, opts = cornell_cam(64), va.make_opts(seed=9, early_stop=False)
    raw = sc.raycast_camera(cam, opts, 0)["raw"]
    n, z = FS.guide_of(raw.cpu().numpy())
    with sc.progressive(cam, opts, moments=True) as p, va.Filter(W, H) as f:
        f.set_guide(raw)
        p.step(8)
        for _ in range(2):
            p.step_adaptive(4, va.make_sampling_params(threshold=0.1, floor=0.01))
        sums, counts = state(p)
        assert len(np.unique(counts)) >= 2
        plain = p.preview()
        assert np.array_equal(plain[..., 4], counts.astype(F))
        assert FS.same_bits(p.preview_filtered(), FS.filtered_frame(plain, n, z))
        plane = sc.albedo_camera(cam, opts, samples=4).cpu().numpy()
        assert FS.same_bits(p.preview_filtered(albedo_samples=4), DS.demodulated_frame(plain, n, z, plane))
        d_var = torch.empty(p.shape, dtype=torch.float32, device="cuda")
        p.error_device(variance=d_var)
        p.preview()
        var = d_var.cpu().numpy()
        assert np.array_equal(bits(var), bits(SS.error_variance(sums, counts)[1]))
        out, _ = f.apply(dev(plain), variance=d_var)
        assert FS.same_bits(out.cpu().numpy(), VS.filtered_frame(plain, var, n, z))
        assert np.array_equal(bits(p.preview()), bits(plain))  # nothing changed


# ---- h. refusals that need a device -------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    pos, nrm, uv = scenes.cornell8()
    cam = cornell_cam(16)
    ones = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    f32 = torch.empty((H, W), dtype=torch.float32, device="cuda")

    def refused(call, match):
        with pytest.raises(va.VmxError, match=match) as e:
            call()
        assert e.value.code == L.VMX_ERR_INVALID

    with va.Scene(pos, nrm, uv) as s:
        # an early-stop handle: no selection entry, with or without moments; state and error still work
        for moments in (False, True):
            with s.progressive(cam, va.make_opts(seed=2, early_stop=True), moments=moments) as p:
                p.step(3)
                before = state(p)
                refused(lambda: p.step_selected(3, ones), "early_stop == 0")
                refused(lambda: p.step_adaptive(3), "early_stop == 0")
                refused(lambda: p.select_device(ones), "early_stop == 0")
                if moments:
                    p.error_device(f32)
                assert np.array_equal(bits(state(p)[0]), bits(before[0]))
                p.step(0)
                assert np.array_equal(bits(p.preview()), bits(s.render(cam, va.make_opts(seed=2, early_stop=True))[0]))
        # a handle without moments: selected steps work, what needs the second moment is refused
        opts = va.make_opts(seed=2, early_stop=False)
        with s.progressive(cam, opts) as p:
            refused(lambda: p.error_device(f32), "VMX_PROGRESSIVE_MOMENTS")
            refused(lambda: p.select_device(ones), "VMX_PROGRESSIVE_MOMENTS")
            refused(lambda: p.step_adaptive(3), "VMX_PROGRESSIVE_MOMENTS")
            assert p.step_selected(3, ones)[1] == W * H
        with s.progressive(cam, opts, moments=True) as p:
            # host pointers where device pointers are due
            host = np.ones((H, W, 4), np.float32)
            lib, hp = s._lib, C_ptr(host)
            for call in (lambda: lib.vmx_progressive_state_device(p._h, hp, None), lambda: lib.vmx_progressive_state_device(p._h, None, hp),
                         lambda: lib.vmx_progressive_step_selected_device(p._h, 3, hp, None, None),
                         lambda: lib.vmx_progressive_error_device(p._h, None, hp, None),
                         lambda: lib.vmx_progressive_error_device(p._h, None, None, hp),
                         lambda: lib.vmx_progressive_select_device(p._h, None, hp, None),
                         lambda: lib.vmx_progressive_select_device(p._h, None, C_ptr_of(ones), hp)):
                assert call() == L.VMX_ERR_INVALID and "device" in lib.vmx_last_error().decode(), lib.vmx_last_error()
            # buffers that overlap at the image's size, though not in their first element
            big = torch.empty((H * W * 5,), dtype=torch.float32, device="cuda")
            assert lib.vmx_progressive_state_device(p._h, big.data_ptr(), big.data_ptr() + 64) == L.VMX_ERR_INVALID
            assert "overlap" in lib.vmx_last_error().decode()
            assert lib.vmx_progressive_error_device(p._h, None, big.data_ptr(), big.data_ptr() + 64) == L.VMX_ERR_INVALID
            assert "overlap" in lib.vmx_last_error().decode()
            assert p.info()["steps"] == 0
            # the Python layer checks its tensors before the library sees them
            with pytest.raises(ValueError):
                p.step_selected(3, torch.ones((H, W), dtype=torch.float32, device="cuda"))
            with pytest.raises(ValueError):
                p.select_device(torch.ones((W, H), dtype=torch.uint8, device="cuda"))
            with pytest.raises(ValueError):
                p.error_device()
            # a scene updated since begin
            p.step(2)
            s.update(pos=pos)
            for call in (lambda: p.step_selected(3, ones), lambda: p.step_adaptive(3)):
                refused(call, "scene updated since vmx_progressive_begin")
            p.error_device(f32), p.select_device(ones), state(p)  # reading the state still works
            assert p.info()["steps"] == 1
    # a handle whose earlier step failed: a pass of 2^41 path slots cannot be allocated (an out-of-memory refusal of the
    # allocator, before anything is launched)
    with va.Scene(pos, nrm, uv) as s:
        huge = va.make_camera(list(cam.position), (0, 0, 0), 128, 128, 1 << 27)
        with s.progressive(huge, va.make_opts(seed=1, early_stop=False, samples_per_batch=1 << 27), moments=True) as p:
            few = torch.ones((128, 128), dtype=torch.uint8, device="cuda")
            with pytest.raises(va.VmxError, match="hipMalloc failed") as e:
                p.step_selected(1, few)
            assert e.value.code == L.VMX_ERR_NOMEM
            for call in (lambda: p.step_selected(1, few), lambda: p.step_adaptive(1), lambda: p.step(1)):
                refused(call, "an earlier step of this handle failed")
            assert p.info()["steps"] == 0
        img, _ = s.render(cam, va.make_opts(seed=2))  # the scene still serves
        assert img.shape == (H, W, 5)


def C_ptr(a):
    import ctypes
    return ctypes.c_void_p(a.ctypes.data)


def C_ptr_of(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


# ---- i. a C++ host through the C ABI ------------------------------------------------------------------------------------------
def test_cpp_host_samples_adaptively_through_the_c_abi(sc, tmp_path):
    """examples/render_progressive.cpp --adaptive: 8 uniform samples, adaptive steps of 4 with the library's defaults until
    the mean count reaches 16; its final preview is what the same calls give from Python"""
    exe = os.path.join(ROOT, "examples", "render_progressive")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    ppm, raw = tmp_path / "a.ppm", tmp_path / "a.f32"
    r = subprocess.run([exe, "--adaptive", str(ppm), "70", "41", "16", "5", "4", str(raw)], capture_output=True, text=True, check=True)
    c = scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 70, 41, 64, back_size=(3.6, F(3.6) * F(41) / F(70)))
    with sc.progressive(cam, va.make_opts(seed=5, early_stop=False), moments=True) as p:
        p.step(8)
        rounds = 0
        while p.info()["samples"] < 16 * W * H and p.info()["pixels_active"]:
            if p.step_adaptive(4)[1] == 0:
                break
            rounds += 1
        want, q = p.preview(rgba8=True)
        info = p.info()
    got = np.fromfile(raw, np.float32).reshape(41, 70, 5)
    assert np.array_equal(bits(got), bits(want))
    head = b"P6\n70 41\n255\n"
    data = ppm.read_bytes()
    assert data[:len(head)] == head and data[len(head):] == q.reshape(-1, 4)[:, :3].tobytes()
    lines = [l for l in r.stdout.splitlines() if "step " in l]
    assert len(lines) == rounds + 1 and rounds >= 1
    assert f"samples {info['samples']}," in r.stdout.splitlines()[-1]


# ---- j. quality, measured and recorded ----------------------------------------------------------------------------------------
QUALITY_SCENES = {
    "cornell": (scenes.cornell8, cornell_cam),
    "lattice": (scenes.lattice, lattice_cam),
}
# adaptive / uniform squared error of the displayed rgb against a converged frame, at the library's default parameters, as
# measured on an MI355X (profiles/sampling_quality.txt; the frames are deterministic).  None: not measured yet.
MEASURED_RATIO = {"cornell": 0.181753, "lattice": 0.188685}


def measure_quality(scene, cam_of, params=None, budget=16, kmax=64, seed=9):
    """adaptive (8 uniform samples, then step_adaptive(4) until budget * npix samples are in) against uniform (a plain
    handle stepped to ceil(total / npix) samples: never fewer) at the same seed; the converged frame is a one-call render of
    4096 spp with another seed.  Returns the two squared errors of the displayed rgb, their ratio, the counts."""
    cam = cam_of(kmax)
    opts = va.make_opts(seed=seed, early_stop=False)
    conv, _ = scene.render(cam_of(4096), va.make_opts(seed=seed + 1000, early_stop=False))
    with scene.progressive(cam, opts, moments=True) as p:
        npix = p.shape[0] * p.shape[1]
        p.step(8)
        rounds = 0
        while p.info()["samples"] < budget * npix and p.info()["pixels_active"]:
            if p.step_adaptive(4, params)[1] == 0:
                break
            rounds += 1
        total = p.info()["samples"]
        adaptive = p.preview()
        counts = state(p)[1]
    with scene.progressive(cam, opts) as p:
        p.step(int(math.ceil(total / npix)))
        uniform = p.preview()
        uniform_total = p.info()["samples"]
    err = lambda img: float(((img[..., :3].astype(np.float64) - conv[..., :3]) ** 2).sum())  # noqa: E731
    ea, eu = err(adaptive), err(uniform)
    return dict(adaptive=ea, uniform=eu, ratio=ea / eu, samples=total, uniform_samples=uniform_total, rounds=rounds,
                histogram=np.bincount(counts.reshape(-1), minlength=kmax + 1))


@pytest.mark.parametrize("name", sorted(QUALITY_SCENES))
def test_adaptive_sampling_quality_at_equal_samples(name):
    """Gate: where the measured ratio is below 1 it must stay below the midpoint between the measured value and 1; where it
    is not (adaptive sampling does not help that scene at these settings, README), the measured ratio is pinned within
    5 %.  The frames are deterministic: the margins only guard against later changes."""
    geometry, cam_of = QUALITY_SCENES[name]
    with va.Scene(*geometry()) as s:
        q = measure_quality(s, cam_of)
    print(f"{name}: adaptive {q['adaptive']:.6g} uniform {q['uniform']:.6g} ratio {q['ratio']:.4f} samples {q['samples']} "
          f"(uniform {q['uniform_samples']}) rounds {q['rounds']} histogram {q['histogram'].tolist()}")
    assert q["uniform_samples"] >= q["samples"]
    measured = MEASURED_RATIO[name]
    assert measured is not None, "no measured ratio recorded for this scene"
    if measured < 1:
        assert q["ratio"] < (measured + 1) / 2, q["ratio"]
    else:
        assert abs(q["ratio"] - measured) <= 0.05 * measured, q["ratio"]
