"""Light-sampled progressive handles (vmx_progressive_begin_nee) and budgeted steps (vmx_progressive_budget_device /
step_budget_device / step_budgeted) on the device.  Every comparison is bit for bit: whatever the schedule of steps, maps
and budgets, a handle run to completion holds vmx_render_nee's frame, which is tests/nee_spec.py's; the state in between is
tests/sampling_spec.py's fold of nee_spec's per-sample radiance on the streams (seed, p, k); the budgets are
tests/budget_spec.py's, uint32 for uint32.

Shapes: 37 x 5 (185 pixels: a width that is no multiple of 64, three waves, the last one partial) and 48 x 32 (1,536: more
than one block of every per-pixel kernel), kmax 8 .. 16."""
import functools

import numpy as np
import pytest

import budget_spec as BS
import demod_spec as DS
import filter_spec as FS
import nee_cases as K
import nee_spec as N
import oracle_lib as O
import sampling_spec as SS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
F = np.float32
SEED = 5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what):
    diff = bits(np.asarray(got, F)) != bits(np.asarray(want, F))
    assert not diff.any(), "%s: %d of %d values differ, first at %s" % (what, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def camera(scene, W, H, spp):
    c = scenes.cornell_camera() if scene == "cornell8" else scenes.lattice_camera()
    return va.make_camera(c["position"], c["rotation_deg"], W, H, spp)


def device_scene(scene, table, channels, builder=L.VMX_BVH_REFERENCE):
    pos, nrm, uv, _, _, _ = K.golden(scene)
    sc = va.Scene(pos, nrm, uv, spheres=K.table(table), builder=builder)
    if channels:
        sc.bind_texture(K.texture(channels))
    return sc


class Spec:
    """nee_spec's answer for one (scene, table, texture, frame): the radiance of sample k of every pixel, [kmax, H, W, 4],
    and the ray counts per k — computed once, shared, never written to"""

    def __init__(self, scene, table, channels, W, H, spp, tree=False):
        pos, nrm, uv, _, _, _ = K.golden(scene)
        self.tb = K.table(table)
        self.tex = K.texture(channels) if channels else None
        t = None
        if tree:
            with device_scene(scene, table, 0, builder=L.VMX_BVH_LBVH) as sc:
                t = sc.bvh()
        self.osc = O.OracleScene(pos, nrm, uv, spheres=self.tb, tree=t)
        if self.tex is not None:
            self.osc.bind_texture(self.tex)
        self.cam, self.opts = camera(scene, W, H, spp), K.opts(SEED)
        self.W, self.H, self.kmax = W, H, 4 * (spp // 4)
        npix = W * H
        pix = np.arange(npix, dtype=np.int64)
        self.rays = []
        self.samples = np.empty((self.kmax, H, W, 4), F)
        self.stats = []
        for k in range(self.kmax):
            o, d = O.primary_rays(self.cam, self.opts, k)
            self.rays.append((o, d))
            s, st = N.radiance(self.osc, o, d, SEED, self.tb, self.opts.sampling, True, self.tex, pix, np.full(npix, k, np.int64))
            self.samples[k] = s.reshape(H, W, 4)
            self.stats.append(st)
        self.samples.setflags(write=False)

    def total(self, key):
        return sum(st[key] for st in self.stats)

    def sums(self, counts):
        """the moments state of a handle whose pixel (y, x) folded its samples 0 .. counts[y, x] - 1"""
        counts = np.asarray(counts).astype(np.int64)
        acc = np.zeros((self.H, self.W, 4), F)
        for k in range(int(counts.max())):
            m = counts > k
            acc[m] = SS.fold(self.samples[k][m][None, :, :3], acc[m])
        return acc

    def frame(self, counts):
        """k_resolve's pixel write of every pixel's first counts[y, x] samples (a preview's unfinished pixels included)"""
        counts = np.broadcast_to(np.asarray(counts), (self.H, self.W)).astype(np.int64)
        acc = self.sums(counts)[..., :3]
        out = np.zeros((self.H, self.W, 5), F)
        fn = counts.astype(F)
        with np.errstate(all="ignore"):
            m = acc / fn[..., None]
        m = np.where(F(1) < m, F(1), m)
        out[..., :3] = np.where(m < F(0), F(0), m)
        out[..., 3] = F(1)
        out[..., 4] = fn
        out[counts == 0] = [0, 0, 0, 1, 0]  # (a pixel without a sample, as k_preview shows it)
        return out

    def paths(self, counts, take):
        """the ray counts of the samples counts[p] .. counts[p] + take[p] - 1 of every pixel p, by one call of the spec on
        exactly those paths"""
        counts, take = np.asarray(counts).reshape(-1).astype(np.int64), np.asarray(take).reshape(-1).astype(np.int64)
        pix = np.repeat(np.arange(counts.size), take)
        k = np.concatenate([np.arange(c, c + t) for c, t in zip(counts, take)]) if pix.size else np.zeros(0, np.int64)
        o = np.stack([self.rays[kk][0][p] for p, kk in zip(pix, k)]) if pix.size else np.zeros((0, 3), F)
        d = np.stack([self.rays[kk][1][p] for p, kk in zip(pix, k)]) if pix.size else np.zeros((0, 3), F)
        rad, st = N.radiance(self.osc, o, d, SEED, self.tb, self.opts.sampling, True, self.tex, pix, k)
        same(rad, self.samples.reshape(self.kmax, -1, 4)[k, pix], "the spec on a list of paths")
        return st


@functools.lru_cache(maxsize=None)
def spec(scene, table, channels, W, H, spp, tree=False):
    return Spec(scene, table, channels, W, H, spp, tree)


def state(p):
    """(sums [rows, W, 4] float32, counts [rows, W] int32) of the handle, read back"""
    import torch
    sums = torch.empty(p.shape + (4,), dtype=torch.float32, device="cuda")
    counts = torch.empty(p.shape, dtype=torch.int32, device="cuda")
    p.state_device(sums, counts)
    p.preview()  # (the host entry synchronises the handle's stream)
    return sums.cpu().numpy(), counts.cpu().numpy()


def budgets_of(p, params=None):
    import torch
    b = torch.full(p.shape, -1, dtype=torch.int32, device="cuda")
    t = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    p.budget_device(b, t, params)
    p.preview()
    return b.cpu().numpy().view(np.uint32), int(t.item())


def add(tot, st):
    for k in tot:
        tot[k] += st[k]


# ---- a. completion -----------------------------------------------------------------------------------------------------------
CASES = [("cornell8", "default", 0, 48, 32, 8), ("lattice", "overlap", 0, 37, 5, 8), ("cornell8", "three", 0, 37, 5, 12),
         ("cornell8", "single", 3, 37, 5, 8)]


def test_the_frame_from_the_shared_samples_is_nee_specs_frame():
    sp = spec("lattice", "overlap", 0, 37, 5, 8)
    want, wst = N.frame(sp.osc, sp.cam, sp.opts, sp.tb, sp.tex)
    same(sp.frame(8), want, "frame")
    assert all(sp.total(k) == wst[k] for k in ("rays_primary", "rays_secondary", "samples"))


@pytest.mark.parametrize("schedule", ["all", "ones", "threes", "batch1"])
@pytest.mark.parametrize("scene,table,channels,W,H,spp", CASES)
def test_a_completed_handle_holds_render_nees_frame(scene, table, channels, W, H, spp, schedule):
    sp = spec(scene, table, channels, W, H, spp)
    kmax = sp.kmax
    opts = K.opts(SEED, samples_per_batch=1 if schedule == "batch1" else 0)
    step = {"all": 0, "ones": 1, "threes": 3, "batch1": 0}[schedule]
    with device_scene(scene, table, channels) as sc:
        one, ost = sc.render_nee(sp.cam, opts)
        # the one-call entry is what it was: the spec's frame and counts, a pass per sample under samples_per_batch = 1
        same(one, sp.frame(kmax), "render_nee")
        assert ost["samples"] == W * H * kmax == sp.total("samples")
        assert ost["rays_primary"] == sp.total("rays_primary") and ost["rays_secondary"] == sp.total("rays_secondary")
        if schedule == "batch1":
            assert ost["passes"] == kmax
        with sc.progressive_nee(sp.cam, opts) as p:
            tot = dict(rays_primary=0, rays_secondary=0, samples=0, passes=0)
            steps, done = 0, 0
            while p.info()["pixels_active"]:
                st = p.step(step)
                take = min(step, kmax - done) if step else kmax - done
                assert st["samples"] == W * H * take
                done += take
                steps += 1
                add(tot, st)
                info = p.info()
                assert (info["samples"], info["steps"], info["passes"]) == (W * H * done, steps, tot["passes"])
                assert info["pixels_active"] == (0 if done == kmax else W * H)
            assert steps == (1 if step == 0 else -(-kmax // step)) and (info["width"], info["rows"], info["kmax"]) == (W, H, kmax)
            same(p.preview(), one, "the completed handle")
            assert all(tot[k] == ost[k] for k in ("rays_primary", "rays_secondary", "samples"))
            if schedule == "batch1":
                assert tot["passes"] == kmax
            assert p.step(0)["samples"] == 0 and p.info()["steps"] == steps  # nothing left


# ---- b. previews -------------------------------------------------------------------------------------------------------------
def test_plain_previews():
    """after n < kmax samples the preview is the clamped mean of the frame's own first n samples, the fifth float n.  (Not
    vmx_render_nee's frame at rays_per_pixel = n: sample k's film stratum is k / (rays_per_pixel / 4), primary_ray, so the
    first n samples of a kmax-sample frame are not the samples of an n-sample frame — for plain handles neither.)"""
    sp = spec("cornell8", "default", 0, 48, 32, 8)
    opts = sp.opts
    with device_scene("cornell8", "default", 0) as sc:
        with sc.progressive(sp.cam, opts) as plain:
            empty = plain.preview()
        four = sp.frame(4)
        with sc.progressive_nee(sp.cam, opts) as p:
            same(p.preview(), empty, "before the first step")
            p.step(3)
            same(p.preview(), sp.frame(3), "after 3 samples")
            p.step(1)
            got, q = p.preview(rgba8=True)
            same(got, four, "after 4 samples")
            assert (got[..., 4] == 4).all()
            assert np.array_equal(q, np.floor(got[..., :4] * F(255)).astype(np.uint8))
            import torch
            d5 = torch.empty((32, 48, 5), dtype=torch.float32, device="cuda")
            p.preview_device(d5)
            p.preview()
            same(d5.cpu().numpy(), four, "preview_device")


def test_filtered_and_demodulated_previews():
    sp = spec("cornell8", "single", 3, 37, 5, 8)
    with device_scene("cornell8", "single", 3) as sc:
        raw = sc.raycast_camera(sp.cam, sp.opts, 0)["raw"]
        n, z = FS.guide_of(raw.cpu().numpy())
        plane = sc.albedo_camera(sp.cam, sp.opts, samples=4).cpu().numpy()
        with sc.progressive_nee(sp.cam, sp.opts) as p:
            for at in (3, 8):
                p.step(3 if at == 3 else 0)
                plain = p.preview()
                same(plain, sp.frame(at), "preview at %d" % at)
                assert FS.same_bits(p.preview_filtered(), FS.filtered_frame(plain, n, z)), at
                assert FS.same_bits(p.preview_filtered(albedo_samples=4), DS.demodulated_frame(plain, n, z, plane)), at
                same(p.preview(), plain, "nothing changed")


# ---- c. moments ---------------------------------------------------------------------------------------------------------------
def test_moments_state_error_and_selection():
    import torch
    sp = spec("cornell8", "default", 0, 48, 32, 8)
    W, H, kmax = sp.W, sp.H, sp.kmax
    with device_scene("cornell8", "default", 0) as sc:
        with sc.progressive_nee(sp.cam, sp.opts, moments=True) as p, sc.progressive_nee(sp.cam, sp.opts) as q:
            for at, step in ((1, 1), (5, 4), (8, 0)):
                p.step(step), q.step(step)
                sums, counts = state(p)
                assert (counts == at).all()
                same(sums, sp.sums(counts), "sums and m2 at %d" % at)
                qs, qc = state(q)
                same(qs[..., :3], sums[..., :3], "a handle without moments: the same colour sums")
                assert not qs[..., 3].any() and np.array_equal(qc, counts)
                same(q.preview(), p.preview(), "the same frames")
                for prm in (None, va.make_sampling_params(threshold=0.2, floor=0.01, min_samples=4, radius=2)):
                    d = SS.params_of(prm)
                    e, v = torch.empty((H, W), dtype=torch.float32, device="cuda"), torch.empty((H, W), dtype=torch.float32, device="cuda")
                    m, c = torch.full((H, W), 7, dtype=torch.uint8, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
                    p.error_device(e, v, prm), p.select_device(m, c, prm)
                    p.preview()
                    we, wv = SS.error_variance(sums, counts, d["floor"])
                    same(e.cpu().numpy(), we, "error"), same(v.cpu().numpy(), wv, "variance")
                    wm = SS.select(sums, counts, kmax, **d)
                    assert np.array_equal(m.cpu().numpy(), wm) and int(c.item()) == int(wm.sum())
            same(p.preview(), sp.frame(kmax), "complete")


# ---- d. selected and adaptive steps -------------------------------------------------------------------------------------------
def maps_of(n, kmax):
    rows, w = n.shape
    yy, xx = np.mgrid[0:rows, 0:w]
    one = np.zeros((rows, w), np.uint8)
    one[rows // 2, w // 3] = 1
    return {"checker": (((xx + yy) & 1) * 3).astype(np.uint8), "one": one, "none": np.zeros((rows, w), np.uint8),
            "finished_too": ((n >= kmax) | (xx % 3 == 0)).astype(np.uint8)}


@pytest.mark.parametrize("scene,table,channels,W,H,spp", [CASES[0], CASES[2]])
def test_ragged_sequences_then_completion(scene, table, channels, W, H, spp):
    sp = spec(scene, table, channels, W, H, spp)
    kmax = sp.kmax
    with device_scene(scene, table, channels) as sc, sc.progressive_nee(sp.cam, sp.opts, moments=True) as p:
        n = np.zeros((H, W), np.int64)
        tot = dict(rays_primary=0, rays_secondary=0, samples=0)
        steps = 0
        for name, samples in (("checker", 3), ("one", 0), ("none", 2), ("checker", 5), ("finished_too", 2)):
            m = maps_of(n, kmax)[name]
            before = state(p)[0]
            st, nsel = p.step_selected(samples, dev(m))
            take = np.where((n < kmax) & (m != 0), np.minimum(samples if samples else kmax, kmax - n), 0)
            assert (nsel, st["samples"]) == (int((take > 0).sum()), int(take.sum())), name
            n = n + take
            steps += nsel > 0
            sums, counts = state(p)
            assert np.array_equal(counts, n), name
            same(sums, sp.sums(n), "state after " + name)
            same(sums[take == 0], before[take == 0], "unselected pixels after " + name)
            same(p.preview(), sp.frame(n), "preview after " + name)
            info = p.info()
            assert info["pixels_active"] == int((n < kmax).sum()) and info["steps"] == steps
            add(tot, st)
        assert (n >= kmax).any() and (n < kmax).any()
        add(tot, p.step(0))
        same(p.preview(), sp.frame(kmax), "complete")
        assert all(tot[k] == sp.total(k) for k in tot)


def test_step_adaptive_is_select_then_step_selected():
    import torch
    sp = spec("cornell8", "default", 0, 48, 32, 8)
    prm = va.make_sampling_params(threshold=0.3, floor=0.01, min_samples=3, radius=1)
    with device_scene("cornell8", "default", 0) as sc:
        with sc.progressive_nee(sp.cam, sp.opts, moments=True) as a, sc.progressive_nee(sp.cam, sp.opts, moments=True) as b:
            a.step(2), b.step(2)
            seen = set()
            for _ in range(3):
                sa, na = a.step_adaptive(2, prm)
                m = torch.empty(b.shape, dtype=torch.uint8, device="cuda")
                b.select_device(m, None, prm)
                sb, nb = b.step_selected(2, m)
                assert na == nb and sa["samples"] == sb["samples"]
                (s1, c1), (s2, c2) = state(a), state(b)
                same(s1, s2, "sums"), same(s1, sp.sums(c1), "against the spec")
                assert np.array_equal(c1, c2)
                seen.add(na)
            assert len(seen) > 1 and 0 < min(seen) < 48 * 32  # the error selects: neither everything nor nothing
            a.step(0)
            same(a.preview(), sp.frame(sp.kmax), "complete")


# ---- e. budgets -----------------------------------------------------------------------------------------------------------------
BUDGET_PARAMS = [dict(), dict(threshold=0.2, floor=0.01, min_samples=4, radius=2), dict(threshold=0.0, min_samples=2, radius=0),
                 dict(threshold=0.05, radius=3, max_step=3), dict(threshold=0.3, floor=0.01, min_samples=3, radius=1, max_step=100)]


@pytest.mark.parametrize("W,H,spp,batch", [(48, 32, 8, 0), (37, 5, 16, 8)])
def test_budget_device_is_the_restatement(W, H, spp, batch):
    sp = spec("cornell8", "default", 0, W, H, spp)
    kmax = sp.kmax
    B = batch if batch else kmax
    opts = K.opts(SEED, samples_per_batch=batch)
    with device_scene("cornell8", "default", 0) as sc, sc.progressive_nee(sp.cam, opts, moments=True) as p:
        yy, xx = np.mgrid[0:H, 0:W]
        for how in ("begin", "uniform", "ragged", "more", "finished"):
            if how == "uniform":
                p.step(3)
            elif how == "ragged":
                p.step_selected(4, dev(((xx + yy) % 3 == 0).astype(np.uint8)))
            elif how == "more":
                p.step_adaptive(2, va.make_sampling_params(threshold=0.3, min_samples=2))
            elif how == "finished":
                p.step_selected(0, dev((xx % 5 == 0).astype(np.uint8)))
            sums, counts = state(p)
            for kw in BUDGET_PARAMS:
                got, total = budgets_of(p, va.make_sampling_budget_params(**kw))
                want = BS.budget(sums, counts, kmax, B, **dict(BS.DEFAULTS, **kw))
                assert np.array_equal(got, want), (how, kw, np.argwhere(got != want)[:4].tolist())
                assert total == int(want.sum(dtype=np.int64)), (how, kw)
                sel = SS.select(sums, counts, kmax, **{k: v for k, v in dict(SS.DEFAULTS, **kw).items() if k != "max_step"})
                assert np.array_equal(got != 0, sel == 1), (how, kw)
            got, _ = budgets_of(p)
            assert np.array_equal(got, BS.budget(sums, counts, kmax, B)), how  # params NULL: the defaults
        assert len(np.unique(counts)) >= 3 and (counts == kmax).any()


def hand_made_plane(counts, kmax, late):
    """budgets 0, 1, 2, 7, 8, 9, 1000 scattered over the image, 14 at the pixel `late`; the item total no multiple of 64"""
    r = np.random.RandomState(11)
    b = r.choice([0, 0, 1, 2, 7, 8, 9, 1000], counts.shape).astype(np.int64)
    b[late] = 14
    take = BS.step_counts(counts, b, kmax, 8)
    if take.sum() % 64 == 0:
        b[0, 0] = 1 if b[0, 0] != 1 else 2
    return b


def test_step_budget_with_a_hand_made_plane():
    W, H, kmax, B = 37, 5, 16, 8
    sp = spec("cornell8", "default", 0, W, H, 16)
    opts = K.opts(SEED, samples_per_batch=B)
    late = (2, 11)
    with device_scene("cornell8", "default", 0) as sc, sc.progressive_nee(sp.cam, opts, moments=True) as p:
        p.step(3)
        one = np.zeros((H, W), np.uint8)
        one[late] = 1
        p.step_selected(10, dev(one))
        sums0, n0 = state(p)
        assert n0[late] == 13 and (np.delete(n0.reshape(-1), late[0] * W + late[1]) == 3).all()
        b = hand_made_plane(n0, kmax, late)
        assert set(np.unique(b)) == {0, 1, 2, 7, 8, 9, 14, 1000}
        info0 = p.info()
        st, nsel = p.step_budget(dev(b.astype(np.int32)))
        want_sums, want_n, take = BS.step(sums0, n0, b, kmax, B, sp.samples)
        assert take[late] == 3 and take.max() == 8 and take.sum() % 64 != 0
        assert np.array_equal(take, np.minimum(np.minimum(b, 8), kmax - n0))
        sums, n = state(p)
        assert np.array_equal(n, n0 + take) and np.array_equal(n, want_n)
        same(sums, want_sums, "sums and m2")
        same(sums, sp.sums(n), "sums and m2, from the first sample on")
        same(sums[b == 0], sums0[b == 0], "pixels with budget 0")
        wst = sp.paths(n0, take)
        assert st["samples"] == int(take.sum()) == wst["samples"] and nsel == int((take > 0).sum())
        assert st["rays_primary"] == wst["rays_primary"] and st["rays_secondary"] == wst["rays_secondary"]
        assert st["passes"] == 1
        info = p.info()
        assert info["steps"] == info0["steps"] + 1 and info["passes"] == info0["passes"] + 1
        assert info["samples"] == info0["samples"] + int(take.sum()) and info["pixels_active"] == int((n < kmax).sum())
        same(p.preview(), sp.frame(n), "preview")
        # any further schedule ends at render_nee's frame
        p.step(2)
        p.step_budget(dev(np.full((H, W), 5, np.int32)))
        p.step_selected(1, dev(np.ones((H, W), np.uint8)))
        p.step(0)
        assert p.info()["pixels_active"] == 0
        same(p.preview(), sp.frame(kmax), "complete")
        same(p.preview(), sc.render_nee(sp.cam, opts)[0], "render_nee")


def test_step_budget_edge_cases():
    W, H, kmax = 37, 5, 8
    sp = spec("lattice", "overlap", 0, W, H, 8)
    with device_scene("lattice", "overlap", 0) as sc, sc.progressive_nee(sp.cam, sp.opts) as p:  # (no moments: the step needs none)
        # all-zero budgets: nothing happens, on a fresh handle too
        st, nsel = p.step_budget(dev(np.zeros((H, W), np.int32)))
        assert (nsel, st["samples"], st["passes"]) == (0, 0, 0) and p.info()["steps"] == 0 and p.info()["pixels_active"] == W * H
        # one pixel, from zero samples
        b = np.zeros((H, W), np.int32)
        b[4, 36] = 3
        st, nsel = p.step_budget(dev(b))
        n = b.astype(np.int64)
        assert (nsel, st["samples"], st["passes"]) == (1, 3, 1) and np.array_equal(state(p)[1], n)
        same(state(p)[0][..., :3], sp.sums(n)[..., :3], "one pixel")
        assert not state(p)[0][..., 3].any()
        # every pixel at budget 1: a second budgeted step, on a handle that is ragged already
        st, nsel = p.step_budget(dev(np.ones((H, W), np.int32)))
        n = n + 1
        assert (nsel, st["samples"]) == (W * H, W * H) and np.array_equal(state(p)[1], n)
        wst = sp.paths(n - 1, np.ones((H, W), np.int64))
        assert st["rays_primary"] == wst["rays_primary"] and st["rays_secondary"] == wst["rays_secondary"]
        same(p.preview(), sp.frame(n), "preview")
        # budgets past kmax, and for the pixels that then are finished
        big = np.full((H, W), 0x7FFFFFFF, np.int32)
        st, nsel = p.step_budget(dev(big))
        assert nsel == W * H and st["samples"] == int((kmax - n).sum()) and p.info()["pixels_active"] == 0
        st, nsel = p.step_budget(dev(big))
        assert (nsel, st["samples"]) == (0, 0) and p.info()["steps"] == 3
        same(p.preview(), sp.frame(kmax), "complete")


def test_step_budgeted_is_budget_device_then_step_budget():
    import torch
    sp = spec("cornell8", "default", 0, 48, 32, 8)
    prm = va.make_sampling_budget_params(threshold=0.3, min_samples=3, radius=1)
    with device_scene("cornell8", "default", 0) as sc:
        with sc.progressive_nee(sp.cam, sp.opts, moments=True) as a, sc.progressive_nee(sp.cam, sp.opts, moments=True) as b:
            a.step(3), b.step(3)
            for _ in range(3):
                sa, na = a.step_budgeted(prm)
                plane = torch.empty(b.shape, dtype=torch.int32, device="cuda")
                b.budget_device(plane, None, prm)
                sb, nb = b.step_budget(plane)
                assert na == nb and na > 0 and all(sa[k] == sb[k] for k in ("samples", "rays_primary", "rays_secondary", "passes"))
                (s1, c1), (s2, c2) = state(a), state(b)
                same(s1, s2, "sums"), same(s1, sp.sums(c1), "against the spec")
                assert np.array_equal(c1, c2) and a.info() == b.info()
            assert len(np.unique(c1)) >= 3
            a.step(0)
            same(a.preview(), sp.frame(sp.kmax), "complete")


@pytest.mark.parametrize("batch,max_step,min_samples", [(0, 0, 2), (8, 0, 4), (8, 3, 2)])
def test_repeated_budgeted_steps_with_a_zero_threshold_finish_the_frame(batch, max_step, min_samples):
    """every pixel with any error asks for the cap, so the frame is done within ceil((kmax - min_samples) / cap) + 1 steps —
    unless a pixel shows no error at all (E = 0 is not above 0): such pixels stop at min_samples, and the run ends with "no
    pixel selected"; a plain step then completes them"""
    W, H, kmax = 37, 5, 16
    sp = spec("cornell8", "default", 0, W, H, 16)
    opts = K.opts(SEED, samples_per_batch=batch)
    B = batch if batch else kmax
    cap = BS.cap_of(B, max_step)
    prm = va.make_sampling_budget_params(threshold=0.0, min_samples=min_samples, radius=3, max_step=max_step)
    with device_scene("cornell8", "default", 0) as sc, sc.progressive_nee(sp.cam, opts, moments=True) as p:
        steps = 0
        while True:
            sums, counts = state(p)
            want = BS.budget(sums, counts, kmax, B, 0.0, BS.DEFAULTS["floor"], min_samples, 3, max_step)
            st, nsel = p.step_budgeted(prm)
            assert nsel == int((want != 0).sum()) and st["samples"] == int(BS.step_counts(counts, want, kmax, B).sum())
            if nsel == 0:
                break
            steps += 1
            assert steps <= 64
        assert p.info()["pixels_active"] == 0, "a window of 7 x 7 without any error in a lit Cornell frame"
        assert steps <= -(-(kmax - min_samples) // cap) + 1
        same(p.preview(), sp.frame(kmax), "complete")
        same(p.preview(), sc.render_nee(sp.cam, opts)[0], "render_nee")


# ---- f. refusals that need a handle -------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    import torch
    W, H = 37, 5
    sp = spec("cornell8", "default", 0, W, H, 8)
    pos = K.golden("cornell8")[0]
    plane = torch.ones((H, W), dtype=torch.int32, device="cuda")
    total = torch.zeros((1,), dtype=torch.int64, device="cuda")

    def refused(call, match):
        with pytest.raises(va.VmxError, match=match) as e:
            call()
        assert e.value.code == L.VMX_ERR_INVALID

    with device_scene("cornell8", "default", 0) as sc:
        lib = sc._lib
        # a plain handle, with or without moments: no budget entry
        for moments in (False, True):
            with sc.progressive(sp.cam, sp.opts, moments=moments) as p:
                for call in (lambda: p.budget_device(plane), lambda: p.step_budget(plane), lambda: p.step_budgeted()):
                    refused(call, "light-sampled handles only")
                assert p.info()["steps"] == 0
        # a light-sampled handle without moments: the step works, what needs the second moment is refused
        with sc.progressive_nee(sp.cam, sp.opts) as p:
            refused(lambda: p.budget_device(plane), "VMX_PROGRESSIVE_MOMENTS")
            refused(lambda: p.step_budgeted(), "VMX_PROGRESSIVE_MOMENTS")
            refused(lambda: p.error_device(torch.empty((H, W), dtype=torch.float32, device="cuda")), "VMX_PROGRESSIVE_MOMENTS")
            assert p.step_budget(plane)[1] == W * H
        with sc.progressive_nee(sp.cam, sp.opts, moments=True) as p:
            # host pointers where device pointers are due
            host = np.ones((H, W), np.int64)
            hp = C.c_void_p(host.ctypes.data)
            for call in (lambda: lib.vmx_progressive_budget_device(p._h, None, hp, None),
                         lambda: lib.vmx_progressive_budget_device(p._h, None, C.c_void_p(plane.data_ptr()), hp),
                         lambda: lib.vmx_progressive_step_budget_device(p._h, hp, None, None)):
                assert call() == L.VMX_ERR_INVALID and "device" in lib.vmx_last_error().decode(), lib.vmx_last_error()
            # buffers that overlap at the image's size, though not in their first element
            big = torch.zeros((H * W + 8,), dtype=torch.int32, device="cuda")
            assert lib.vmx_progressive_budget_device(p._h, None, C.c_void_p(big.data_ptr()), C.c_void_p(big.data_ptr() + 64)) == L.VMX_ERR_INVALID
            assert "overlap" in lib.vmx_last_error().decode()
            assert lib.vmx_progressive_budget_device(p._h, None, C.c_void_p(big.data_ptr()), C.c_void_p(big.data_ptr() + H * W * 4 + 4)) == L.VMX_OK
            assert p.info()["steps"] == 0
            # the Python layer checks its tensors before the library sees them
            with pytest.raises(ValueError):
                p.step_budget(torch.ones((H, W), dtype=torch.float32, device="cuda"))
            with pytest.raises(ValueError):
                p.budget_device(torch.ones((W, H), dtype=torch.int32, device="cuda"))
            with pytest.raises(ValueError):
                p.budget_device(plane, torch.zeros((1,), dtype=torch.int32, device="cuda"))
            # a scene updated since begin
            p.step(2)
            sc.update(pos=pos)
            for call in (lambda: p.step(1), lambda: p.step_budget(plane), lambda: p.step_budgeted(), lambda: p.step_adaptive(1),
                         lambda: p.step_selected(1, torch.ones((H, W), dtype=torch.uint8, device="cuda"))):
                refused(call, "scene updated since vmx_progressive_begin")
            p.budget_device(plane, total), state(p)  # reading the state still works
            assert p.info()["steps"] == 1


# ---- g. the scene's state ------------------------------------------------------------------------------------------------------
def test_a_handle_follows_the_scenes_state():
    """begun after set_spheres with another emitter count and after bind_texture, a handle completes to that scene's frame"""
    pos, nrm, uv, _, _, _ = K.golden("cornell8")
    W, H = 37, 5
    with va.Scene(pos, nrm, uv) as sc:
        sc.set_spheres(K.table("three"))
        sp = spec("cornell8", "three", 0, W, H, 12)
        with sc.progressive_nee(sp.cam, sp.opts, moments=True) as p:
            p.step(5), p.step_budgeted(va.make_sampling_budget_params(threshold=0.1, min_samples=6)), p.step(0)
            same(p.preview(), sp.frame(sp.kmax), "after set_spheres")
            same(p.preview(), sc.render_nee(sp.cam, sp.opts)[0], "after set_spheres, render_nee")
        sc.set_spheres(K.table("single"))
        sc.bind_texture(K.texture(3))
        sp = spec("cornell8", "single", 3, W, H, 8)
        with sc.progressive_nee(sp.cam, sp.opts, moments=True) as p:
            p.step(3), p.step_budgeted(va.make_sampling_budget_params(threshold=0.1, min_samples=4)), p.step(0)
            same(p.preview(), sp.frame(sp.kmax), "after bind_texture")


def test_a_handle_on_a_device_built_tree():
    sp = spec("lattice", "default", 0, 37, 5, 8, True)
    with device_scene("lattice", "default", 0, builder=L.VMX_BVH_LBVH) as sc, sc.progressive_nee(sp.cam, sp.opts, moments=True) as p:
        p.step(3)
        st, nsel = p.step_budgeted(va.make_sampling_budget_params(threshold=0.1, min_samples=4, max_step=2))
        assert nsel > 0
        sums, n = state(p)
        same(sums, sp.sums(n), "state")
        p.step(0)
        same(p.preview(), sp.frame(sp.kmax), "LBVH frame")
        same(p.preview(), sc.render_nee(sp.cam, sp.opts)[0], "render_nee")
