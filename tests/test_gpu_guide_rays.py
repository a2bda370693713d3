"""The device's guide walk, pinned to the host program ray by ray.

guide_walk.h argues its margins for the host walk gw_walk, and tests/test_guide_walk.py holds "0 wrong rays" for the
stand-alone host program.  The kernel does not run gw_walk: the GUIDE step of k_trace_w<1> is a second implementation, on
its own stack, with its own cut / second bookkeeping, its held finished rays, its wave-level fallback append and its
unwalked path.  vmx_guide_trace (Scene.guide_trace) runs that step on explicit rays, and every case here asks, with no
tolerance and no allowed exceptions:

  (a) the pin: the device settles exactly the rays the host program settles (verdict SETTLED or MISS), with the host
      program's reference slot and the bits of its t; every INPUT ray is a fallback ray; vmx_guide_rays agrees;
  (b) the composition: with the launch over the fallback list, every ray carries the oracle's triangle and the bits of
      its t over the reference tree, and what vmx_trace returns;
  (c) exactly one of the two: settled or listed, never both or neither — checked inside the entry, which fails otherwise;
  (d) both forms of the kernel (a hit record per path; dense records) agree on everything.

Rays: the bounce rays of tests/test_guide_walk.py (parity: mostly unwalked; corrected; uniform) on its four scenes and the
duplicate soup, every adversarial construction of guide_spec.adversarial_cases, ray counts around a wave and a block, one
block and three blocks for many refills per lane, two LDS stack levels against the default.  The stack cases assert, from
the host program's report, that the guide is deeper than the LDS levels and deeper than the reference tree.

The lines this file prints (rays, settled, fallback by the host program's reason) are copied to profiles/guide_tree.txt."""
import ctypes as C
import os

import numpy as np
import pytest

import guide_spec as G
import oracle_lib as O
import vermilion_amd as va
from shared_inputs import random_soup, rays_inside_and_outside
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = {"cornell8": (96, 64), "lattice": (96, 64), "bunny70k": (160, 90), "sponza260k": (160, 90)}
CAMERAS = {"cornell8": scenes.cornell_camera, "bunny70k": scenes.bunny_camera, "sponza260k": scenes.sponza_camera,
           "lattice": scenes.lattice_camera}
TREE_KEYS = ("start", "nprims", "right_offset", "bbox", "prim_order")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the rays (no device needed: the mutation counts in profiles/guide_tree.txt come from these on the host program alone)
def bounce_case(name, kinds=("parity", "corrected", "uniform")):
    """(pos, nrm, uv, o, d): the bounce rays test_settled_rays_are_the_oracles feeds the host program for this scene"""
    pos, nrm, uv = getattr(scenes, name)()
    c = CAMERAS[name]()
    W, H = SIZES[name]
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 64)
    osc = O.OracleScene(pos, nrm, uv)
    rays = [G.bounce_rays(osc, cam, 5 + ("parity", "corrected", "uniform").index(k), k) for k in kinds]
    return pos, nrm, uv, np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])


def soup_case():
    """the duplicate soup's camera rays plus uniform bounce rays, as test_soup_settles_no_duplicated_triangle builds them"""
    g = np.load(os.path.join(HERE, "golden", "ref_soup_duplicates.npz"))
    pos, nrm = g["pos"].reshape(-1, 9), g["nrm"].reshape(-1, 9)
    tree = {k: g["bvh_" + k] for k in TREE_KEYS}
    osc = O.OracleScene(pos, nrm, None, tree=tree)
    cam = va.make_camera(g["cam"][:3], g["cam"][3:6], 96, 64, 64)
    o0, d0 = O.primary_rays(cam, va.make_opts(seed=3), 0)
    o1, d1 = G.bounce_rays(osc, cam, 3, "uniform")
    return pos, nrm, None, np.concatenate([o0, o1]), np.concatenate([d0, d1])


def scales_case():
    """700 triangles of the `scales` soup (a few huge over many tiny): its guide is deeper than its reference tree"""
    pos, nrm, uv = random_soup(np.random.default_rng(14), 700, "scales")
    o, d = rays_inside_and_outside(pos, 6000, 21)
    return pos.reshape(-1, 9), nrm.reshape(-1, 9), None, o, d


# ---- the checks
class Pinned:
    """one device scene beside the oracle's, and the host program's answers for one set of rays"""

    def __init__(self, pos, nrm, uv, o, d, gpu=None):
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
        self.o, self.d = np.ascontiguousarray(o, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        self.own = gpu is None
        self.gpu = va.Scene(pos, nrm, uv, device=0) if gpu is None else gpu
        self.cpu = O.OracleScene(pos, nrm, uv)
        self.tree = self.gpu.bvh()
        ref = self.cpu.bvh()
        for k in TREE_KEYS:  # a reference-tree scene: the device's tree is the oracle's
            assert np.array_equal(np.asarray(self.tree[k]).view(np.uint32), np.asarray(ref[k]).view(np.uint32)), k
        self.host = G.host_guide(self.pos, self.tree, self.o, self.d)
        self.tri, self.t = self.cpu.trace(self.o, self.d)

    def close(self):
        if self.own:
            self.gpu.close()

    def report(self, name):
        v = self.host["verdict"]
        print("%s: %d rays, host program settles %d (%d hits, %d misses), fallback %d: %s; guide depth %d, reference tree %d"
              % (name, len(v), int(np.isin(v, (G.SETTLED, G.MISS)).sum()), int(np.sum(v == G.SETTLED)), int(np.sum(v == G.MISS)),
                 int((~np.isin(v, (G.SETTLED, G.MISS))).sum()),
                 ", ".join("%s %d" % (G.REASONS[k], int(np.sum(v == k))) for k in (G.INPUT, G.LIMIT, G.TIE, G.BOX)),
                 self.host["guide_depth"], self.host["ref_depth"]))

    def pin(self, n=None, **kw):
        """(a), (c) and (d) for the first n rays under the entry's keywords; returns (settled, slot, t)"""
        n = len(self.o) if n is None else n
        v, hs, ht = self.host["verdict"][:n], self.host["slot"][:n], self.host["t"][:n]
        want = np.isin(v, (G.SETTLED, G.MISS))
        out = []
        for records in (False, True):
            settled, slot, t = self.gpu.guide_trace(self.o[:n], self.d[:n], records=records, **kw)  # (c): the call succeeds
            s = settled.astype(bool)
            tag = ("records" if records else "plain", kw)
            assert int(np.sum(s != want)) == 0, (tag, "rays settled on one side only", np.flatnonzero(s != want)[:8], v[s != want][:8])
            assert not np.any(s[v == G.INPUT]), tag
            assert int(np.sum(slot[s] != hs[s])) == 0, (tag, "slots differ", np.flatnonzero(s & (slot != hs))[:8])
            assert int(np.sum(bits(t[s]) != bits(ht[s]))) == 0, (tag, "t differs", np.flatnonzero(s & (bits(t) != bits(ht)))[:8])
            assert np.all(slot[s & (v == G.MISS)] == G.NONE), tag
            assert np.all(slot[~s] == G.NONE) and np.all(bits(t[~s]) == 0), tag
            assert self.gpu.guide_rays() == (int(s.sum()), n - int(s.sum())), tag
            assert self.gpu.guide_list_entries() == n, tag
            out.append((settled, slot, t))
        (a, sa, ta), (b, sb, tb) = out
        assert np.array_equal(a, b) and np.array_equal(sa, sb) and np.array_equal(bits(ta), bits(tb)), (kw, "the two forms differ")
        return out[0]

    def compose(self, n=None, **kw):
        """(b) and (d) for the first n rays: with the launch over the fallback list every ray has the oracle's answer"""
        n = len(self.o) if n is None else n
        order = np.asarray(self.tree["prim_order"]).astype(np.int64)
        dtri, dt = self.gpu.trace(self.o[:n], self.d[:n])
        out = []
        for records in (False, True):
            settled, slot, t = self.gpu.guide_trace(self.o[:n], self.d[:n], records=records, complete=True, **kw)
            tag = ("records" if records else "plain", kw)
            tri = np.where(slot == G.NONE, -1, order[np.minimum(slot, len(order) - 1)])
            assert int(np.sum(tri != self.tri[:n])) == 0, (tag, "triangles differ from the oracle's", np.flatnonzero(tri != self.tri[:n])[:8])
            assert int(np.sum(bits(t) != bits(self.t[:n]))) == 0, (tag, "t differs from the oracle's", np.flatnonzero(bits(t) != bits(self.t[:n]))[:8])
            assert np.array_equal(tri, dtri.astype(np.int64)) and np.array_equal(bits(t), bits(dt)), (tag, "differs from vmx_trace")
            out.append((settled, slot, t))
        (a, sa, ta), (b, sb, tb) = out
        assert np.array_equal(a, b) and np.array_equal(sa, sb) and np.array_equal(bits(ta), bits(tb)), (kw, "the two forms differ")
        return out[0]


@pytest.fixture(scope="module")
def bunny():
    """bunny70k under its corrected and uniform bounce rays, about 18 k (a uniform set alone is the camera's 9 k hits):
    real divergence, a guide of 22 levels over a reference tree of 21"""
    p = Pinned(*bounce_case("bunny70k", kinds=("corrected", "uniform")))
    yield p
    p.close()


@pytest.fixture(scope="module")
def cornell():
    p = Pinned(*bounce_case("cornell8", kinds=("uniform",)))
    yield p
    p.close()


@pytest.mark.parametrize("name", ["cornell8", "lattice", "bunny70k", "sponza260k"])
def test_bounce_rays(name):
    p = Pinned(*bounce_case(name))
    try:
        p.report("%s %dx%d" % ((name,) + SIZES[name]))
        nan = ~np.isfinite(p.d).all(axis=1)
        assert nan.any() and np.all(p.host["verdict"][nan] == G.INPUT)  # the unwalked path is in the set
        whole = p.pin()
        assert whole[0].any() and not whole[0].all()
        p.compose()
        # three blocks: every lane takes many rays, so unwalked rays, fallback rays and settled rays meet in one wave's refill
        for x, y in zip(whole, p.pin(grid_blocks=3)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    finally:
        p.close()


def test_soup_no_duplicated_triangle_is_settled_on_the_device():
    pos, nrm, uv, o, d = soup_case()
    p = Pinned(pos, nrm, uv, o, d)
    try:
        p.report("soup 96x64")
        whole = p.pin()
        settled = whole[0]
        # one block and three: a fifth of these rays tie, so finished rays that fall back and rays that are settled share
        # a wave at most refills, and the fallback append comes from partly idle waves
        assert 5 * int((~settled.astype(bool)).sum()) > len(settled) >= 20 * 256
        for blocks in (1, 3):
            for x, y in zip(whole, p.pin(grid_blocks=blocks)):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        _, inverse, counts = np.unique(p.pos, axis=0, return_inverse=True, return_counts=True)
        dup = counts[inverse.reshape(-1)] > 1
        on_dup = (p.tri >= 0) & dup[np.maximum(p.tri, 0)]
        assert on_dup.any()
        assert not np.any(settled[on_dup])
        p.compose()
    finally:
        p.close()


def test_adversarial_scenes_on_the_device():
    """every case of the generator test_adversarial_scenes runs on the host program, same seed, same rays"""
    kinds = set()
    for kind, pos, o, d in G.adversarial_cases():
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
        p = Pinned(pos, G.flat_normals(pos), None, o, d)
        try:
            p.report(kind)
            settled, _, _ = p.pin()
            if kind in ("zero direction component", "origins outside the bounds", "close planes"):
                assert not settled[p.tri >= 0].any(), kind
            if kind == "tie across subtrees":  # the patch is triangles 0-15: each of its hits ties with the pair behind it
                on_patch = (p.tri >= 0) & (p.tri < 16)
                assert on_patch.sum() > 1000 and not settled[on_patch].any()
            p.compose()
        finally:
            p.close()
        kinds.add(kind)
    assert len(kinds) == 11


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000])
def test_ray_counts(cornell, n):
    """a wave that is never full (1, 63), a block that is never full (65, 255), a list that ends inside a reserved chunk
    (every n that is no multiple of 64)"""
    assert len(cornell.o) >= 1000
    if n == 1000:
        cornell.report("cornell8 uniform (the ray counts take its first rays)")
    cornell.pin(n=n)
    cornell.compose(n=n)


@pytest.mark.parametrize("grid_blocks", [1, 3])
def test_refills(bunny, grid_blocks):
    """one block and three: 256 or 768 lanes take about 18 k rays, dozens each, so every refill finds finished and
    running lanes in one wave, and fallback appends come from partly idle waves"""
    n = len(bunny.o)
    assert n >= 20 * 3 * 256
    if grid_blocks == 1:
        bunny.report("bunny70k corrected + uniform 160x90")
    whole = bunny.pin()
    capped = bunny.pin(grid_blocks=grid_blocks)
    for a, b in zip(whole, capped):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    whole = bunny.compose()
    capped = bunny.compose(grid_blocks=grid_blocks)
    for a, b in zip(whole, capped):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _stack_conditions(p):
    # two LDS levels and the bottom entry hold a walk of depth 1: the guide must be deeper, and deeper than the reference
    # tree, the case bind_stack's max exists for
    assert p.host["guide_depth"] + 2 > 2 + 1
    assert p.host["guide_depth"] > p.host["ref_depth"]


@pytest.mark.parametrize("grid_blocks", [0, 1])
def test_stack_two_lds_levels_bunny(bunny, grid_blocks):
    _stack_conditions(bunny)
    shallow = va.make_opts(lds_entries=2)
    a = bunny.pin(grid_blocks=grid_blocks)
    b = bunny.pin(opts=shallow, grid_blocks=grid_blocks)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    bunny.compose(opts=shallow, grid_blocks=grid_blocks)


def test_stack_two_lds_levels_scales_soup():
    p = Pinned(*scales_case())
    try:
        p.report("scales soup, 700 triangles")
        _stack_conditions(p)
        shallow = va.make_opts(lds_entries=2)
        a = p.pin()
        assert a[0].any()
        for kw in (dict(opts=shallow), dict(opts=shallow, grid_blocks=1), dict(grid_blocks=1)):
            b = p.pin(**kw)
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
            p.compose(**kw)
    finally:
        p.close()


def test_rebuild_gives_a_fresh_scenes_results_and_a_refit_refuses(cornell):
    moved = np.array(cornell.pos, np.float32, copy=True)
    moved[0, 0] += 0.25
    nrm, o, d = scenes.cornell8()[1], cornell.o, cornell.d
    with va.Scene(cornell.pos, nrm, None, device=0) as sc:
        sc.update(pos=moved)
        with pytest.raises(L.VmxError) as e:
            sc.guide_trace(o, d)
        assert e.value.code == L.VMX_ERR_INVALID
        sc.update(pos=moved, rebuild=True)
        p = Pinned(moved, nrm, None, o, d, gpu=sc)
        p.report("cornell8 with a moved vertex, rebuilt")
        rebuilt = p.pin()
        rebuilt_all = p.compose()
        with va.Scene(moved, nrm, None, device=0) as fresh:
            for kw, want in ((dict(), rebuilt), (dict(complete=True), rebuilt_all)):
                got = fresh.guide_trace(o, d, **kw)
                for x, y in zip(got, want):
                    assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_refusals(cornell):
    o, d, n = cornell.o[:300], cornell.d[:300], 300
    before = cornell.gpu.guide_trace(o, d)
    lib = L.lib()

    def raw(h, po, pd, popts, flags, ps, pslot, pt):
        return lib.vmx_guide_trace(h, po, pd, n, popts, flags, 0, ps, pslot, pt)

    def still_works():
        after = cornell.gpu.guide_trace(o, d)
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))

    opts = va.make_opts()
    s, sl, t = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.float32)
    args = [cornell.gpu._h, o.ctypes.data, d.ctypes.data, C.byref(opts), 0, s.ctypes.data, sl.ctypes.data, t.ctypes.data]
    assert raw(*args) == L.VMX_OK
    for k in (0, 1, 2, 3, 5, 6, 7):  # NULL for each pointer in turn
        a = list(args)
        a[k] = None
        assert raw(*a) == L.VMX_ERR_INVALID, k
        assert b"NULL" in lib.vmx_last_error()
    still_works()
    for flags in (4, 8, 0x80000000, 0xFFFFFFFC):
        a = list(args)
        a[4] = flags
        assert raw(*a) == L.VMX_ERR_INVALID, flags
    still_works()
    with pytest.raises(L.VmxError) as e:
        cornell.gpu.guide_trace(o, d, opts=va.make_opts(collect_counters=True))
    assert e.value.code == L.VMX_ERR_INVALID
    still_works()
    nrm = scenes.cornell8()[1]
    for builder in (L.VMX_BVH_SAH, L.VMX_BVH_LBVH, L.VMX_BVH_PLOC):
        with va.Scene(cornell.pos, nrm, None, device=0, builder=builder) as other:
            with pytest.raises(L.VmxError) as e:
                other.guide_trace(o, d)
            assert e.value.code == L.VMX_ERR_INVALID, builder
            tri, _ = other.trace(o, d)  # ... and the scene goes on working
            assert len(tri) == n and np.array_equal(tri >= 0, cornell.tri[:n] >= 0)
    # no rays: nothing happens, the last call's counts stay
    counts = cornell.gpu.guide_rays()
    e0 = np.zeros((0, 3), np.float32)
    got = cornell.gpu.guide_trace(e0, e0)
    assert all(len(x) == 0 for x in got) and cornell.gpu.guide_rays() == counts
    still_works()
