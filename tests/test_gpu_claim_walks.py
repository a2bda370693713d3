"""The claim tables when the list walks run in dense waves (k_pixel_claims: the claim of every pixel and one ballot word
per tile; the scan and scatter of the live list; k_pixel_lists: one lane per pixel that may get a list).  Both planes
stay the host program's (tests/cpp/pixel_claim_list_test.cpp) bit for bit at the shapes where a compaction can go wrong:
frames smaller than a tile and no multiple of one, no pixel to walk for, almost every pixel, counts around one and four
waves of entries, stripes whose rows end inside a tile, and a smaller frame after a larger one on the same scene.
Frames that take the tables equal the oracle's and the frames with lists off.

Every table is compared after a first call with another camera on the same scene has filled both planes with other
values: a pixel the kernels leave unwritten shows up as a difference."""
import os

import numpy as np
import pytest

import claim_list_spec as LS
import oracle_lib as O
import pixel_claim_spec as S
import vermilion_amd as va
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NONE = LS.NONE
NO_LISTS = 0x2000
NO_FUSE = 0x1000
COUNT_KEYS = ("rays_primary", "rays_secondary", "samples", "samples_discarded", "passes")
FRONT = dict(position=(0.0, 0.0, 5.0), rotation_deg=(25.0, 30.0, 0.0))  # looks at the plane z = 0; no ray of the view lies in a coordinate plane (pc_cone refuses a pixel that touches one)
COUNTS = (63, 64, 65, 255, 256, 257)
COUNT_SIZE = (96, 64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def camera(desc, W, H, spp=64, shift=(0.0, 0.0, 0.0)):
    p = tuple(float(a) + float(b) for a, b in zip(desc["position"], shift))
    return va.make_camera(p, desc["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))


def _soup():
    g = np.load(os.path.join(HERE, "golden", "ref_soup_duplicates.npz"))
    return (g["pos"].reshape(-1, 9), g["nrm"].reshape(-1, 9), None), dict(position=tuple(g["cam"][:3]), rotation_deg=tuple(g["cam"][3:6]))


BACKDROP = np.array([[-200.0, -200.0, 0.0, 200.0, -200.0, 0.0, 0.0, 200.0, 0.0]], np.float32)


def _flat(pos):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    nrm = np.tile(np.array([0, 0, 1] * 3, np.float32), (pos.shape[0], 1))
    return pos, nrm, None


def _full():
    """one triangle that fills the view: every pixel has a claim"""
    return _flat(BACKDROP), FRONT


_cells = {}


def device_tree(pos, nrm, uv):
    with va.Scene(pos, nrm, uv, device=0) as sc:
        return sc.bvh()


def unclaimed_count(scene, tree_of):
    pos, nrm, uv = scene
    W, H = COUNT_SIZE
    return int(np.sum(LS.host_lists(pos, tree_of(pos, nrm, uv), [camera(FRONT, W, H)])[0][0] == NONE))


def speck_cells(tree_of):
    """Candidate specks for the COUNT_SIZE frame: small triangles half-way between the camera and the backdrop, one per
    4 x 4 block of pixels, on the central ray of the block's pixel (2, 2).  Returns (their triangles [k, 9], the number
    of pixels of its block that the host program leaves without a claim when all of them are in the scene [k]): a
    speck lies inside the widened cones of one to three pixels of its own block and of no other block's."""
    if not _cells:
        W, H = COUNT_SIZE
        cam = camera(FRONT, W, H)
        cells = [(y, x) for y in range(0, H, 4) for x in range(0, W, 4)]
        q = np.array([(y + 2) * W + x + 2 for y, x in cells], np.int64)
        d = S.footprint_directions(cam, q)[4].astype(np.float64)  # the footprint's centre
        o = np.array(FRONT["position"], np.float64)
        c = o + d * ((2.5 - o[2]) / d[:, 2])[:, None]
        e = 0.1 * (3.6 / W) * (2.5 / 6.0)  # a tenth of a pixel at that depth
        tri = np.concatenate([c + [-e, -e, 0.0], c + [e, -e, 0.0], c + [0.0, e, 0.0]], axis=1).astype(np.float32)
        pos, nrm, uv = _flat(np.concatenate([BACKDROP, tri]))
        claims = LS.host_lists(pos, tree_of(pos, nrm, uv), [cam])[0][0]
        per = np.array([int(np.sum(claims[y:y + 4, x:x + 4] == NONE)) for y, x in cells])
        _cells["tri"], _cells["per"] = tri, per
    return _cells["tri"], _cells["per"]


def _specks(n, tree_of=device_tree):
    """the backdrop and a subset of the candidate specks such that the host program leaves exactly n pixels of the
    COUNT_SIZE frame without a claim: a subset sum over the per-block counts, corrected by what the host program counts
    on the subset's own scene (the culled walk depends on the tree, so a block's count can move by one with its
    neighbours gone); every other pixel sees the backdrop alone and is claimed"""
    tri, per = speck_cells(tree_of)
    order = np.random.default_rng(1234).permutation(len(per))
    target = n
    for _ in range(8):
        reach = {0: []}  # sum -> indices
        for i in order:
            if target in reach:
                break
            for t, idx in list(reach.items()):
                if t + per[i] <= target and t + per[i] not in reach:
                    reach[t + per[i]] = idx + [int(i)]
        scene = _flat(np.concatenate([BACKDROP, tri[sorted(reach[target])]]))
        got = unclaimed_count(scene, tree_of)
        if got == n:
            return scene, FRONT
        target += n - got
    raise AssertionError("no speck scene with %d pixels without a claim" % n)


SCENES = {
    "cornell8": lambda: (scenes.cornell8(), scenes.cornell_camera()),
    "sponza260k": lambda: (scenes.sponza260k(), scenes.sponza_camera()),
    "soup": _soup,
    "full": _full,
}
for _n in COUNTS:
    SCENES["specks%d" % _n] = (lambda n: lambda: _specks(n))(_n)


class Loaded:
    def __init__(self, name):
        (pos, nrm, uv), self.cam_desc = SCENES[name]()
        self.name, self.pos, self.nrm, self.uv = name, pos, nrm, uv
        self.gpu = va.Scene(pos, nrm, uv, device=0)
        self.tree = self.gpu.bvh()
        self._host, self._cpu, self._refs = {}, None, {}

    def host(self, W, H, shift=(0.0, 0.0, 0.0)):
        """the host program's (claims, lists) of a camera, computed once, shared and never written to"""
        key = (W, H, shift)
        if key not in self._host:
            c, l, _, _ = LS.host_lists(self.pos, self.tree, [camera(self.cam_desc, W, H, shift=shift)])[0]
            c.setflags(write=False), l.setflags(write=False)
            self._host[key] = (c, l)
        return self._host[key]

    def reference(self, W, H, spp):
        key = (W, H, spp)
        if key not in self._refs:
            if self._cpu is None:
                self._cpu = O.OracleScene(self.pos, self.nrm, self.uv)
            img, st = self._cpu.render(camera(self.cam_desc, W, H, spp), va.make_opts(seed=4, early_stop=False))
            img.setflags(write=False)
            self._refs[key] = (img, st)
        return self._refs[key]


_loaded = {}


@pytest.fixture(scope="module")
def load():
    def get(name):
        if name not in _loaded:
            _loaded[name] = Loaded(name)
        return _loaded[name]
    yield get
    for s in _loaded.values():
        s.gpu.close()
    _loaded.clear()


def check_tables(s, W, H, shift=(0.0, 0.0, 0.0), prefill=(0.37, 0.21, -0.4), **okw):
    """both planes and the count of the device for one camera against the host program's, over planes that another
    camera's call filled before"""
    opts = va.make_opts(seed=4, **okw)
    hc, hl = s.host(W, H, shift)
    rows = va.local_row_indices(H, opts.stripe_rows, opts.rank, opts.world)
    hc, hl = hc[rows], hl[rows]
    if prefill is not None:
        s.gpu.pixel_claim_lists(camera(s.cam_desc, W, H, shift=prefill), opts)
    cam = camera(s.cam_desc, W, H, shift=shift)
    claims, lists, n = s.gpu.pixel_claim_lists(cam, opts)
    assert claims.shape == hc.shape and lists.shape == hl.shape
    assert np.array_equal(claims, hc), "claims differ from the host program's"
    assert np.array_equal(lists, hl), "list records differ from the host program's"
    assert n == int(np.sum(hc != NONE)), "the number of claimed pixels"
    assert np.all(lists[claims != NONE] == NONE), "a claimed pixel's record is not the empty one"
    only, n0 = s.gpu.pixel_claims(cam, opts)  # the launch that builds no lists
    assert np.array_equal(only, hc) and n0 == n
    return hc, hl


TABLE_CASES = [("cornell8", 8, 8), ("cornell8", 1, 1), ("cornell8", 37, 19), ("cornell8", 96, 64), ("cornell8", 160, 90),
               ("sponza260k", 160, 90), ("sponza260k", 37, 19), ("soup", 96, 64), ("soup", 37, 19), ("full", 37, 19), ("full", 96, 64)]


@pytest.mark.parametrize("name,W,H", TABLE_CASES, ids=["%s-%dx%d" % c for c in TABLE_CASES])
def test_tables_are_the_host_programs(load, name, W, H):
    s = load(name)
    hc, hl = check_tables(s, W, H)
    un = int(np.sum(hc == NONE))
    print("%s %dx%d: %d of %d pixels without a claim, %d with a list" % (name, W, H, un, hc.size, int(np.sum(LS.list_lengths(hl) > 0))))
    if name == "full":
        assert un == 0  # no entry for the list kernel
    if name == "soup" and hc.size > 64:
        assert un > 0.9 * np.sum(hc != S.MISS)  # almost every pixel that sees the soup


@pytest.mark.parametrize("n", COUNTS)
def test_counts_around_one_and_four_waves(load, n):
    s = load("specks%d" % n)
    W, H = COUNT_SIZE
    hc, _ = s.host(W, H)
    assert int(np.sum(hc == NONE)) == n, "the input: the host program leaves exactly n pixels without a claim"
    # (the first call's camera sees the specks in other pixels)
    check_tables(s, W, H, prefill=(0.05, 0.03, 0.0))


@pytest.mark.parametrize("name,W,H,stripe", [("cornell8", 96, 64, 5), ("sponza260k", 160, 90, 16), ("soup", 37, 19, 3)])
def test_stripes(load, name, W, H, stripe):
    s = load(name)
    some_partial = False
    for world in (2, 3):
        for rank in range(world):
            rows = va.local_row_indices(H, stripe, rank, world)
            some_partial |= len(rows) % 8 != 0
            check_tables(s, W, H, world=world, rank=rank, stripe_rows=stripe)
    assert some_partial  # local rows that end inside a tile


def test_a_smaller_frame_after_a_larger_one(load):
    s = load("sponza260k")
    a = (0.0, 0.0, 0.0)
    b = (0.6, -0.1, 0.3)
    check_tables(s, 160, 90, shift=a, prefill=None)
    check_tables(s, 37, 19, shift=b, prefill=None)   # fewer tiles, fewer entries: nothing of the first call is left
    check_tables(s, 160, 90, shift=b, prefill=None)
    check_tables(s, 8, 8, shift=a, prefill=None)
    hc, _ = s.host(160, 90, a)
    hd, _ = s.host(160, 90, b)
    assert not np.array_equal(hc, hd)  # each camera has its own table


FRAMES = [("cornell8", 96, 64), ("sponza260k", 160, 90)]
FORMS = (0x100, 4 | 0x100, 4, 0)  # the bench's form; the split passes: plain one-phase (fused claimed pixels), sorted rays; the default routing


@pytest.mark.parametrize("name,W,H", FRAMES, ids=[f[0] for f in FRAMES])
def test_frames_equal_the_oracles_and_the_frames_without_lists(load, name, W, H):
    s = load(name)
    cam = camera(s.cam_desc, W, H, 64)
    ref, rst = s.reference(W, H, 64)
    for form in FORMS:
        out = []
        for off in (0, NO_LISTS, NO_FUSE):
            img, st = s.gpu.render(cam, va.make_opts(seed=4, early_stop=False, pipeline=form | off))
            out.append((img, st, s.gpu.timings()["other"]["launches"], s.gpu.list_settled_rays()))
        (a, sa, la, na), (b, sb, lb, nb), (c, sc_, lc, nc) = out
        assert np.array_equal(bits(a), bits(ref)), (hex(form), "frame differs from the oracle's")
        assert np.array_equal(bits(a), bits(b)), (hex(form), "lists on / off differ")
        assert np.array_equal(bits(a), bits(c)), (hex(form), "fused / three-kernel route differ")
        for k in COUNT_KEYS:
            assert sa[k] == sb[k] == sc_[k], (hex(form), k)
        assert sa["samples"] == rst["samples"]
        assert la == lb == lc, (hex(form), la, lb, lc)
        assert la == (1 if form & 4 else 0), (hex(form), la)  # one timed interval per call that builds claims
        assert nb == 0 and na == nc, (hex(form), na, nb, nc)  # the tally follows the rule, not the route
        if form & 4:
            assert 0 < na < sa["rays_primary"], hex(form)
        print("form %s: %d of %d camera rays settled by a list" % (hex(form), na, sa["rays_primary"]))
