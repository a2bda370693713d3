"""The persistent kernels' work loops at test sizes: every case creates its scene under VMX_CU_LIMIT (a scene that counts
1 or 3 compute units launches the grids of such a device), asserts that the limit took hold (Scene.compute_units) and that
the launch is loaded -- items >= 4 * 64 * 32 * compute_units: a compute unit holds at most 32 waves of 64 lanes, so the
launch's waves take four reservations each on average -- and compares the entry bit for bit with the reference the entry's
own test uses: tests/nee_spec.py, tests/budget_spec.py, the oracle, the host program of the claim tables.  Equality with a
scene created without the limit is a second check, never the only one.

What the small frames of the other files never run, and these do: a wave's second and later trips through its work loop
(a lane refilled next to lanes in mid-walk, the tile loop of k_pixel_claims, the chunk loop of k_pixel_lists), reservations
of 128 and 256 items, the block-stride loops behind the launch routines' grid bounds, and buffers sized from the grid
(the overflow slab, the record lists' padding, the guide's fallback grid).

Every test prints `load: <what> items=.. compute_units=.. reservations_per_wave=..` (items / (64 * 32 * compute_units))."""
import functools

import numpy as np
import pytest

import budget_spec as BS
import claim_list_spec as LS
import nee_cases as K
import nee_spec as N
import oracle_lib as O
import test_gpu_claim_walks as CW
import test_gpu_nee as TN
import test_gpu_nee_progressive as TP
import test_gpu_query as TQ
import test_gpu_raycast as TR
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
F = np.float32
NONE = LS.NONE
NO_LISTS, NO_FUSE, NO_GUIDE = 0x2000, 0x1000, 0x4000


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what):
    diff = bits(np.asarray(got, F)) != bits(np.asarray(want, F))
    assert not diff.any(), "%s: %d of %d values differ, first at %s" % (what, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())


def limited(monkeypatch, limit, make):
    """make() under VMX_CU_LIMIT = limit: the variable is read when a scene is created, and only then"""
    monkeypatch.setenv("VMX_CU_LIMIT", str(limit))
    made = make()
    monkeypatch.delenv("VMX_CU_LIMIT")
    sc = getattr(made, "gpu", made)
    assert sc.compute_units == limit, "VMX_CU_LIMIT was ignored: the scene counts %d compute units" % sc.compute_units
    return made


def loaded(sc, items, what):
    """the load condition, from the scene's own count"""
    cus = sc.compute_units
    print("load: %s items=%d compute_units=%d reservations_per_wave=%.1f" % (what, items, cus, items / (64.0 * 32 * cus)))
    assert items >= 4 * 64 * 32 * cus, (what, items, cus)


def device_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the variable itself ------------------------------------------------------------------------------------------------------
def test_the_limit_only_lowers_the_count(monkeypatch):
    pos, nrm, uv = scenes.cornell8()
    own = device_units()
    assert own > 3
    for value, want in ((None, own), ("", own), ("0", own), ("100000", own), (str(own), own), ("abc", own), ("3x", own), ("-1", own),
                        ("1", 1), ("3", 3), (str(own - 1), own - 1)):
        if value is None:
            monkeypatch.delenv("VMX_CU_LIMIT", raising=False)
        else:
            monkeypatch.setenv("VMX_CU_LIMIT", value)
        with va.Scene(pos, nrm, uv) as sc:
            monkeypatch.setenv("VMX_CU_LIMIT", "2")  # read at creation only
            assert sc.compute_units == want, (value, sc.compute_units)
    assert L.load().vmx_scene_compute_units(None) == 0


# ---- k_nee, work source 0: frames ---------------------------------------------------------------------------------------------
# (scene, table, texture channels, W, H, spp, limit): cornell8 48 x 32 x 8 is test_gpu_nee's frame (12,288 paths); the lattice's
# 40 x 24 x 4 has 3,840 and is rendered at 64 x 32 x 4 = 8,192; limit 3 needs 24,576 = 48 x 32 x 16.  47 x 33 has 1,551
# pixels: the launch's items are the 1,600 padded slots' samples (always a multiple of 64), and the items of the last 49
# slots, which lie inside the last reservations, are no paths.
NEE_FRAMES = [("cornell8", "default", 0, 48, 32, 8, 1), ("lattice", "default", 0, 64, 32, 4, 1), ("cornell8", "overlap", 0, 48, 32, 8, 1),
              ("cornell8", "single", 3, 48, 32, 8, 1), ("cornell8", "default", 0, 48, 32, 16, 3), ("cornell8", "default", 0, 47, 33, 8, 1)]


@pytest.mark.parametrize("scene,table,channels,W,H,spp,limit", NEE_FRAMES)
def test_render_nee_under_the_limit(monkeypatch, scene, table, channels, W, H, spp, limit):
    want, wst = TN.spec_frame(scene, table, channels, W, H, spp, 5)
    cam, opts = TN.camera(scene, W, H, spp), K.opts(5)
    with limited(monkeypatch, limit, lambda: TN.device_scene(scene, table, channels)) as sc:
        loaded(sc, W * H * spp, "render_nee %s %s" % (scene, table))
        got, st = sc.render_nee(cam, opts)
        # two stack levels in LDS: the deeper ones of every walk in the overflow slab, a row of it per wave of the grid
        spilled, sst = sc.render_nee(cam, K.opts(5, lds_entries=2))
    same(got, want, "frame against nee_spec")
    same(spilled, want, "frame against nee_spec, stacks in the overflow slab")
    assert sst["rays_secondary"] == wst["rays_secondary"]
    assert st["passes"] == 1  # one launch over all W * H * spp paths
    assert st["samples"] == wst["samples"] == W * H * spp
    assert st["rays_primary"] == wst["rays_primary"] and st["rays_secondary"] == wst["rays_secondary"]
    with TN.device_scene(scene, table, channels) as sc:
        free, fst = sc.render_nee(cam, opts)
    same(got, free, "frame against the unlimited scene's")
    assert all(st[k] == fst[k] for k in ("samples", "rays_primary", "rays_secondary", "passes"))


# ---- k_nee, work source 1: explicit rays --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shuffled_rays(repeats):
    """the golden camera rays of both scenes, `repeats` times over, in a fixed shuffled order: a ray stands at several
    indices, and ray i runs on stream (seed, i, 0), so each of its copies is another path"""
    o = np.concatenate([K.golden(s)[3] for s in ("cornell8", "lattice")] * repeats)
    d = np.concatenate([K.golden(s)[4] for s in ("cornell8", "lattice")] * repeats)
    p = np.random.default_rng(2024).permutation(len(o))[:-27]  # a count that is no multiple of 64: the last reservation is clipped
    o, d = np.ascontiguousarray(o[p]), np.ascontiguousarray(d[p])
    o.setflags(write=False), d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def spec_shuffled(repeats, table, scene="cornell8"):
    pos, nrm, uv, _, _, _ = K.golden(scene)
    o, d = shuffled_rays(repeats)
    tb = K.table(table)
    osc = O.OracleScene(pos, nrm, uv, spheres=tb)
    out, st = N.radiance(osc, o, d, 7, tb, K.CORRECTED, True)
    osc.close()
    out.setflags(write=False)
    return out, st


# 2,496 golden rays: 9,957 and 24,933 paths; the lattice's tree is 7 deep, so with two stack levels in LDS its walks use the
# overflow slab
@pytest.mark.parametrize("scene,limit,repeats,lds", [("cornell8", 1, 4, 0), ("cornell8", 3, 10, 0), ("lattice", 1, 4, 2)])
def test_radiance_nee_under_the_limit(monkeypatch, scene, limit, repeats, lds):
    o, d = shuffled_rays(repeats)
    want, wst = spec_shuffled(repeats, "default", scene)
    with limited(monkeypatch, limit, lambda: TN.device_scene(scene, "default", 0)) as sc:
        loaded(sc, len(o), "radiance_nee %s" % scene)
        got, st = sc.radiance_nee(o, d, K.opts(7, lds_entries=lds))
    same(got, want, "radiance against nee_spec")
    assert len(o) % 64 != 0
    assert st["rays_primary"] == wst["rays_primary"] == len(o) and st["samples"] == len(o)
    assert st["rays_secondary"] == wst["rays_secondary"]
    # the copies of one ray are different paths: the index is part of the stream's key
    first = np.unique(np.concatenate([o, d], axis=1), axis=0, return_inverse=True)[1].reshape(-1)
    copies = np.flatnonzero(first == first[0])
    assert len(copies) >= repeats and len(np.unique(bits(want[copies]), axis=0)) > 1
    with TN.device_scene(scene, "default", 0) as sc:
        free, fst = sc.radiance_nee(o, d, K.opts(7))
    same(got, free, "radiance against the unlimited scene's")
    assert fst["rays_secondary"] == st["rays_secondary"]


# ---- k_nee with reservations of 128 and 256 items -----------------------------------------------------------------------------
RESERVE_TABLE = "single"


@functools.lru_cache(maxsize=None)
def reserve_rays(n):
    """n rays for the cornell8 scene under the table `single`.  Every 16th is a golden camera ray (a whole path).  The others
    are one-cast paths: from behind the camera toward the emitter, which they hit first, so the path ends at its first hit
    (length(hitColour) > 1) and its row is (the emitter's colour, the hit distance).  Ray i starts (i % 1024) / 4 units
    further back, so the distance differs between any two rays less than 1,024 apart."""
    pos, nrm, uv, go, gd, _ = K.golden("cornell8")
    c = np.float64([300.0, 600.0, 200.0])  # the emitter, radius 60 (nee_cases.table)
    i = np.arange(n)
    org = np.float64(scenes.cornell_camera()["position"])[None, :] + np.stack([np.zeros(n), np.zeros(n), (i % 1024) * 0.25], axis=1)
    # distinct points of a patch in the middle of the disc the emitter shows the camera
    a = (i // 1024) * 0.61803398875 * 2 * np.pi
    r = 12.0 * np.sqrt(((i // 1024) % 512 + 0.5) / 512.0)
    tgt = c[None, :] + np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], axis=1)
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = org.astype(F), d.astype(F)
    gi = np.arange(0, n, 16)
    o[gi], d[gi] = go[(gi // 16) % len(go)], gd[(gi // 16) % len(go)]
    o.setflags(write=False), d.setflags(write=False)
    return o, d, gi


@functools.lru_cache(maxsize=None)
def spec_reserve(n):
    """nee_spec.radiance of reserve_rays(n): the golden rays through the spec itself, on their own streams (seed, i, 0); the
    one-cast rays by the oracle's RayCast and the spec's first step, which is all a path takes that hits an emitter first:
    accumColour = 0 + 1 * hitColour, .w = the distance, no draw, no further ray (nee_spec.radiance steps 1 to 3).  That every
    such ray does hit the emitter first is asserted here; that the short cut is the spec's own answer is asserted on the
    first 4,096 rays by the test.  (The spec draws a stream per path in Python: for 524,288 paths that alone is more than
    the test may take.)"""
    pos, nrm, uv, _, _, _ = K.golden("cornell8")
    o, d, gi = reserve_rays(n)
    tb = K.table(RESERVE_TABLE)
    osc = O.OracleScene(pos, nrm, uv, spheres=tb)
    out = np.empty((n, 4), F)
    h = osc.raycast(o, d)
    col = h["colour"].astype(F)
    one = np.ones(n, bool)
    one[gi] = False
    assert ((h["flags"][one] & 1) != 0).all() and (np.sqrt(N._dot(col[one], col[one])) > F(1)).all(), "a one-cast ray misses the emitter"
    out[:, :3] = F(0) + F(1) * col
    out[:, 3] = h["distance"]
    out[gi], st = N.radiance(osc, o[gi], d[gi], 7, tb, K.CORRECTED, True, None, gi.astype(np.int64), np.zeros(len(gi), np.int64))
    head, hst = N.radiance(osc, o[:4096], d[:4096], 7, tb, K.CORRECTED, True)
    osc.close()
    st = dict(st, rays_primary=n, samples=n)
    out.setflags(write=False)
    return out, st, head


RESERVE_RAYS = 256 * 8 * 256 + 37  # 524,325: 256 items per lane on a grid of 8 blocks, and no multiple of any reservation
# bind_stack reserves 64, 128 or 256 items per atomic by items / (grid * 256) < 64, < 256 or more.  The grid is the kernel's
# occupancy, 1 to 8 blocks of 256 threads per compute unit, which no entry reports: with 100 * 256 * b + 37 rays for every
# b from 1 to 8, the run whose b is the occupancy has 100 items per lane, so one of them is sure to reserve 128; the others
# reserve 64, 128 or 256.  524,325 rays reserve 256 at any occupancy.  Every count is ragged against every reservation.
RESERVE_COUNTS = [100 * 256 * b + 37 for b in range(1, 9)] + [RESERVE_RAYS]


def test_radiance_nee_with_wide_reservations(monkeypatch):
    """reservations of 128 and 256 items, the last one clipped by the number of rays (RESERVE_COUNTS).  Ray i runs on stream
    (seed, i, 0) whatever the count, so the answer for n rays is the first n rows of the answer for all of them.  The
    reference is nee_spec's, with the one-cast rays taken through the oracle's RayCast and the spec's first step
    (spec_reserve says why and checks it)."""
    o, d, gi = reserve_rays(RESERVE_RAYS)
    want, wst, head = spec_reserve(RESERVE_RAYS)
    same(want[:4096], head, "the one-cast short cut against nee_spec.radiance itself")
    for s in (64, 128, 256):  # a reservation handed to the wrong lanes, or twice, must show: no two rows that far apart are equal
        assert not (bits(want[s:]) == bits(want[:-s])).all(axis=1).any(), s
    with limited(monkeypatch, 1, lambda: TN.device_scene("cornell8", RESERVE_TABLE, 0)) as sc:
        cus = sc.compute_units
        for n in RESERVE_COUNTS:
            loaded(sc, n, "radiance_nee reserve sweep")
            assert all(n % r for r in (64, 128, 256))
            got, st = sc.radiance_nee(o[:n], d[:n], K.opts(7))
            same(got, want[:n], "radiance of %d rays against nee_spec" % n)
            assert st["rays_primary"] == n and st["samples"] == n, n
        assert [64 <= RESERVE_COUNTS[b - 1] // (b * cus * 256) < 256 for b in range(1, 9)] == [True] * 8
        assert RESERVE_RAYS // (8 * cus * 256) >= 256
        assert st["rays_secondary"] == wst["rays_secondary"]


# ---- k_nee, work source 2: budgeted steps -------------------------------------------------------------------------------------
def budget_plane(counts, kmax, B):
    """budgets 0, 1, the cap, past the cap and values between, scattered over the image"""
    r = np.random.RandomState(11)
    b = r.choice([0, 1, 5, 7, 8, 8, 9, 1000], counts.shape).astype(np.int64)
    if BS.step_counts(counts, b, kmax, B).sum() % 64 == 0:
        b[0, 0] = 1 if b[0, 0] != 1 else 2
    return b


def test_budgeted_steps_under_the_limit(monkeypatch):
    """test_step_budget_with_a_hand_made_plane at 48 x 32 x 16: ragged cursors (3 and 7 samples), then one budgeted step of
    more than 8,192 items, then steps to completion"""
    W, H, kmax, B = 48, 32, 16, 8
    sp = TP.spec("cornell8", "default", 0, W, H, 16)
    opts = K.opts(TP.SEED, samples_per_batch=B)
    yy, xx = np.mgrid[0:H, 0:W]
    with limited(monkeypatch, 1, lambda: TP.device_scene("cornell8", "default", 0)) as sc, sc.progressive_nee(sp.cam, opts, moments=True) as p:
        p.step(3)
        p.step_selected(4, TP.dev(((xx + yy) % 3 == 0).astype(np.uint8)))
        sums0, n0 = TP.state(p)
        assert set(np.unique(n0)) == {3, 7}
        same(sums0, sp.sums(n0), "the ragged state")
        got_b, total = TP.budgets_of(p)
        want_b = BS.budget(sums0, n0, kmax, B)
        assert np.array_equal(got_b, want_b) and total == int(want_b.sum(dtype=np.int64))
        b = budget_plane(n0, kmax, B)
        want_sums, want_n, take = BS.step(sums0, n0, b, kmax, B, sp.samples)
        assert take.min() == 0 and take.max() == B and set(np.unique(take)) >= {0, 1, 5, 7, 8} and take.sum() % 64 != 0
        loaded(sc, int(take.sum()), "step_budget")
        st, nsel = p.step_budget(TP.dev(b.astype(np.int32)))
        sums, n = TP.state(p)
        assert np.array_equal(n, want_n) and np.array_equal(n, n0 + take)
        same(sums, want_sums, "sums and m2 against budget_spec.step")
        same(sums, sp.sums(n), "sums and m2, from the first sample on")
        same(sums[b == 0], sums0[b == 0], "pixels with budget 0")
        wst = sp.paths(n0, take)
        assert st["samples"] == int(take.sum()) == wst["samples"] and nsel == int((take > 0).sum())
        assert st["rays_primary"] == wst["rays_primary"] and st["rays_secondary"] == wst["rays_secondary"]
        assert st["passes"] == 1
        same(p.preview(), sp.frame(n), "preview")
        left = int((kmax - n).sum())
        fst = p.step(0)
        assert fst["samples"] == left and p.info()["pixels_active"] == 0
        same(p.preview(), sp.frame(kmax), "complete")
        same(p.preview(), TN.spec_frame("cornell8", "default", 0, W, H, 16, TP.SEED)[0], "complete, against nee_spec.frame")


# ---- k_pixel_claims, the live-list scan and scatter, k_pixel_lists ---------------------------------------------------------------
_tables = {}


@pytest.fixture(scope="module")
def tables(request):
    """get(monkeypatch, name, limit): the scene `name` of test_gpu_claim_walks created under the limit (None: without one),
    its tree and its host tables; created once, closed with the module"""
    def get(monkeypatch, name, limit):
        if (name, limit) not in _tables:
            _tables[name, limit] = limited(monkeypatch, limit, lambda: CW.Loaded(name)) if limit else CW.Loaded(name)
        s = _tables[name, limit]
        assert s.gpu.compute_units == (limit if limit else device_units())
        return s
    yield get
    for s in _tables.values():
        s.gpu.close()
    _tables.clear()


# 96 x 64 has 96 tiles, 6,144 lanes of the claim kernel: 128 x 64 is the smallest frame of whole tiles with 8,192.  (Limit 1
# only: at 3 the condition asks for 24,576 lanes, and the largest frame, 160 x 90, has 15,360.)
TABLE_CASES = [("cornell8", 128, 64, 1), ("cornell8", 160, 90, 1), ("sponza260k", 160, 90, 1), ("soup", 128, 64, 1), ("full", 128, 64, 1)]


def check_loaded_tables(s, W, H, **okw):
    opts = va.make_opts(seed=4, **okw)
    rows = len(va.local_row_indices(H, opts.stripe_rows, opts.rank, opts.world))
    loaded(s.gpu, ((W + 7) // 8) * ((rows + 7) // 8) * 64, "pixel_claim_lists %s %dx%d" % (s.name, W, rows))
    hc, hl = CW.check_tables(s, W, H, **okw)
    un = int(np.sum(hc == NONE))
    print("load: k_pixel_lists %s entries=%d chunks_of_64=%d" % (s.name, un, (un + 63) // 64))
    return hc, hl, un


@pytest.mark.parametrize("name,W,H,limit", TABLE_CASES, ids=["%s-%dx%d-%d" % c for c in TABLE_CASES])
def test_claim_tables_under_the_limit(monkeypatch, tables, name, W, H, limit):
    s = tables(monkeypatch, name, limit)
    hc, hl, un = check_loaded_tables(s, W, H)
    if name in ("soup", "sponza260k"):
        assert un >= 512, "fewer than 8 chunks of 64 entries for the list kernel"
    if name == "full":
        assert un == 0


def test_claim_tables_of_a_stripe_under_the_limit(monkeypatch, tables):
    """rank 0 of 2 with stripes of 37 rows: 53 local rows, which end inside a tile"""
    s = tables(monkeypatch, "sponza260k", 1)
    rows = va.local_row_indices(90, 37, 0, 2)
    assert len(rows) == 53
    hc, hl, un = check_loaded_tables(s, 160, 90, world=2, rank=0, stripe_rows=37)
    assert un >= 512


# ---- the camera and bounce kernels of vmx_render --------------------------------------------------------------------------------
RENDER_SCENES = [("cornell8", 96, 64, 1), ("sponza260k", 160, 90, 1), ("cornell8", 96, 64, 3)]
RENDER_FORMS = (0x100, 4 | 0x100, 4, 4 | 0x200, 0)
COUNT_KEYS = ("rays_primary", "rays_secondary", "samples", "samples_discarded", "passes")
STAGE_KEYS = ("rays", "tri_hits", "continued")


_oracle = {}


def oracle_frame(s, W, H, spp, early_stop):
    """the oracle's frame and counts of the loaded scene s, rendered once and not written to"""
    key = (s.name, W, H, spp, early_stop)
    if key not in _oracle:
        osc = O.OracleScene(s.pos, s.nrm, s.uv)
        img, st = osc.render(CW.camera(s.cam_desc, W, H, spp), va.make_opts(seed=4, early_stop=early_stop))
        osc.close()
        img.setflags(write=False)
        _oracle[key] = (img, st)
    return _oracle[key]


def check_counts(st, rst, tag):
    assert st["samples"] == rst["samples"], tag
    if st["samples_discarded"] == 0:
        assert st["rays_primary"] == rst["rays_primary"] and st["rays_secondary"] == rst["rays_secondary"], tag
        assert st["primary"]["tri_hits"] + st["bounce"]["tri_hits"] == rst["primary"]["tri_hits"], tag
        assert st["primary"]["continued"] + st["bounce"]["continued"] == rst["primary"]["continued"], tag
    else:  # speculative samples that an early stop discarded were traced too
        assert st["rays_primary"] == rst["rays_primary"] + st["samples_discarded"], tag


@pytest.mark.parametrize("form", RENDER_FORMS, ids=[hex(f) for f in RENDER_FORMS])
@pytest.mark.parametrize("name,W,H,limit", RENDER_SCENES, ids=["%s-%d" % (s[0], s[3]) for s in RENDER_SCENES])
def test_frames_under_the_limit(monkeypatch, tables, name, W, H, limit, form):
    """the frames of test_gpu_claim_walks (64 samples: claims and lists are built), every pipeline form with lists on, lists
    off and the three-kernel route, form 4 with the early stop too: the oracle's frame and counts"""
    s = tables(monkeypatch, name, limit)
    free = tables(monkeypatch, name, None)
    cam = CW.camera(s.cam_desc, W, H, 64)
    loaded(s.gpu, W * H * 64, "render %s form %s" % (name, hex(form)))
    for early_stop in ((False, True) if form == 4 else (False,)):
        ref, rst = oracle_frame(s, W, H, 64, early_stop)
        for off in (0, NO_LISTS, NO_FUSE):
            tag = (name, hex(form | off), early_stop)
            opts = va.make_opts(seed=4, early_stop=early_stop, pipeline=form | off)
            img, st = s.gpu.render(cam, opts)
            assert np.array_equal(bits(img), bits(ref)), (tag, "frame differs from the oracle's")
            check_counts(st, rst, tag)
            settled = s.gpu.list_settled_rays()
            fimg, fst = free.gpu.render(cam, opts)
            assert np.array_equal(bits(img), bits(fimg)), (tag, "frame differs from the unlimited scene's")
            for k in COUNT_KEYS:
                assert st[k] == fst[k], (tag, k)
            for stage in ("primary", "bounce"):
                for k in STAGE_KEYS:
                    assert st[stage][k] == fst[stage][k], (tag, stage, k)
            assert settled == free.gpu.list_settled_rays(), tag
    if form == 4:  # VMX_SAMPLING_ELIDE_DEAD: k_raygen<1>, the live list's scan and scatter, k_raygen_live; the same frame
        ref, rst = oracle_frame(s, W, H, 64, False)
        opts = va.make_opts(seed=4, early_stop=False, sampling=va.VMX_SAMPLING_PARITY | va.VMX_SAMPLING_ELIDE_DEAD, pipeline=form)
        img, st = s.gpu.render(cam, opts)
        assert np.array_equal(bits(img), bits(ref)), (name, "the elided frame differs from the oracle's")
        assert st["samples"] == rst["samples"] and 0 < st["rays_primary"] < rst["rays_primary"]
        fimg, fst = free.gpu.render(cam, opts)
        assert np.array_equal(bits(img), bits(fimg))
        for k in COUNT_KEYS:
            assert st[k] == fst[k], (name, "elided", k)


# ---- vmx_radiance: k_radiance_init_ids and the bounce generations of explicit rays ------------------------------------------------
@pytest.mark.parametrize("form", [{}, {"pipeline": 4, "tail_threshold": 1}], ids=["default", "split-notail"])
def test_radiance_under_the_limit(monkeypatch, form):
    """test_radiance_paths_bit_exact over the 9,957 shuffled golden rays: k_radiance_init_ids strides over them on 16 blocks;
    with tail_threshold = 1 every generation runs k_trace_w<1> + k_shade<1>, else the fused tail takes them"""
    pos, nrm, uv, _, _, _ = K.golden("cornell8")
    o, d = shuffled_rays(4)
    opts = va.make_opts(seed=5, **form)
    osc = O.OracleScene(pos, nrm, uv)
    want, wst = osc.radiance(o, d, opts)
    osc.close()
    with limited(monkeypatch, 1, lambda: va.Scene(pos, nrm, uv)) as sc:
        loaded(sc, len(o), "radiance")
        got, st = sc.radiance(o, d, opts)
    same(got, want, "radiance against the oracle")
    assert st["rays_primary"] == wst["rays_primary"] == len(o) and st["rays_secondary"] == wst["rays_secondary"]
    assert wst["rays_secondary"] > 0


# ---- the guide walks and their fallback launch ----------------------------------------------------------------------------------
GUIDE_FORMS = (4, 4 | 0x100, 4 | 0x200)


@pytest.mark.parametrize("split", [True, False], ids=["split", "tail"])
@pytest.mark.parametrize("name", ["cornell8", "soup"])
def test_guided_frames_under_the_limit(monkeypatch, tables, name, split):
    """test_gpu_guide (tail_threshold = 1: every bounce generation in k_trace_w<1, .., GUIDE> and, for the rays the rule does
    not settle, the fallback launch -- most rays of the soup) and test_gpu_guide_fused (the default threshold: k_paths' GUIDE
    forms), 96 x 64 x 64: the oracle's frame, and the guide's counters of the unlimited scene"""
    W, H = 96, 64
    s = tables(monkeypatch, name, 1)
    free = tables(monkeypatch, name, None)
    cam = CW.camera(s.cam_desc, W, H, 64)
    ref, rst = oracle_frame(s, W, H, 64, False)
    loaded(s.gpu, W * H * 64, "guided render %s" % name)
    kw = dict(tail_threshold=1) if split else {}
    for form in GUIDE_FORMS:
        for off in (0, NO_GUIDE):
            tag = (name, hex(form | off), split)
            opts = va.make_opts(seed=4, early_stop=False, pipeline=form | off, **kw)
            out = []
            for sc in (s.gpu, free.gpu):
                img, st = sc.render(cam, opts)
                out.append((img, st, sc.guide_rays(), sc.guide_fused_rays(), sc.guide_list_entries()))
            (img, st, rays, fused, handed), (fimg, fst, frays, ffused, fhanded) = out
            assert np.array_equal(bits(img), bits(ref)), (tag, "frame differs from the oracle's")
            check_counts(st, rst, tag)
            assert np.array_equal(bits(img), bits(fimg)), tag
            for k in COUNT_KEYS:
                assert st[k] == fst[k], (tag, k)
            assert (rays, fused, handed) == (frays, ffused, fhanded), tag
            if off:
                assert rays == (0, 0) and fused == (0, 0) and handed == 0, tag
            elif split:
                assert sum(rays) == handed > 0, tag
                if name == "soup":
                    assert rays[1] > 0, tag  # the fallback launch had work
            else:
                assert sum(fused) > 0, tag


# ---- the query kernels, RayCast, k_trace, k_bruteforce -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,limit", [("cornell8", 1), ("sponza260k", 1), ("cornell8", 3)])
def test_queries_and_raycasts_under_the_limit(monkeypatch, name, limit):
    """test_gpu_query's and test_gpu_raycast's batches (60,000 rays) against the oracle: vmx_trace, every query mode through
    the host and the device entry with both fetch forms, RayCast's records"""
    gen, _ = scenes.SCENES[name]
    pos, nrm, uv = gen()
    o, d = TR.cornell_rays(60000, 31) if name == "cornell8" else TQ.rand_rays(60000, 11)
    osc = O.OracleScene(pos, nrm, uv)
    otri, ot = osc.trace(o, d)
    orec = osc.raycast(o, d)
    osc.close()
    assert (otri >= 0).any() and (otri < 0).any()
    with limited(monkeypatch, limit, lambda: va.Scene(pos, nrm, uv)) as sc:
        loaded(sc, len(o), "query / raycast %s" % name)
        tri, t = sc.trace(o, d)
        assert np.array_equal(tri, otri) and np.array_equal(bits(t), bits(ot)), "vmx_trace"
        TQ.check_all_modes(sc, o, d, ref=(otri, ot), tag=name)
        r = np.random.RandomState(5)
        tmax = np.where(r.rand(len(o)) < 0.5, ot, r.uniform(1, 2500, len(o))).astype(F)  # (test_nearest_on_other_trees' bounds)
        TQ.check_all_modes(sc, o, d, tmax, ref=(otri, ot), tag=(name, "bounded"))
        for per_lane in (False, True):
            dtri, dt, dhit = sc.query(TQ.dev(o), TQ.dev(d), per_lane_fetch=per_lane)
            assert np.array_equal(dtri.cpu().numpy(), otri) and np.array_equal(bits(dt.cpu().numpy()), bits(ot)), per_lane
            assert np.array_equal(dhit.cpu().numpy(), otri >= 0), per_lane
        host = TR.check_both_fetches(sc, o, d, tag=name)
        TR.check(host, orec, name, pad=False)


def test_bruteforce_under_the_limit(monkeypatch):
    """one lane per pixel: 128 x 64 is the smallest frame of test_gpu_bruteforce's kind with 8,192 of them"""
    pos, nrm, uv = scenes.cornell8()
    cc = scenes.cornell_camera()
    W, H, spp = 128, 64, 16
    cam = va.make_camera(cc["position"], cc["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))
    osc = O.OracleScene(pos, nrm, uv)
    with limited(monkeypatch, 1, lambda: va.Scene(pos, nrm, uv)) as sc, va.Scene(pos, nrm, uv) as free:
        loaded(sc, W * H, "render_bruteforce")
        for flags in (0, L.VMX_BF_ABS_INT):
            opts = va.make_opts(seed=13)
            img, st = sc.render_bruteforce(cam, opts, flags)
            ref, rst = osc.render_bruteforce(cam, opts, flags)
            same(img, ref, "bruteforce frame, flags %d" % flags)
            assert st["samples"] == rst["samples"] and st["rays_primary"] == rst["rays_primary"] == st["samples"]
            assert st["rays_secondary"] == rst["rays_secondary"]
            fimg, fst = free.render_bruteforce(cam, opts, flags)
            same(img, fimg, "against the unlimited scene's")
            assert st["rays_secondary"] == fst["rays_secondary"]
    osc.close()
