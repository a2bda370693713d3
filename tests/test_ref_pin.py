"""The oracle against the reference's OWN compiled code (oracle/_ref/libvmx_ref.so: the reference's translation units,
unmodified, built by `make -C oracle ref` against the stand-in headers of oracle/ref_standin/).  CPU only.

Every comparison is bitwise (uint32 views; NaN == NaN, see nbad) on the parity build (-O2 -ffp-contract=off on both sides).  What this
pins is the reference's program text — control flow, operand order, comparisons, constants, the BVH build, the
traversal and its tie order, the sphere table, the draw order of Radiance, the texture lookup.  What it does not pin is
GLM's own arithmetic: the stand-in defines it to the readings of DESIGN_HISTORY.md §2, the same ones the oracle restates.

Out of reach of this file, by construction:
 * custom sphere tables: the reference's eight spheres are written into MeshEngine::RayCast, so every scene here
   uses the default table; `spheres=` of the oracle and the kernels is a project extension _ref cannot speak to;
 * vmx_rayhit.tri_id / tri_t: RayCast does not return the BVH hit on its own; those two fields are this project's
   additions to the record and are checked against BVH::getIntersection instead (test_get_intersection_*);
 * PathTracer::Render / BruteForceTracer::Render: seeded from random_device / time(0) inside their loops.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
import ref_lib as R
import vermilion_amd as va
from shared_inputs import (LIGHT1, LIGHT2, SOUP_KINDS, SOUP_SEEDS, SOUP_SIZES, light_rays, random_soup,
                           rays_inside_and_outside, special_rays, unit, wall_rays)
from vermilion_amd import scenes

if not R.available():
    pytest.skip("neither oracle/_ref/libvmx_ref.so nor a reference tree to build it from", allow_module_level=True)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BRANCH_FLOOR = 100


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def nbad(a, b):
    """number of elements (rows for 2-D input) with any differing bit.  One exception, the one same_f32 of the GPU tests
    makes: a NaN equals a NaN.  IEEE 754 leaves the sign and payload of a NaN result unspecified, and two compilations of
    the same expression differ in it (seen here: the normal of a zero-area triangle, 0/0 negated — 0x7fc00000 from one
    build, 0xffc00000 from the other); nothing downstream can tell them apart."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    x, y = bits(a), bits(b)
    assert x.shape == y.shape
    d = (x != y) & ~(np.isnan(a) & np.isnan(b))
    return int(d.reshape(d.shape[0], -1).any(axis=1).sum()) if d.ndim else int(d)


def assert_trees_equal(ref_tree, orc_tree, tag):
    for k in ("start", "nprims", "right_offset", "prim_order"):
        if k in ref_tree:
            assert np.array_equal(ref_tree[k], orc_tree[k]), (tag, k)
    assert ref_tree["bbox"].shape == orc_tree["bbox"].shape, tag
    assert nbad(ref_tree["bbox"], orc_tree["bbox"]) == 0, (tag, "bbox")


def assert_trace_equal(rs, os_, o, d, tag):
    rtri, rt = rs.trace(o, d)
    otri, ot = os_.trace(o, d)
    assert np.array_equal(rtri, otri), (tag, "ids", int((rtri != otri).sum()), len(o))
    assert nbad(rt, ot) == 0, (tag, "t", nbad(rt, ot), len(o))
    return otri, ot


def assert_raycast_equal(rs, os_, o, d, tag):
    """every field MeshEngine::RayCast returns; tri_id / tri_t are the project's additions and stay oracle-only"""
    a, b = rs.raycast(o, d), os_.raycast(o, d)
    for f in R.RAYHIT_REFERENCE_FIELDS:
        x, y = a[f], b[f]
        bad = nbad(x, y) if x.dtype == np.float32 else int((x != y).sum())
        assert bad == 0, (tag, f, bad, len(o))
    return b


SCENE_NAMES = ("cornell8", "lattice", "bunny70k", "sponza260k")


@pytest.fixture(scope="module", params=SCENE_NAMES)
def named_scene(request):
    gen, camf = scenes.SCENES[request.param]
    return request.param, gen(), camf


# ---- BVH::build -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [1, 2, 4, 7, 31])
def test_tree_bit_exact(named_scene, leaf):
    name, (pos, nrm, uv), _ = named_scene
    rs, os_ = R.RefScene(pos, nrm, uv, leaf_size=leaf), O.OracleScene(pos, nrm, uv, leaf_size=leaf)
    rt, ot = rs.bvh(), os_.bvh()
    assert rs.describe()["n_nodes"] == os_.describe()["n_nodes"] and rs.describe()["n_leaves"] == os_.describe()["n_leaves"]
    assert_trees_equal(rt, ot, (name, leaf))
    assert sorted(rt["prim_order"].tolist()) == list(range(len(pos)))
    if leaf == 4:  # MeshEngine::load -> createBVH builds the same tree from the aiScene (always the default leaf of 4)
        assert_trees_equal(rs.bvh(engine_tree=True), ot, (name, "createBVH"))
    rs.close(), os_.close()


@pytest.mark.parametrize("kind", SOUP_KINDS)
def test_tree_and_get_intersection_on_soups(kind):
    """the soups of test_random_soups_production_kernels_bit_exact: zero-thickness boxes, exact ties between duplicated
    triangles (the first tested wins, bvh.cpp:90), slivers and zero-area triangles, huge over tiny"""
    rng = np.random.default_rng(SOUP_SEEDS[kind])
    for n, leaf in SOUP_SIZES:
        pos, nrm, uv = random_soup(rng, n, kind)
        rs, os_ = R.RefScene(pos, nrm, uv, leaf_size=leaf), O.OracleScene(pos, nrm, uv, leaf_size=leaf)
        assert_trees_equal(rs.bvh(), os_.bvh(), (kind, n, leaf))
        o, d = rays_inside_and_outside(pos, 30000, n + leaf)
        # rays aimed exactly at triangle centroids: on "duplicates" every such hit is a tie between copies
        r = np.random.default_rng(n)
        pick = r.integers(0, n, 10000)
        c = pos.reshape(-1, 3, 3)[pick].astype(np.float64).mean(axis=1)
        oc = (c + r.normal(size=c.shape) * 700).astype(np.float32)
        o, d = np.concatenate([o, oc]), np.concatenate([d, unit(c - oc)])
        tri, t = assert_trace_equal(rs, os_, o, d, (kind, n, leaf))
        if n >= 700:
            assert (tri >= 0).sum() > 1000, (kind, n)
        # RayCast goes through createBVH's tree (always leaf 4; another leaf size resolves coplanar overlaps differently)
        os4 = os_ if leaf == 4 else O.OracleScene(pos, nrm, uv, leaf_size=4)
        assert_raycast_equal(rs, os4, o[::4], d[::4], (kind, n, "raycast"))  # meshes without UVs
        rs.close(), os_.close(), os4.close()


# ---- BVH::getIntersection ---------------------------------------------------------------------------------------------
def test_get_intersection_bit_exact(named_scene):
    name, (pos, nrm, uv), camf = named_scene
    n = 20000 if name == "cornell8" else 60000
    o, d = rays_inside_and_outside(pos, n, 21)
    c = camf()
    cam = va.make_camera(c["position"], c["rotation_deg"], 160, 96, 4)
    po, pd = O.primary_rays(cam, va.make_opts(seed=3), 1)
    o, d = np.concatenate([o, po]), np.concatenate([d, pd])
    for leaf in (4, 1) if name in ("cornell8", "lattice") else (4,):
        rs, os_ = R.RefScene(pos, nrm, uv, leaf_size=leaf), O.OracleScene(pos, nrm, uv, leaf_size=leaf)
        tri, t = assert_trace_equal(rs, os_, o, d, (name, leaf))
        assert (tri >= 0).sum() > 2000 and (tri < 0).sum() > 2000
        rs.close(), os_.close()


@pytest.mark.parametrize("name", ["cornell8", "lattice"])
def test_get_intersection_special_rays(name):
    """NaN and zero direction components (NaN slabs), rays lying in box faces, the fixtures' special rays"""
    pos, nrm, uv = scenes.SCENES[name][0]()
    o, d = special_rays()
    g = np.load(os.path.join(GOLD, name + ".npz"))
    o, d = np.concatenate([o, g["ray_o"]]), np.concatenate([d, g["ray_d"]])
    for leaf in (4, 1, 2):
        rs, os_ = R.RefScene(pos, nrm, uv, leaf_size=leaf), O.OracleScene(pos, nrm, uv, leaf_size=leaf)
        assert_trace_equal(rs, os_, o, d, (name, leaf))
        if leaf == 4:
            assert_raycast_equal(rs, os_, o, d, (name, "special"))
        rs.close(), os_.close()
    # the committed fixture is the oracle's own output: with the reference agreeing, it is the reference's too
    rs = R.RefScene(pos, nrm, uv)
    tri, t = rs.trace(g["ray_o"], g["ray_d"])
    assert np.array_equal(tri, g["trace_id"]) and nbad(t, g["trace_t"]) == 0
    rs.close()


# ---- MeshEngine::RayCast / RayCastCollision -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell8", "lattice", "bunny70k"])
def test_raycast_records_bit_exact(name):
    pos, nrm, uv = scenes.SCENES[name][0]()
    rs, os_ = R.RefScene(pos, nrm, uv), O.OracleScene(pos, nrm, uv)
    o, d = rays_inside_and_outside(pos, 50000 if name != "bunny70k" else 20000, 31)
    h = assert_raycast_equal(rs, os_, o, d, (name, "random"))
    assert ((h["flags"] & 2) != 0).sum() > 1000 and ((h["flags"] & 2) == 0).sum() > 1000
    if name != "bunny70k":
        o, d = wall_rays()
        assert_raycast_equal(rs, os_, o, d, (name, "walls"))
    o, d = light_rays(40000, 32)
    h = assert_raycast_equal(rs, os_, o, d, (name, "lights"))
    assert (np.abs(h["colour"]).sum(axis=1) > 0).sum() > 5000
    rs.close(), os_.close()


def test_raycast_meshes_without_uvs_and_several_meshes():
    """a mesh without texture coordinates leaves createBVH's default-constructed glm::vec2 in its triangles: zeros under
    the stand-in (the kUvOfMeshesWithoutUvs reading), and the oracle's uv=None gives the same records.  Several meshes in
    one scene: *ppImpactMaterial is taken from slot 0 whatever mesh was hit (hitMeshIndex = 0, meshEngine.cpp:370)."""
    pos, nrm, uv = scenes.lattice()
    o, d = rays_inside_and_outside(pos, 40000, 41)
    rs, os_ = R.RefScene(pos, nrm, None), O.OracleScene(pos, nrm, None)
    h = assert_raycast_equal(rs, os_, o, d, "no uvs")
    assert (h["tri_id"] >= 0).sum() > 5000 and not h["uv"].any()
    rs.close(), os_.close()
    # three meshes, the middle one without UVs: its triangles interpolate zeros, the others their own coordinates
    sizes = [60, 80, 60]
    uv_mixed = uv.copy()
    uv_mixed[60:140] = 0
    rs, os_ = R.RefScene(pos, nrm, uv, mesh_sizes=sizes, mesh_has_uv=[1, 0, 1]), O.OracleScene(pos, nrm, uv_mixed)
    a = rs.raycast(o, d)
    h = assert_raycast_equal(rs, os_, o, d, "three meshes")
    hit_mesh = np.searchsorted(np.cumsum(sizes), h["tri_id"], side="right")
    for m in range(3):
        assert ((h["tri_id"] >= 0) & (hit_mesh == m)).sum() > 500, m
    assert set(np.unique(a["pad"])) == {0, 1}  # material slot 0 (+1) or none, never the hit mesh's own
    assert h["uv"][(h["tri_id"] >= 0) & (hit_mesh != 1)].any() and not h["uv"][(h["tri_id"] >= 0) & (hit_mesh == 1)].any()
    rs.close(), os_.close()


@pytest.mark.parametrize("name", ["cornell8", "lattice"])
def test_raycast_collision(name):
    """RayCastCollision: `tw && ii.t > 1e-3` with a float t against a double literal (meshEngine.cpp:202); the oracle's
    answer is that expression on orc_trace's result.  Origins pulled back to within [0, 2e-3] of a hit straddle it."""
    pos, nrm, uv = scenes.SCENES[name][0]()
    rs, os_ = R.RefScene(pos, nrm, uv), O.OracleScene(pos, nrm, uv)
    o, d = rays_inside_and_outside(pos, 120000, 51)
    tri, t = os_.trace(o, d)
    keep = (tri >= 0) & (t > 1.0)
    o, d, t = o[keep], d[keep], t[keep]
    back = np.random.default_rng(52).uniform(0, 2e-3, len(t)).astype(np.float32)
    o2 = (o + d * (t - back)[:, None]).astype(np.float32)
    o, d = np.concatenate([o, o2]), np.concatenate([d, d])
    tri, t = os_.trace(o, d)
    expect = (tri >= 0) & (t.astype(np.float64) > 1e-3)
    near = (tri >= 0) & (t <= 2e-3)
    assert near.sum() > 1000 and expect[near].any() and (~expect[near]).any()
    got = rs.collision(o, d)
    assert np.array_equal(got, expect), int((got != expect).sum())
    rs.close(), os_.close()


# ---- VermiTexture::Sample ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("size", [(1, 7), (7, 1), (2, 2), (64, 32)])  # (W, H)
def test_texture_sample(channels, size):
    w, h = size
    r = np.random.default_rng(w * 100 + h * 10 + channels)
    tex = r.random((h, w, channels), dtype=np.float32) if channels > 1 else r.random((h, w), dtype=np.float32)
    grid = np.float32([-3, -2, -1, -0.5, -0.0, 0, 0.25, 0.5, 0.75, 1, 2, 3, 1e-8, -1e-8, 1 - 2**-24, -1 + 2**-24,
                       0.4999999, 0.5000001, 123456.78, -123456.78, 8388607.5, -8388608, 1e30, -1e30, 3.4e38, -3.4e38])
    gu, gv = np.meshgrid(grid, grid)
    half = (np.arange(4 * max(w, h) + 1, dtype=np.float32) / np.float32(2 * max(max(w, h) - 1, 1)))  # texel centres and edges
    uv = np.concatenate([np.stack([gu.ravel(), gv.ravel()], 1), np.stack([half, half[::-1]], 1),
                         r.uniform(-4, 4, (20000, 2)).astype(np.float32)]).astype(np.float32)
    a, b = R.texture_sample(tex, uv), O.texture_sample(tex, uv)
    assert nbad(a, b) == 0, (size, channels, nbad(a, b))
    assert not (a == -1).any()  # every component written


# ---- Radiance -----------------------------------------------------------------------------------------------------------
def corridor():
    """the textured scene: two large facing quads (floor y=132, just under light 1, and a lid at y=600) with UVs, so that a bounce off one lands on the
    other and every hit has a material — the only place a deep path multiplies texture samples into its throughput"""
    a = scenes._quad((-1500, 132, 1500), (1500, 132, 1500), (1500, 132, -1500), (-1500, 132, -1500), (0, 1, 0))
    b = scenes._quad((-1500, 600, 1500), (1500, 600, 1500), (1500, 600, -1500), (-1500, 600, -1500), (0, -1, 0))
    P, N, T = (np.concatenate([x[i] for x in (a, b)]) for i in range(3))
    T = T * np.float32(40.0) - np.float32(0.7)  # UVs far outside [0, 1): the wrap; about 75 units of floor per texture
    pos, nrm, uv = scenes._finish(P, N, T)
    tex = np.random.default_rng(5).uniform(0.2, 1.0, (32, 64, 3)).astype(np.float32)
    return pos, nrm, uv, tex


def radiance_inputs(name, pos, nrm, camf, seeds_fixture):
    """≥ 10^5 paths whose starts are chosen to reach every arm of Radiance (random rays return light in < 1 path of 500)"""
    r = np.random.default_rng(61)
    sets = []
    if camf is not None:
        c = camf()
        cam = va.make_camera(c["position"], c["rotation_deg"], 200, 120, 4)
        sets.append(O.primary_rays(cam, va.make_opts(seed=3), 2))  # the scene's camera: 24,000 paths
    sets.append(light_rays(24000, 62))                             # light at depth 0, and near misses
    # mirror rays: aimed at a point of the geometry so that the specular reflection (1 draw in 25) heads for a light
    tris = pos.reshape(-1, 3, 3).astype(np.float64)
    pick = r.integers(0, len(tris), 30000)
    w = r.dirichlet((1, 1, 1), len(pick))
    p = (tris[pick] * w[:, :, None]).sum(axis=1)
    nrm_g = np.cross(tris[pick, 1] - tris[pick, 0], tris[pick, 2] - tris[pick, 0])
    nrm_g /= np.maximum(np.linalg.norm(nrm_g, axis=1, keepdims=True), 1e-30)
    nrm_s = (nrm.reshape(-1, 3, 3).astype(np.float64)[pick] * w[:, :, None]).sum(axis=1)  # the interpolated normal
    nrm_s /= np.maximum(np.linalg.norm(nrm_s, axis=1, keepdims=True), 1e-30)               # is what Radiance mirrors on
    to_light = np.where(r.random((len(p), 1)) < 0.5, LIGHT1.astype(np.float64), LIGHT2.astype(np.float64)) - p
    to_light /= np.linalg.norm(to_light, axis=1, keepdims=True)
    incoming = to_light - 2 * (to_light * nrm_s).sum(1, keepdims=True) * nrm_s  # its mirror image leaves toward the light
    sets.append(((p - incoming * 300).astype(np.float32), unit(incoming)))
    # from points just off the geometry, aimed at and around the lights (diffuse starts next to surfaces)
    off = p[:12000] + nrm_g[:12000] * np.where((to_light[:12000] * nrm_g[:12000]).sum(1, keepdims=True) > 0, 0.5, -0.5)
    tgt = np.where(r.random((len(off), 1)) < 0.5, LIGHT1.astype(np.float64), LIGHT2.astype(np.float64))
    sets.append((off.astype(np.float32), unit(tgt + r.normal(size=off.shape) * 30 - off)))
    sets.append(rays_inside_and_outside(pos, 12000, 63))            # misses at depth 0 and plain diffuse bounces
    o = np.concatenate([s[0] for s in sets])
    d = np.concatenate([s[1] for s in sets])
    # directions that are no rays (NaN, zero): the only way to miss at depth 0 inside the room of wall spheres
    no = np.tile(np.float32([[0, 300, 900]]), (300, 1))
    nd = np.tile(np.float32([[np.nan, np.nan, np.nan], [0, 0, 0], [np.nan, 1, 0]]), (100, 1))
    o, d = np.concatenate([o, no]), np.concatenate([d, nd])
    seeds = (np.arange(len(o), dtype=np.uint64) + np.uint64(1000003))
    # deep paths: seeds whose r2 draws keep a path alive to the roulette of depth > 5 (tools/make_ref_golden.py).
    # sphere walk: from a corner of the room with no geometry above or below, bouncing floor sphere <-> ceiling sphere
    sw = seeds_fixture["sphere_walk"]
    so = np.tile(np.float32([[1700, 500, -1700]]), (len(sw), 1))
    sd = np.tile(np.float32([[0, -1, 0]]), (len(sw), 1))
    o, d, seeds = np.concatenate([o, so]), np.concatenate([d, sd]), np.concatenate([seeds, sw])
    if name == "corridor":  # triangle to triangle, three draws a step
        cw = seeds_fixture["corridor"]
        co = np.tile(np.float32([[0, 350, 0]]), (len(cw), 1))
        cd = np.tile(np.float32([[0, -1, 0]]), (len(cw), 1))
        o, d, seeds = np.concatenate([o, co]), np.concatenate([d, cd]), np.concatenate([seeds, cw])
        # onto the floor right under light 1 (centre 8 above it, radius 3.5): about a fifth of the surviving diffuse
        # bounces (r2 < 1: one draw in ten) run into the light with a texture sample in their throughput
        n = 40000
        fp = np.stack([15 + r.uniform(-5, 5, n), np.full(n, 132.0), 25 + r.uniform(-5, 5, n)], 1)
        fo = fp + np.stack([r.uniform(-300, 300, n), np.full(n, 200.0), r.uniform(-300, 300, n)], 1)
        o, d = np.concatenate([o, fo.astype(np.float32)]), np.concatenate([d, unit(fp - fo)])
        seeds = np.concatenate([seeds, np.arange(n, dtype=np.uint64) + np.uint64(77000001)])
    assert len(o) >= 100000
    return o, d, seeds


_branch_totals = {}


@pytest.mark.parametrize("reading", ["default", "libm_double"])
@pytest.mark.parametrize("name", ["cornell8", "lattice", "corridor"])
def test_radiance_bit_exact(name, reading):
    """orc_radiance_mt against the reference's Radiance with the same per-path mt19937_64 seeds.  `default`: cos / sin of
    a float argument are cosf / sinf (libvmx_ref.so, sampling 0); `libm_double`: C's double functions
    (libvmx_ref_libmdouble.so, VMX_SAMPLING_LIBM_DOUBLE).  VMX_SAMPLING_CORRECTED corresponds to no reference text."""
    seeds_fixture = np.load(os.path.join(GOLD, "ref_seeds.npz"))
    if name == "corridor":
        pos, nrm, uv, tex = corridor()
        camf = lambda: dict(position=(0.0, 350.0, 1400.0), rotation_deg=(8.0, 0.0, 0.0))
    else:
        (pos, nrm, uv), tex = scenes.SCENES[name][0](), None
        camf = scenes.SCENES[name][1]
    which, sampling = (R.PARITY, 0) if reading == "default" else (R.LIBM_DOUBLE, va._lib.VMX_SAMPLING_LIBM_DOUBLE)
    rs, os_ = R.RefScene(pos, nrm, uv, which=which), O.OracleScene(pos, nrm, uv)
    if tex is not None:
        rs.bind_texture(tex), os_.bind_texture(tex)
    o, d, seeds = radiance_inputs(name, pos, nrm, camf, seeds_fixture)
    want, branches = os_.radiance_mt_branches(o, d, seeds, sampling)
    got = rs.radiance_mt(o, d, seeds)
    counts = {k: int(((branches & v) != 0).sum()) for k, v in O.BRANCHES.items()}
    print(f"radiance {name} {reading}: {len(o)} paths, branches {counts}, differing {nbad(got, want)}")
    assert nbad(got, want) == 0, (name, reading, nbad(got, want), len(o))
    assert nbad(os_.radiance_mt(o, d, seeds, sampling), want) == 0  # the counting entry is the plain one
    # the floor is a condition on the inputs, taken from the oracle alone: a branch nobody exercised fails here
    for k, c in counts.items():
        assert c >= BRANCH_FLOOR, (name, reading, k, c)
    if tex is not None:  # texture samples reached results: lit paths with a diffuse triangle bounce, many distinct colours
        textured = ((branches & O.BRANCHES["diffuse_triangle"]) != 0) & ((branches & O.BRANCHES["light_deeper"]) != 0)
        assert textured.sum() >= BRANCH_FLOOR, int(textured.sum())
        assert len(np.unique(bits(want[textured, :3]), axis=0)) >= BRANCH_FLOOR // 2
        print(f"  textured lit paths {int(textured.sum())}, distinct colours {len(np.unique(bits(want[textured, :3]), axis=0))}")
    rs.close(), os_.close()


# ---- Camera::saveFrame -------------------------------------------------------------------------------------------------
def test_save_frame_quantisation():
    """saveFrame's float -> unsigned char conversion (camera.cpp:159-163) on the values Render can store: setPixelValue
    receives colours clamped to [0, 1], alpha 1 and a sample count as depth"""
    r = np.random.default_rng(71)
    W, H = 64, 48
    f = np.empty((W * H, 5), np.float32)
    f[:, :3] = r.random((W * H, 3), dtype=np.float32)
    f[:200, :3] = np.float32([0, 1, 0.5, 1 / 255, 254.999 / 255, 0.99999994])[r.integers(0, 6, (200, 3))]
    f[:, 3] = 1.0
    f[:, 4] = r.integers(1, 257, W * H)
    a_rgba, a_depth = R.quantize(f, W, H)
    b_rgba, b_depth = O.quantize(f)
    assert np.array_equal(a_rgba, b_rgba) and nbad(a_depth, b_depth) == 0


# ---- -Ofast: measured by tools/ref_pin_report.py into profiles/ref_pin.txt, never asserted ---------------------------
def test_fast_build_loads_and_runs():
    pos, nrm, uv = scenes.cornell8()
    rs = R.RefScene(pos, nrm, uv, which=R.FAST)
    assert rs.l.ref_build_flags() == b"-Ofast"
    o, d = rays_inside_and_outside(pos, 1000, 81)
    tri, t = rs.trace(o, d)
    assert tri.shape == (1000,) and (tri >= 0).any()
    rs.close()
