"""The trees the GPU builds (VMX_BVH_LBVH, VMX_BVH_PLOC) against tree_spec.py, bit for bit, on the input families of
shared_inputs.py; and the device records against the oracle run over the SPEC's tree, never the exported one, so that
the records are held to a tree the device did not produce.  test_tree_spec.py checks on the CPU what is assumed here:
which inputs are within the traversal stack and which are refused."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import tree_spec as T
import vermilion_amd as va
from shared_inputs import TREE_FAMILY_NAMES, deep_lbvh, nan_cycle, tree_family
from test_gpu_update import scene_rays
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
BUILDERS = {"reference": L.VMX_BVH_REFERENCE, "sah": L.VMX_BVH_SAH, "lbvh": L.VMX_BVH_LBVH, "ploc": L.VMX_BVH_PLOC}
FAMILIES = tuple(f for f in TREE_FAMILY_NAMES if f != "huge")
SIZES = (1, 2, 3, 63, 64, 65, 1000)
LEAF_SIZES = (1, 4, 31)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_tree_is_spec(sc, spec, what):
    tree = sc.bvh()
    assert sc.describe()["n_nodes"] == len(spec["start"]), what
    for k in ("start", "nprims", "right_offset", "prim_order"):
        assert np.array_equal(tree[k], spec[k]), (what, k)
    assert np.array_equal(bits(tree["bbox"]), bits(spec["bbox"])), (what, "bbox")


def family_camera(pos):
    v = np.asarray(pos, np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, ext = (lo + hi) / 2, max(float((hi - lo).max()), 1.0)
    return va.make_camera((c[0], c[1], hi[2] + 1.2 * ext), (0.0, 0.0, 0.0), 48, 32, 16)


def assert_traces_like_oracle(sc, osc, pos, what, frames=True):
    o, d = scene_rays(pos)
    tri, t = sc.trace(o, d)
    otri, ot = osc.trace(o, d)
    assert np.array_equal(tri, otri) and np.array_equal(bits(t), bits(ot)), what
    if frames:
        cam = family_camera(pos)
        ref, _ = osc.render(cam, va.make_opts(seed=3, early_stop=False))
        for form in (0, 4):
            img, _ = sc.render(cam, va.make_opts(seed=3, early_stop=False, pipeline=form))
            assert np.array_equal(bits(img), bits(ref)), (what, "form", form)
    return tri


@pytest.mark.parametrize("leaf_size", LEAF_SIZES)
@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
@pytest.mark.parametrize("family", FAMILIES)
def test_device_tree_and_records_equal_the_spec(family, builder, leaf_size):
    hits = 0
    for n in SIZES + ((4096,) if leaf_size == 4 else ()):
        what = (family, builder, leaf_size, n)
        pos, nrm = tree_family(family, n)
        spec = T.build(builder, pos, leaf_size)
        assert spec is not None, what  # within the stack (test_tree_spec.py)
        with va.Scene(pos, nrm, None, leaf_size=leaf_size, builder=BUILDERS[builder]) as sc:
            assert_tree_is_spec(sc, spec, what)
            osc = O.OracleScene(pos, nrm, None, leaf_size=leaf_size, tree=spec)
            tri = assert_traces_like_oracle(sc, osc, pos, what)
            hits += int((tri >= 0).sum())
            osc.close()
    assert hits > 0


@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
@pytest.mark.parametrize("family", FAMILIES)
def test_rebuild_gives_the_spec_of_the_new_positions(family, builder):
    for n in (3, 65, 1000):
        pos, nrm = tree_family(family, n)
        new, _ = tree_family(family, n, seed=1)
        spec = T.build(builder, new, 4)
        assert spec is not None
        osc = O.OracleScene(new, nrm, None, tree=spec)
        for how in ("host", "device"):
            with va.Scene(pos, nrm, None, builder=BUILDERS[builder]) as sc:
                sc.update(pos=new if how == "host" else torch.from_numpy(new).cuda(), rebuild=True)
                assert_tree_is_spec(sc, spec, (family, builder, n, how))
                assert_traces_like_oracle(sc, osc, new, (family, builder, n, how), frames=False)
        osc.close()


@pytest.mark.parametrize("family", ["coincident", "same_box"])
def test_coincident_triangles_hit_alike_under_every_builder(family):
    """ties between triangles at one distance are resolved by test order, so the ids may differ between the trees: which
    rays hit and the bits of t may not"""
    for n in (65, 1000):
        pos, nrm = tree_family(family, n)
        o, d = scene_rays(pos)
        got = {}
        for name, b in BUILDERS.items():
            with va.Scene(pos, nrm, None, builder=b) as sc:
                tri, t = sc.trace(o, d)
                got[name] = (tri >= 0, bits(t).copy())
        assert got["reference"][0].any() and not got["reference"][0].all()
        for name in BUILDERS:
            assert np.array_equal(got[name][0], got["reference"][0]), (family, n, name)
            assert np.array_equal(got[name][1], got["reference"][1]), (family, n, name)


def test_radix_chain_is_refused_cleanly_and_other_builders_take_it():
    pos, nrm = deep_lbvh()
    assert T.build("lbvh", pos) is None  # 63 edges deep: test_tree_spec.py
    cp, cn, cuv = scenes.cornell8()
    o, d = scene_rays(cp)
    with va.Scene(cp, cn, cuv) as sc:
        tri0, t0 = sc.trace(o, d)
    with pytest.raises(L.VmxError) as e:
        va.Scene(pos, nrm, None, builder=L.VMX_BVH_LBVH)
    assert e.value.code == L.VMX_ERR_DEPTH
    with va.Scene(cp, cn, cuv) as sc:
        tri, t = sc.trace(o, d)
    assert np.array_equal(tri, tri0) and np.array_equal(bits(t), bits(t0)) and (tri >= 0).any()
    for leaf_size in LEAF_SIZES:
        spec = T.build("ploc", pos, leaf_size)
        with va.Scene(pos, nrm, None, leaf_size=leaf_size, builder=L.VMX_BVH_PLOC) as sc:
            assert_tree_is_spec(sc, spec, ("deep_lbvh", leaf_size))
            osc = O.OracleScene(pos, nrm, None, leaf_size=leaf_size, tree=spec)
            assert_traces_like_oracle(sc, osc, pos, ("deep_lbvh", "ploc", leaf_size))
            osc.close()
    osc = O.OracleScene(pos, nrm, None)  # builds the reference's tree itself
    with va.Scene(pos, nrm, None) as sc:
        assert_traces_like_oracle(sc, osc, pos, ("deep_lbvh", "reference"))
    osc.close()
    with va.Scene(pos, nrm, None, builder=L.VMX_BVH_SAH) as sc:
        osc = O.OracleScene(pos, nrm, None, tree=sc.bvh())  # a host builder: no restatement to hold it to
        assert_traces_like_oracle(sc, osc, pos, ("deep_lbvh", "sah"))
        osc.close()


@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
def test_overflowing_extents_build_the_spec_tree(builder):
    """finite coordinates near the end of float32: centroid sums, centroid bounds and box extents overflow.  From the
    code: an infinite extent makes the Morton scale 2097151 / inf = 0 and fmaxf drops the NaN of inf * 0, so those keys
    are 0 and the sort falls back on the triangle index; boxes are min / max of finite numbers; a NaN half area counts as
    the worst cost.  So the build succeeds and the tree is the spec's.  (Nothing is traced: that is not the builders'.)"""
    for n in SIZES + (4096,):
        pos, nrm = tree_family("huge", n)
        with va.Scene(pos, nrm, None, builder=BUILDERS[builder]) as sc:
            assert_tree_is_spec(sc, T.build(builder, pos, 4), ("huge", builder, n))


def test_nan_half_area_does_not_stall_the_clustering():
    """three finite triangles on which a NaN cost that never loses a comparison leaves no mutual pair ("a round merged
    nothing"): a legal scene, which builds"""
    pos, nrm = nan_cycle()
    for leaf_size in (1, 4):
        with va.Scene(pos, nrm, None, leaf_size=leaf_size, builder=L.VMX_BVH_PLOC) as sc:
            assert_tree_is_spec(sc, T.build("ploc", pos, leaf_size), ("nan_cycle", leaf_size))
