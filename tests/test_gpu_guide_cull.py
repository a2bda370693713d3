"""The device's guide walk with the skip of boxes that end behind the ray's origin (guide_walk.h, premise (B)).

The pin.  vmx_guide_trace_visits runs the counting form of k_trace_w<1, .., GUIDE> on explicit rays and returns, beside
what vmx_guide_trace returns, the inner records and the triangle tests of every ray's walk.  Held with no tolerance: the
device settles exactly the rays the host program (tests/cpp/guide_cull_test.cpp, the library's own marks) settles, with
its slot and the bits of its t; the device's visit counts equal the host program's RAY BY RAY — a device that never
skipped would pass every comparison of answers, and fails this one wherever the host walk skips; with the fallback
launch every ray carries the oracle's answer.

Frames.  Bit-identical to the oracle's, with the counts of vmx_stats equal to those of the same frame without the guide:
the split forms with tail_threshold = 1 and the default, the fused GUIDE forms (pipeline forms 0 and 1), corrected
sampling, one rank of a two-rank stripe, and after a REBUILD.

Fallback.  For every one of those frames, vmx_guide_rays (the split launches) and vmx_guide_fused_rays (the GUIDE forms
of k_paths: the tail and the fused passes, where culled guide lanes and reference lanes share a wave): settled + fallback
is the parent commit's total, and the fallback share is not above the parent's by more than a tenth — the skip must not
turn settled rays into fallback rays or restarts.  The parent's counts (PARENT below) are those of profiles/guide_tree.txt
section 4 and profiles/guide_fused.txt section 4 where those list the case, and for all cases what the parent commit's
library returned for these frames in the session of profiles/guide_cull.txt (section 6)."""
import os

import numpy as np
import pytest

import guide_cull_spec as S
import guide_spec as G
import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TREE_KEYS = ("start", "nprims", "right_offset", "bbox", "prim_order")
NO_GUIDE = 0x4000
COUNT_KEYS = ("rays_primary", "rays_secondary", "samples", "samples_discarded", "passes")
STAGE_KEYS = ("rays", "inner_visits", "tri_tests", "tri_hits", "continued")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _soup():
    g = np.load(os.path.join(HERE, "golden", "ref_soup_duplicates.npz"))
    return (g["pos"].reshape(-1, 9), g["nrm"].reshape(-1, 9), None), dict(position=tuple(g["cam"][:3]), rotation_deg=tuple(g["cam"][3:6]))


SCENES = {
    "cornell8": (lambda: (scenes.cornell8(), scenes.cornell_camera()), (96, 64)),
    "sponza260k": (lambda: (scenes.sponza260k(), scenes.sponza_camera()), (160, 90)),
    "soup": (_soup, (96, 64)),
}


# ---- the pin
def pin(name, pos, nrm, uv, o, d, gpu=None, must_skip=False):
    """the device's walk against the host program's for the rays (o, d); returns (host walk that never skips, host walk
    with the library's marks)"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    o, d = np.ascontiguousarray(o, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    n = len(o)
    sc = va.Scene(pos, nrm, uv, device=0) if gpu is None else gpu
    try:
        cpu = O.OracleScene(pos, nrm, uv)
        tree = sc.bvh()
        ref = cpu.bvh()
        for k in TREE_KEYS:  # a reference-tree scene: the device's tree is the oracle's
            assert np.array_equal(np.asarray(tree[k]).view(np.uint32), np.asarray(ref[k]).view(np.uint32)), k
        plain, host = S.host_cull(pos, tree, o, d)
        tri, t = cpu.trace(o, d)
        assert int(S.wrong(tri, t, tree, host).sum()) == 0, name
        want = np.isin(host["verdict"], (G.SETTLED, G.MISS))
        for blocks in (0, 3):  # a render's grid, and three blocks: every lane takes many rays, one after the other
            settled, slot, dt, nv, nt = sc.guide_trace_visits(o, d, grid_blocks=blocks)
            s = settled.astype(bool)
            assert int(np.sum(s != want)) == 0, (name, blocks, "rays settled on one side only", np.flatnonzero(s != want)[:8])
            assert int(np.sum(slot[s] != host["slot"][s])) == 0, (name, blocks, "slots differ")
            assert int(np.sum(bits(dt[s]) != bits(host["t"][s]))) == 0, (name, blocks, "t differs")
            assert np.all(slot[~s] == G.NONE) and np.all(bits(dt[~s]) == 0), (name, blocks)
            assert int(np.sum(nv != host["inner"])) == 0, (name, blocks, "inner visits differ", np.flatnonzero(nv != host["inner"])[:8])
            assert int(np.sum(nt != host["tris"])) == 0, (name, blocks, "triangle tests differ", np.flatnonzero(nt != host["tris"])[:8])
            assert sc.guide_rays() == (int(s.sum()), n - int(s.sum())) and sc.guide_list_entries() == n, (name, blocks)
        # the plain entry runs the product kernel: the same answers
        ps, pslot, pt = sc.guide_trace(o, d)
        assert np.array_equal(ps, settled) and np.array_equal(pslot, slot) and np.array_equal(bits(pt), bits(dt)), name
        # with the launch over the fallback list every ray has the oracle's answer
        _, slot, dt, nv2, nt2 = sc.guide_trace_visits(o, d, complete=True)
        order = np.asarray(tree["prim_order"]).astype(np.int64)
        got = np.where(slot == G.NONE, -1, order[np.minimum(slot, len(order) - 1)])
        assert int(np.sum(got != tri)) == 0 and int(np.sum(bits(dt) != bits(t))) == 0, (name, "differs from the oracle")
        assert np.array_equal(nv2, nv) and np.array_equal(nt2, nt), name
        steps = [int(r["inner"].sum()) + int(r["tris"].sum()) for r in (plain, host)]
        print("%s: %d rays, %d settled; steps of the walk %d without the skip, %d with it (host and device): %.3f x"
              % (name, n, int(want.sum()), steps[0], steps[1], steps[1] / max(steps[0], 1)))
        if must_skip:
            assert steps[1] < 0.9 * steps[0], name
        return plain, host
    finally:
        if gpu is None:
            sc.close()


def _bounce_case(name):
    (pos, nrm, uv), c = SCENES[name][0]()
    W, H = SCENES[name][1]
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 64)
    if name == "soup":
        g = np.load(os.path.join(HERE, "golden", "ref_soup_duplicates.npz"))
        osc = O.OracleScene(pos, nrm, None, tree={k: g["bvh_" + k] for k in TREE_KEYS})
        o0, d0 = O.primary_rays(cam, va.make_opts(seed=3), 0)
        o1, d1 = G.bounce_rays(osc, cam, 3, "uniform")
        return pos, nrm, uv, np.concatenate([o0, o1]), np.concatenate([d0, d1])
    osc = O.OracleScene(pos, nrm, uv)
    rays = [G.bounce_rays(osc, cam, 5 + k, kind) for k, kind in enumerate(("parity", "corrected", "uniform"))]
    return pos, nrm, uv, np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])


@pytest.mark.parametrize("name", list(SCENES))
def test_pin_bounce_rays(name):
    pin("%s %dx%d" % ((name,) + SCENES[name][1]), *_bounce_case(name), must_skip=name == "sponza260k")


def test_pin_generator_cases():
    """every case of guide_cull_spec.cull_cases cut to about 4,000 rays"""
    kinds, skipped = 0, 0
    for kind, K, pos, o, d in S.cull_cases(4000):
        plain, host = pin(kind, pos, G.flat_normals(pos), None, o[:4000], d[:4000])
        kinds += 1
        skipped += int(np.any(host["inner"] < plain["inner"]) or np.any(host["tris"] < plain["tris"]))
    # (19 pushed constructions: every adversarial case but "zero direction component", which has no finite ray)
    assert kinds == len(S.FANS) + len(S.WALLS) + 19 and skipped >= 5


# ---- frames
class Loaded:
    def __init__(self, name):
        (pos, nrm, uv), self.cam_desc = SCENES[name][0]()
        self.name, self.pos, self.nrm, self.uv, self.size = name, pos, nrm, uv, SCENES[name][1]
        self.gpu = va.Scene(pos, nrm, uv, device=0)
        self.cpu = O.OracleScene(pos, nrm, uv)
        self.refs = {}

    def camera(self, spp):
        W, H = self.size
        return va.make_camera(self.cam_desc["position"], self.cam_desc["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))

    def reference(self, case):
        """the oracle's frame of a case, computed once"""
        if case not in self.refs:
            self.refs[case] = self.cpu.render(self.camera(case[0]), _opts(case, 0))[0]
        return self.refs[case]


@pytest.fixture(scope="module", params=list(SCENES))
def loaded(request):
    s = Loaded(request.param)
    yield s
    s.gpu.close()


def _opts(case, form, **kw):
    spp, sampling, world, rank = case
    return va.make_opts(seed=4, early_stop=False, sampling=sampling, pipeline=form, world=world, rank=rank, **kw)


def _check(loaded, case, form, gpu=None, **kw):
    """one frame with and without the guide: both the oracle's, the counts equal; returns the guide's counts"""
    gpu = loaded.gpu if gpu is None else gpu
    cam = loaded.camera(case[0])
    a, sa = gpu.render(cam, _opts(case, form, **kw))
    rays, fused, handed = gpu.guide_rays(), gpu.guide_fused_rays(), gpu.guide_list_entries()
    b, sb = gpu.render(cam, _opts(case, form | NO_GUIDE, **kw))
    tag = (loaded.name, case, hex(form), kw)
    assert np.array_equal(bits(a), bits(b)), (tag, "guide on / off differ")
    for k in COUNT_KEYS:
        assert sa[k] == sb[k], (tag, k)
    for stage in ("primary", "bounce"):
        for k in STAGE_KEYS:
            assert sa[stage][k] == sb[stage][k], (tag, stage, k)
    assert rays[0] + rays[1] == handed, tag
    return a, rays, fused


PARITY, CORRECTED = va.VMX_SAMPLING_PARITY, va.VMX_SAMPLING_CORRECTED
CASES = {"64": (64, PARITY, 1, 0), "corrected16": (16, CORRECTED, 1, 0), "stripe": (64, PARITY, 2, 1)}
# (settled, fallback) of the PARENT commit per scene and case: "split" — vmx_guide_rays of forms 4, 4|0x100, 4|0x200 with
# tail_threshold = 1; "tail" — vmx_guide_fused_rays of the same forms with the default threshold (every bounce generation
# of these frames runs in the tail); "fused" — vmx_guide_fused_rays of forms 0, 1 and 0x100 (fused passes, camera rays
# included)
PARENT = {
    ("cornell8", "64"): {"split": (54941, 0), "tail": (54941, 0), "fused": (448155, 2)},
    ("cornell8", "corrected16"): {"split": (1581553, 714221), "tail": (1581553, 714227), "fused": (1679855, 714229)},
    ("cornell8", "stripe"): {"split": (27920, 0), "tail": (27920, 0), "fused": (224526, 2)},
    ("sponza260k", "64"): {"split": (143744, 618), "tail": (143745, 618), "fused": (1063746, 2217)},
    ("sponza260k", "corrected16"): {"split": (5408543, 37092), "tail": (5408574, 37092), "fused": (5638553, 37513)},
    ("sponza260k", "stripe"): {"split": (67127, 273), "tail": (67127, 273), "fused": (497014, 466)},
    ("soup", "64"): {"split": (44421, 2223), "tail": (44421, 2223), "fused": (373519, 66341)},
    ("soup", "corrected16"): {"split": (1379164, 922392), "tail": (1379164, 922416), "fused": (1461435, 938449)},
    ("soup", "stripe"): {"split": (22049, 1550), "tail": (22050, 1550), "fused": (179865, 40343)},
}


def _share(loaded, cid, kind, got, tag):
    """settled + fallback is the parent's total; the fallback share is not above the parent's by more than a tenth"""
    settled, fallback = PARENT[(loaded.name, cid)][kind]
    print("%s %s %s %s: %d settled + %d fallback (parent %d + %d)" % (loaded.name, cid, kind, tag, got[0], got[1], settled, fallback))
    assert got[0] + got[1] == settled + fallback, (loaded.name, cid, kind, tag, got)
    assert got[1] * (settled + fallback) <= 1.1 * fallback * (got[0] + got[1]), (loaded.name, cid, kind, tag, got)


def test_frames_split_forms(loaded):
    case = CASES["64"]
    ref = loaded.reference(case)
    for form in (4, 4 | 0x100, 4 | 0x200):
        for kw in (dict(tail_threshold=1), dict()):
            img, rays, fused = _check(loaded, case, form, **kw)
            assert np.array_equal(bits(img), bits(ref)), (loaded.name, hex(form), kw, "frame differs from the oracle's")
            if kw:
                _share(loaded, "64", "split", rays, hex(form))
            else:
                assert rays == (0, 0)  # the default threshold: every bounce generation of this frame runs in the tail
                _share(loaded, "64", "tail", fused, hex(form))


def test_frames_fused_forms(loaded):
    case = CASES["64"]
    ref = loaded.reference(case)
    for form in (0, 1):
        img, rays, fused = _check(loaded, case, form)
        assert np.array_equal(bits(img), bits(ref)), (loaded.name, form, "frame differs from the oracle's")
        assert rays == (0, 0)
        _share(loaded, "64", "fused", fused, hex(form))


def test_frames_corrected_and_stripe(loaded):
    for cid in ("corrected16", "stripe"):
        case = CASES[cid]
        ref = loaded.reference(case)
        for form, kw, kind in ((4, dict(tail_threshold=1), "split"), (4, dict(), "tail"), (0x100, dict(), "fused"), (1, dict(), "fused")):
            img, rays, fused = _check(loaded, case, form, **kw)
            assert np.array_equal(bits(img), bits(ref)), (loaded.name, cid, hex(form), "frame differs from the oracle's")
            _share(loaded, cid, kind, rays if kind == "split" else fused, hex(form))


def test_frames_after_a_rebuild():
    (pos, nrm, uv), c = scenes.cornell8(), scenes.cornell_camera()
    moved = np.array(pos, np.float32, copy=True).reshape(-1, 9)
    moved[0, 0] += 0.25
    case = CASES["64"]
    cam = va.make_camera(c["position"], c["rotation_deg"], 96, 64, 64, back_size=(3.6, 2.4))
    ref, _ = O.OracleScene(moved, nrm, uv).render(cam, _opts(case, 0))
    with va.Scene(pos, nrm, uv, device=0) as sc:
        sc.update(pos=moved, rebuild=True)
        for form, kw in ((4, dict(tail_threshold=1)), (0, dict())):
            img, _ = sc.render(cam, _opts(case, form, **kw))
            assert np.array_equal(bits(img), bits(ref)), hex(form)
            assert sum(sc.guide_rays()) + sum(sc.guide_fused_rays()) > 0
        # the rebuilt guide carries fresh marks: the device's walk is the host program's over the moved triangles
        o, d = G.bounce_rays(O.OracleScene(moved, nrm, uv), va.make_camera(c["position"], c["rotation_deg"], 96, 64, 64), 7, "uniform")
        pin("cornell8 with a moved vertex, rebuilt", moved, nrm, uv, o, d, gpu=sc)
