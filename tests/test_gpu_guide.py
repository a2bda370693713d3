"""The guide tree on the device (k_trace_w<1, .., GUIDE>, vermilion_amd/csrc/guide_walk.h): the bounce rays of a
reference-tree scene walk the scene's quality tree, a per-ray rule settles those for which the reference tree returns the
same (t, slot), and the unchanged kernel traces the others over the reference tree.  Frames are bit-identical with the
guide on and off (vmx_opts.reserved[0] bit 14) and identical to the oracle's, the counts of vmx_stats do not change, and
vmx_guide_rays counts the rays of either kind.

tail_threshold = 1 (reserved[2]) keeps the bounce generations split, so that they run in k_trace_w<1> and not in the
fused tail.  Scenes and sizes are those of test_gpu_claim_lists.py: more than one block of paths, sizes that are no
multiple of a wave, and in the soup every hit on a duplicated triangle is a fallback ray."""
import os

import numpy as np
import pytest

import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = (4, 4 | 0x100, 4 | 0x200)  # rays sorted by the traversal kernel; plain one-phase (dense records); two-phase
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
# (samples per pixel, sampling, world, rank)
CASES = [(64, va.VMX_SAMPLING_PARITY, 1, 0), (100, va.VMX_SAMPLING_PARITY, 1, 0), (16, va.VMX_SAMPLING_CORRECTED, 1, 0),
         (64, va.VMX_SAMPLING_PARITY, 2, 1)]
CASE_IDS = ["64", "100", "corrected16", "stripe"]


class Loaded:
    def __init__(self, name):
        (pos, nrm, uv), self.cam_desc = SCENES[name][0]()
        self.name, self.pos, self.nrm, self.uv, self.size = name, pos, nrm, uv, SCENES[name][1]
        self.gpu = va.Scene(pos, nrm, uv, device=0)
        self.cpu = O.OracleScene(pos, nrm, uv)

    def camera(self, spp):
        W, H = self.size
        return va.make_camera(self.cam_desc["position"], self.cam_desc["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))


@pytest.fixture(scope="module", params=list(SCENES))
def loaded(request):
    s = Loaded(request.param)
    yield s
    s.gpu.close()


def _opts(case, form, **kw):
    spp, sampling, world, rank = case
    return va.make_opts(seed=4, early_stop=False, sampling=sampling, pipeline=form, tail_threshold=1, world=world, rank=rank, **kw)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_frames_and_counts_with_and_without_the_guide(loaded, case):
    cam = loaded.camera(case[0])
    ref, rst = loaded.cpu.render(cam, _opts(case, 0))
    for form in FORMS:
        out = []
        for off in (0, NO_GUIDE):
            img, st = loaded.gpu.render(cam, _opts(case, form | off))
            out.append((img, st, loaded.gpu.guide_rays(), loaded.gpu.guide_list_entries()))
        (a, sa, (settled, fallback), handed), (b, sb, off_rays, off_handed) = out
        assert np.array_equal(bits(a), bits(b)), (hex(form), "guide on / off differ")
        assert np.array_equal(bits(a), bits(ref)), (hex(form), "frame differs from the oracle's")
        for k in COUNT_KEYS:
            assert sa[k] == sb[k], (hex(form), k)
        for stage in ("primary", "bounce"):
            for k in STAGE_KEYS:
                assert sa[stage][k] == sb[stage][k], (hex(form), stage, k)
        assert sa["samples"] == rst["samples"]
        assert off_rays == (0, 0) and off_handed == 0
        # `handed`: the entries of the lists the host handed to k_trace_w<1, .., GUIDE>, one per bounce ray it traces
        # (vmx_guide_list_entries).  Every path that goes on after a step is one entry of some generation's list; only a
        # last generation of a single path (tail_threshold = 1) runs in the fused tail instead, with its further steps.
        entries = sa["primary"]["continued"] + sa["bounce"]["continued"]
        print("%s form %s: %d settled + %d fallback of %d entries handed to the guide form (%d paths went on)"
              % (loaded.name, hex(form), settled, fallback, handed, entries))
        assert settled + fallback == handed, hex(form)
        assert 0 < handed <= entries, hex(form)
        if not loaded.gpu.timings()["tail"]["launches"]:
            assert handed == entries, hex(form)
        if loaded.name != "soup":
            assert settled > 0, hex(form)


def test_no_guide_where_it_must_stay_off(loaded):
    case = CASES[0]
    cam = loaded.camera(case[0])
    # the counting build: its visit counts are the oracle's
    loaded.gpu.render(cam, _opts(case, 4, collect_counters=True))
    assert loaded.gpu.guide_rays() == (0, 0)
    d = loaded.gpu.describe()
    ref_tree = loaded.cpu.describe()
    assert d["n_nodes"] == ref_tree["n_nodes"] and d["max_depth"] == ref_tree["max_depth"]  # still the reference tree
    # a quality-tree scene has no guide
    with va.Scene(loaded.pos, loaded.nrm, loaded.uv, device=0, builder=1) as sah:  # VMX_BVH_SAH
        sah.render(cam, _opts(case, 4))
        assert sah.guide_rays() == (0, 0)
        assert d["device_bytes"] > sah.describe()["device_bytes"]  # the guide is counted


def test_a_moved_vertex_retires_the_guide():
    (pos, nrm, uv), c = scenes.cornell8(), scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 96, 64, 64, back_size=(3.6, 2.4))
    case = CASES[0]
    moved = np.array(pos, np.float32, copy=True).reshape(-1, 9)
    moved[0, 0] += 0.25
    with va.Scene(pos, nrm, uv, device=0) as sc:
        sc.render(cam, _opts(case, 4))
        assert sc.guide_rays()[0] > 0
        sc.update(pos=moved)
        a, _ = sc.render(cam, _opts(case, 4))
        assert sc.guide_rays() == (0, 0)
        b, _ = sc.render(cam, _opts(case, 4 | NO_GUIDE))
        assert np.array_equal(bits(a), bits(b))
        # a REBUILD runs both host builders again, beside each other: the guide of the new positions, as a fresh scene's
        sc.update(pos=moved, rebuild=True)
        a, _ = sc.render(cam, _opts(case, 4))
        rebuilt_rays = sc.guide_rays()
        assert rebuilt_rays[0] > 0
        b, _ = sc.render(cam, _opts(case, 4 | NO_GUIDE))
        assert np.array_equal(bits(a), bits(b))
        with va.Scene(moved, nrm, uv, device=0) as fresh:
            f, _ = fresh.render(cam, _opts(case, 4))
            assert fresh.guide_rays() == rebuilt_rays
            assert np.array_equal(bits(a), bits(f))
            assert fresh.describe() == sc.describe()
