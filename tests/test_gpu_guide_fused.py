"""The guide tree in the fused kernel (the GUIDE forms of k_paths, vermilion_amd/csrc/guide_walk.h): where a frame's paths are kept to
their end in one launch -- the tail of a split pass, every pass of pipeline form 1, the small passes of form 0 -- a ray of
any depth that may walk the guide does, the per-ray rule settles it before the path is shaded, and a ray it does not
settle starts again over the reference tree in the same lane.  Frames are bit-identical with the guide on and off
(vmx_opts.reserved[0] bit 14) and identical to the oracle's, the counts of vmx_stats do not change, vmx_guide_fused_rays
counts every traversal of those launches once, and vmx_guide_rays / vmx_guide_list_entries keep counting the guided
split launches alone.

Scenes and sizes are those of test_gpu_guide.py: more than one block of paths, path counts that are no multiple of 64,
the soup, where every hit on a duplicated triangle falls back (the in-lane restart runs in most waves), and the Cornell
box under `corrected` sampling, where after a few bounces about a third of the origins lie beyond the rule's reach and
never walk the guide.  With the default tail_threshold every bounce generation of these frames runs in the tail."""
import os

import numpy as np
import pytest

import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TAIL_FORMS = (4, 4 | 0x100, 4 | 0x200)
NO_GUIDE = 0x4000
COUNT_KEYS = ("rays_primary", "rays_secondary", "samples", "samples_discarded", "passes")
STAGE_KEYS = ("rays", "tri_hits", "continued")


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
        self._ref = {}

    def camera(self, spp):
        W, H = self.size
        return va.make_camera(self.cam_desc["position"], self.cam_desc["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))

    def oracle(self, case, early_stop):
        """the oracle's frame and stats of a case, rendered once and not written to"""
        key = (case, early_stop)
        if key not in self._ref:
            img, st = self.cpu.render(self.camera(case[0]), _opts(case, 0, early_stop=early_stop))
            img.setflags(write=False)
            self._ref[key] = (img, st)
        return self._ref[key]


@pytest.fixture(scope="module", params=list(SCENES))
def loaded(request):
    s = Loaded(request.param)
    yield s
    s.gpu.close()


def _opts(case, form, early_stop=False, **kw):
    spp, sampling, world, rank = case
    return va.make_opts(seed=4, early_stop=early_stop, sampling=sampling, pipeline=form, world=world, rank=rank, **kw)


def _render(loaded, case, form, **kw):
    img, st = loaded.gpu.render(loaded.camera(case[0]), _opts(case, form, **kw))
    return img, st, loaded.gpu.guide_fused_rays(), loaded.gpu.guide_rays(), loaded.gpu.guide_list_entries()


def _same_frame_and_counts(loaded, case, form, on, off, early_stop=False):
    (a, sa), (b, sb) = on[:2], off[:2]
    ref, rst = loaded.oracle(case, early_stop)
    assert np.array_equal(bits(a), bits(b)), (hex(form), "guide on / off differ")
    assert np.array_equal(bits(a), bits(ref)), (hex(form), "frame differs from the oracle's")
    for k in COUNT_KEYS:
        assert sa[k] == sb[k], (hex(form), k)
    for stage in ("primary", "bounce"):
        for k in STAGE_KEYS:
            assert sa[stage][k] == sb[stage][k], (hex(form), stage, k)
    assert sa["samples"] == rst["samples"]
    assert off[2] == (0, 0) and off[3] == (0, 0) and off[4] == 0, hex(form)


def _shares(loaded, case, form, fused):
    settled, fallback = fused
    if loaded.name != "soup":
        assert settled > 0, hex(form)
    if loaded.name == "soup" or (loaded.name == "cornell8" and case[1] == va.VMX_SAMPLING_CORRECTED):
        assert fallback > 0, hex(form)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_tail_frames_and_counts_with_and_without_the_guide(loaded, case):
    for form in TAIL_FORMS:
        on = _render(loaded, case, form)
        off = _render(loaded, case, form | NO_GUIDE)
        _same_frame_and_counts(loaded, case, form, on, off)
        _, st, (settled, fallback), (split_settled, split_fallback), handed = on
        # every path that goes on after a step is one traversal, in a split launch's list or in the tail
        entries = st["primary"]["continued"] + st["bounce"]["continued"]
        print("%s form %s: %d settled + %d over the reference tree in the tail, %d entries handed to the split guide form, %d paths went on"
              % (loaded.name, hex(form), settled, fallback, handed, entries))
        assert settled + fallback == entries - handed, hex(form)
        assert split_settled + split_fallback == handed, hex(form)
        assert loaded.gpu.timings()["tail"]["launches"] > 0 and settled + fallback > 0, hex(form)
        _shares(loaded, case, form, (settled, fallback))
        # the same case with the bounce generations split (test_gpu_guide.py): the split launches' counters count those
        # launches alone, the tail's (a last generation of a single path, if any) the rest
        split = _render(loaded, case, form, tail_threshold=1)
        assert np.array_equal(bits(split[0]), bits(on[0])), hex(form)
        s_entries = split[1]["primary"]["continued"] + split[1]["bounce"]["continued"]
        assert s_entries == entries, hex(form)
        assert split[3][0] + split[3][1] == split[4] and 0 < split[4] <= entries, hex(form)
        assert split[2][0] + split[2][1] == entries - split[4], hex(form)
        assert split[4] >= handed, hex(form)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fused_passes_with_and_without_the_guide(loaded, case):
    for form, early_stop in ((1, False), (0, True)):
        on = _render(loaded, case, form, early_stop=early_stop)
        off = _render(loaded, case, form | NO_GUIDE, early_stop=early_stop)
        _same_frame_and_counts(loaded, case, form, on, off, early_stop)
        _, st, (settled, fallback), split_rays, handed = on
        print("%s form %d%s: %d settled + %d over the reference tree of %d + %d rays"
              % (loaded.name, form, " early stop" if early_stop else "", settled, fallback, st["rays_primary"], st["rays_secondary"]))
        if form == 1:
            # camera rays included; a traversal with a non-finite direction is traced and not counted as a ray
            assert settled + fallback >= st["rays_primary"] + st["rays_secondary"]
            assert split_rays == (0, 0) and handed == 0
        else:
            assert settled + fallback > 0
            assert split_rays[0] + split_rays[1] == handed
        _shares(loaded, case, form, (settled, fallback))


def test_no_guide_where_it_must_stay_off(loaded):
    case = CASES[0]
    for form in (4, 1):
        # the counting build: its visit counts are the oracle's
        assert _render(loaded, case, form, collect_counters=True)[2] == (0, 0)
        assert _render(loaded, case, form | NO_GUIDE)[2] == (0, 0)
        # a quality-tree scene has no guide
        with va.Scene(loaded.pos, loaded.nrm, loaded.uv, device=0, builder=1) as sah:  # VMX_BVH_SAH
            sah.render(loaded.camera(case[0]), _opts(case, form))
            assert sah.guide_fused_rays() == (0, 0)
            assert loaded.gpu.describe()["device_bytes"] > sah.describe()["device_bytes"]  # the guide is counted


def test_a_moved_vertex_retires_the_guide():
    (pos, nrm, uv), c = scenes.cornell8(), scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 96, 64, 64, back_size=(3.6, 2.4))
    case = CASES[0]
    moved = np.array(pos, np.float32, copy=True).reshape(-1, 9)
    moved[0, 0] += 0.25
    with va.Scene(pos, nrm, uv, device=0) as sc:
        for form in (4, 1):
            sc.render(cam, _opts(case, form))
            assert sc.guide_fused_rays()[0] > 0
        sc.update(pos=moved)
        for form in (4, 1):
            a, _ = sc.render(cam, _opts(case, form))
            assert sc.guide_fused_rays() == (0, 0)
            b, _ = sc.render(cam, _opts(case, form | NO_GUIDE))
            assert np.array_equal(bits(a), bits(b))
        # a REBUILD builds the guide of the new positions beside the tree, in the new allocation, as a fresh scene's
        sc.update(pos=moved, rebuild=True)
        with va.Scene(moved, nrm, uv, device=0) as fresh:
            for form in (4, 1):
                a, _ = sc.render(cam, _opts(case, form))
                rebuilt_rays = sc.guide_fused_rays()
                assert rebuilt_rays[0] > 0
                b, _ = sc.render(cam, _opts(case, form | NO_GUIDE))
                assert np.array_equal(bits(a), bits(b))
                f, _ = fresh.render(cam, _opts(case, form))
                assert fresh.guide_fused_rays() == rebuilt_rays
                assert np.array_equal(bits(a), bits(f))
            assert fresh.describe() == sc.describe()
