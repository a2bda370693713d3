"""List pixels' camera rays settled where k_raygen forms them (k_raygen<0, true>, the walk-slot list of k_walk_words,
the straggler source of k_trace_w<0>): in a fused plain camera pass of a run with list claims the ray generation kernel
runs pc_list_settle (pixel_claim.h) on every ray of a listed pixel, writes the hit record of those it settles and leaves
the path ids of the others to the traversal kernel, which otherwise walks only the pixels without a list.

Three routes render every case: the new one (form 4 | 0x100), the same call with vmx_opts.reserved[0] bit 12 (claimed
pixels not fused: the rule runs at refill time in k_trace_w<0>, over every unclaimed ray) and with bit 13 (no lists: every
unclaimed ray walks).  Frames are bit-identical to each other and to the oracle's, the counts of vmx_stats are equal, the
claim kernel stays the one launch under `other`, and vmx_list_settled_rays is EQUAL with and without bit 12: the same rule
on the same rays.  The stragglers (rays of listed pixels that the rule leaves to the walk) are n_list x spp - settled;
at least one scene must have some, so that the straggler source is really traced.

Scenes and sizes are those of test_gpu_claimed_fused.py."""
import os

import numpy as np
import pytest

import claim_list_spec as LS
import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORM = 4 | 0x100  # every pass split, one-phase shading: the plain camera pass
NOT_FUSED = 0x1000
NO_LISTS = 0x2000
ROUTES = (0, NOT_FUSED, NO_LISTS)
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
# (samples per pixel, early stop, samples per pass, world, rank): 64; 128 in one pass (two chunks of 64 per pixel); 128 in
# two passes of 64; 3600 with early stop on a quarter of the frame (the first pass takes 61 + 3 = 64 samples; the later
# ones run over shrunken pixel lists, and all three slot lists are rebuilt for each); one stripe call
CASES = [(64, False, 0, 1, 0), (128, False, 0, 1, 0), (128, False, 64, 1, 0), (3600, True, 0, 1, 0), (64, False, 0, 2, 1)]
CASE_IDS = ["64", "128", "128x2", "3600es", "stripe"]
WALL_POSE = dict(position=(200.0, 300.0, -600.0), rotation_deg=(20.0, 30.0, 0.0))  # test_gpu_claimed_fused.py: every pixel claimed


class Loaded:
    def __init__(self, name):
        (pos, nrm, uv), self.cam_desc = SCENES[name][0]()
        self.name, self.size = name, SCENES[name][1]
        self.gpu = va.Scene(pos, nrm, uv, device=0)
        self.cpu = O.OracleScene(pos, nrm, uv)
        self.refs = {}

    def camera(self, spp, desc=None):
        W, H = self.size
        if spp > 1024:
            W, H = W // 2, H // 2
        desc = desc or self.cam_desc
        return va.make_camera(desc["position"], desc["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))

    def reference(self, case):
        """the oracle's frame of a case, rendered once, shared and never written to"""
        if case not in self.refs:
            spp, es, _, world, rank = case
            img, st = self.cpu.render(self.camera(spp), va.make_opts(seed=4, early_stop=es, world=world, rank=rank))
            img.setflags(write=False)
            self.refs[case] = (img, st)
        return self.refs[case]

    def render(self, cam, **kw):
        img, st = self.gpu.render(cam, va.make_opts(seed=4, **kw))
        return img, st, self.gpu.timings()["other"]["launches"], self.gpu.list_settled_rays()

    def three(self, cam, **kw):
        """(frame, stats, `other` launches, settled rays) of the new route, the bit-12 route and the bit-13 route"""
        return [self.render(cam, pipeline=FORM | off, **kw) for off in ROUTES]

    def listed_pixels(self, cam, **kw):
        _, lists, _ = self.gpu.pixel_claim_lists(cam, va.make_opts(seed=4, **kw))
        return int(np.sum(LS.list_lengths(lists) > 0))


@pytest.fixture(scope="module")
def all_loaded():
    s = {name: Loaded(name) for name in SCENES}
    yield s
    for v in s.values():
        v.gpu.close()


@pytest.fixture(params=list(SCENES))
def loaded(request, all_loaded):
    return all_loaded[request.param]


def same_counts(sa, sb):
    for k in COUNT_KEYS:
        assert sa[k] == sb[k], k
    for stage in ("primary", "bounce"):
        for k in STAGE_KEYS:
            assert sa[stage][k] == sb[stage][k], (stage, k)


def check_three(out, ref, rst, claims=True):
    """claims: the run builds the claim planes (one launch under `other`; none below the claims' sample threshold)"""
    (a, sa, la, na), (b, sb, lb, nb), (c, sc, lc, nc) = out
    assert np.array_equal(bits(a), bits(ref)), "frame differs from the oracle's"
    assert np.array_equal(bits(a), bits(b)), "the rule in k_raygen / in k_trace_w<0> (bit 12) differ"
    assert np.array_equal(bits(a), bits(c)), "lists on / off (bit 13) differ"
    same_counts(sa, sb)
    same_counts(sa, sc)
    if rst is not None:
        assert sa["samples"] == rst["samples"]
    assert la == lb == lc == (1 if claims else 0)  # the claim kernel, and nothing else, under `other`
    assert na == nb, "the same rule on the same rays settles the same number"
    assert nc == 0
    return na


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_frames_counts_and_settled_rays(loaded, case):
    spp, es, batch, world, rank = case
    cam = loaded.camera(spp)
    ref, rst = loaded.reference(case)
    out = loaded.three(cam, early_stop=es, samples_per_batch=batch, world=world, rank=rank)
    settled = check_three(out, ref, rst)
    print("%s %s: %d of %d camera rays settled by a list" % (loaded.name, case, settled, out[0][1]["rays_primary"]))
    assert settled < out[0][1]["rays_primary"]
    if loaded.name != "soup":
        assert settled > 0
    if es:
        assert out[0][1]["passes"] > 1  # the planes were reused, and the three lists rebuilt, over shrunken pixel lists
    else:  # every listed pixel takes spp samples: what the rule did not settle was traced as a straggler
        n_list = loaded.listed_pixels(cam, world=world, rank=rank)
        stragglers = n_list * spp - out[1][3]  # by the bit-12 route
        print("%d listed pixels, %d stragglers" % (n_list, stragglers))
        assert 0 <= stragglers <= n_list * spp
        assert n_list * spp - out[0][3] == stragglers


def test_stragglers_are_traced(all_loaded):
    """the rays of listed pixels that the rule leaves to the walk: n_list x spp - settled, from the bit-12 route; where a
    scene has some, the new route shows the same number and still renders the oracle's frame"""
    seen = 0
    for name, s in all_loaded.items():
        cam = s.camera(64)
        n_list = s.listed_pixels(cam)
        _, _, _, settled_old = s.render(cam, early_stop=False, pipeline=FORM | NOT_FUSED)
        stragglers = n_list * 64 - settled_old
        print("%s: %d listed pixels, %d stragglers of %d rays" % (name, n_list, stragglers, n_list * 64))
        assert stragglers >= 0
        if stragglers > 0:
            img, st, _, settled_new = s.render(cam, early_stop=False, pipeline=FORM)
            ref, rst = s.reference((64, False, 0, 1, 0))
            assert n_list * 64 - settled_new == stragglers
            assert np.array_equal(bits(img), bits(ref))
            assert st["samples"] == rst["samples"]
            seen += 1
    assert seen > 0, "no scene has a straggler: add a camera pose that has, found with the bit-12 route"


def test_two_progressive_steps(loaded):
    """two steps of 64 samples of a 128-sample frame: each step is one fused pass"""
    cam = loaded.camera(128)
    ref, rst = loaded.reference((128, False, 0, 1, 0))
    out = []
    for off in ROUTES:
        steps = []
        with loaded.gpu.progressive(cam, va.make_opts(seed=4, early_stop=False, pipeline=FORM | off)) as p:
            for _ in range(2):
                st = p.step(64)
                steps.append((st, loaded.gpu.timings()["other"]["launches"], loaded.gpu.list_settled_rays()))
            assert p.info()["pixels_active"] == 0
            out.append((p.preview(), steps))
    (a, new), (b, old), (c, none) = out
    assert np.array_equal(bits(a), bits(ref)), "frame differs from the oracle's"
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    for (sa, la, na), (sb, lb, nb), (sc, lc, nc) in zip(new, old, none):
        same_counts(sa, sb)
        same_counts(sa, sc)
        assert la == lb == lc
        assert na == nb and nc == 0
    assert sum(s[0]["samples"] for s in new) == rst["samples"]


def test_every_pixel_claimed(all_loaded):
    """no unclaimed slot: the rule, the walk-slot list and the straggler source run over empty lists"""
    s = all_loaded["cornell8"]
    cam = s.camera(64, WALL_POSE)
    claims, _, n = s.gpu.pixel_claim_lists(cam, va.make_opts(seed=4))
    assert n == claims.size, "the pose no longer claims every pixel"
    ref, rst = s.cpu.render(cam, va.make_opts(seed=4, early_stop=False))
    settled = check_three(s.three(cam, early_stop=False), ref, rst)
    assert settled == 0


@pytest.mark.parametrize("spp", [16, 100])
def test_passes_that_are_not_fused(loaded, spp):
    """16 samples (below the claims' threshold: no planes) and 100 (ragged: a wave straddles two pixels): today's route,
    frames and counts unchanged, the rule where it was"""
    cam = loaded.camera(spp)
    ref, rst = loaded.cpu.render(cam, va.make_opts(seed=4, early_stop=False))
    settled = check_three(loaded.three(cam, early_stop=False), ref, rst, claims=spp >= 64)
    if spp == 16:
        assert settled == 0
