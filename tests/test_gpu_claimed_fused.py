"""Claimed pixels fused into the camera shading kernel (k_shade<0, .., DENSE, CLAIMED>, the lists of launch_slot_lists,
k_raygen<0> / k_trace_w<0> over the unclaimed slots): in the plain one-phase split form a pass of a multiple of 64
samples forms, tests and shades the rays of its claimed pixels in one kernel.  Frames are bit-identical with the fused
route on and off (vmx_opts.reserved[0] bit 12) and identical to the oracle's, the counts of vmx_stats do not change, and
vmx_fused_camera_paths says how many camera paths took the route: the claimed pixels' samples where a pass is fused,
none in every other form.

Scenes and sizes are those of test_gpu_pixel_claims.py (claimed shares in profiles/pixel_claims.txt section 1: cornell8
59.5 % slot + 26.7 % MISS claims, sponza260k 19.6 % slot claims, the duplicate soup): each has claimed and unclaimed
pixels, more than one block of pixels, and pixel counts that are no multiple of the 8 bands."""
import os

import numpy as np
import pytest

import oracle_lib as O
import pixel_claim_spec as S
import vermilion_amd as va
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORM = 4 | 0x100  # every pass split, one-phase shading: the plain camera pass
NOT_FUSED = 0x1000
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
# two passes of 64; 3600 with early stop on a quarter of the frame (the first pass takes 61 + 3 = 64 samples and is fused;
# the later ones run over shrinking pixel lists, and the lists of unclaimed and claimed slots are rebuilt for each); one
# stripe call
CASES = [(64, False, 0, 1, 0), (128, False, 0, 1, 0), (128, False, 64, 1, 0), (3600, True, 0, 1, 0), (64, False, 0, 2, 1)]
CASE_IDS = ["64", "128", "128x2", "3600es", "stripe"]


class Loaded:
    def __init__(self, name):
        (pos, nrm, uv), self.cam_desc = SCENES[name][0]()
        self.size = SCENES[name][1]
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
        return img, st, self.gpu.timings()["other"]["launches"], self.gpu.fused_camera_paths()


@pytest.fixture(scope="module", params=list(SCENES))
def loaded(request):
    s = Loaded(request.param)
    yield s
    s.gpu.close()


def same_counts(sa, sb):
    for k in COUNT_KEYS:
        assert sa[k] == sb[k], k
    for stage in ("primary", "bounce"):
        for k in STAGE_KEYS:
            assert sa[stage][k] == sb[stage][k], (stage, k)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_frames_counts_and_the_fused_count(loaded, case):
    spp, es, batch, world, rank = case
    cam = loaded.camera(spp)
    ref, rst = loaded.reference(case)
    kw = dict(early_stop=es, samples_per_batch=batch, world=world, rank=rank)
    a, sa, la, fa = loaded.render(cam, pipeline=FORM, **kw)
    b, sb, lb, fb = loaded.render(cam, pipeline=FORM | NOT_FUSED, **kw)
    assert np.array_equal(bits(a), bits(b)), "fused route on / off differ"
    assert np.array_equal(bits(a), bits(ref)), "frame differs from the oracle's"
    same_counts(sa, sb)
    assert sa["samples"] == rst["samples"]
    assert la == lb == 1  # the claim kernel, and nothing else, under `other`: the lists are timed with the ray generation
    print("fused camera paths: %d of %d" % (fa, sa["rays_primary"]))
    assert fb == 0
    assert 0 < fa < sa["rays_primary"]
    if not es:  # every pixel takes spp samples, every pass is fused: the claimed pixels' samples, exactly
        claims, n = loaded.gpu.pixel_claims(cam, va.make_opts(seed=4, world=world, rank=rank))
        assert n == int(np.sum(claims != S.NONE))
        assert fa == n * spp
    else:
        assert sa["passes"] > 1  # the table was reused, and the lists rebuilt, over shrunken pixel lists


def test_two_progressive_steps(loaded):
    """two steps of 64 samples of a 128-sample frame: each step is one fused pass"""
    cam = loaded.camera(128)
    ref, rst = loaded.reference((128, False, 0, 1, 0))
    _, n = loaded.gpu.pixel_claims(cam, va.make_opts(seed=4))
    out = []
    for off in (0, NOT_FUSED):
        steps = []
        with loaded.gpu.progressive(cam, va.make_opts(seed=4, early_stop=False, pipeline=FORM | off)) as p:
            for _ in range(2):
                st = p.step(64)
                steps.append((st, loaded.gpu.timings()["other"]["launches"], loaded.gpu.fused_camera_paths()))
            assert p.info()["pixels_active"] == 0
            out.append((p.preview(), steps))
    (a, on), (b, no) = out
    assert np.array_equal(bits(a), bits(b)), "fused route on / off differ"
    assert np.array_equal(bits(a), bits(ref)), "frame differs from the oracle's"
    for (sa, la, fa), (sb, lb, fb) in zip(on, no):
        same_counts(sa, sb)
        assert la == lb
        assert fa == n * 64 and fb == 0
    assert sum(s[0]["samples"] for s in on) == rst["samples"]


def test_no_fused_path_in_the_other_forms(loaded):
    def fused(spp, **kw):
        loaded.gpu.render(loaded.camera(spp), va.make_opts(seed=4, early_stop=False, **kw))
        return loaded.gpu.fused_camera_paths()

    assert fused(64, pipeline=FORM) > 0
    assert fused(100, pipeline=FORM) == 0               # ragged: k_shade<0> is not dense, a wave straddles two pixels
    assert fused(64, pipeline=4) == 0                   # camera rays sorted by the traversal kernel
    assert fused(64, pipeline=4 | 0x200) == 0           # two-phase shading through k_shade_ends
    assert fused(64, pipeline=FORM, collect_counters=True) == 0  # the counting build traces every ray
    assert fused(16, pipeline=FORM) == 0                # below the claims' sample threshold: no table
    assert fused(64, pipeline=FORM | 0x800) == 0        # no claims
    # the ragged frame is still the oracle's (it runs the three-kernel route with claims, as before)
    img, _ = loaded.gpu.render(loaded.camera(100), va.make_opts(seed=4, early_stop=False, pipeline=FORM))
    ref, _ = loaded.cpu.render(loaded.camera(100), va.make_opts(seed=4, early_stop=False))
    assert np.array_equal(bits(img), bits(ref))


# cornell8, the camera 200 units in front of the back wall and turned off the axes: every camera ray of every pixel hits
# one and the same triangle, and tests/cpp/pixel_claim_test.cpp claims all 96 x 64 pixels of this pose for it.  (Facing
# the wall squarely does not do: the pixels whose rays straddle a zero direction component keep their walk — 159 of
# 6,144 at position (300, 200, -700), rotation 0.)
WALL_POSE = dict(position=(200.0, 300.0, -600.0), rotation_deg=(20.0, 30.0, 0.0))


def test_every_pixel_claimed():
    """the lists' edge: no unclaimed slot — k_raygen and k_trace_w<0> launch over an empty list and return"""
    s = Loaded("cornell8")
    try:
        cam = s.camera(64, WALL_POSE)
        claims, n = s.gpu.pixel_claims(cam, va.make_opts(seed=4))
        assert n == claims.size, "the pose no longer claims every pixel"
        img, st, _, f = s.render(cam, early_stop=False, pipeline=FORM)
        ref, rst = s.cpu.render(cam, va.make_opts(seed=4, early_stop=False))
        assert np.array_equal(bits(img), bits(ref))
        assert st["samples"] == rst["samples"]
        assert f == st["rays_primary"] == claims.size * 64
    finally:
        s.gpu.close()
