"""List claims on the device (k_pixel_claims' second plane, the refill branch of k_trace_w<0>): the rays of a pixel
without a single claim are tested against the pixel's short list of triangles and skip the BVH walk where pc_list_settle
(pixel_claim.h) says so.  Frames are bit-identical with lists on and off (vmx_opts.reserved[0] bit 13) and identical to
the oracle's, the counts of vmx_stats do not change, the device's list plane is the host program's
(tests/cpp/pixel_claim_list_test.cpp), and vmx_list_settled_rays counts the rays that took the route.

Scenes and sizes are those of test_gpu_pixel_claims.py: each has claimed, listed and walking pixels, more than one block
of pixels, and pixel counts that are no multiple of the 8 bands."""
import os

import numpy as np
import pytest

import claim_list_spec as LS
import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = (4, 4 | 0x100, 4 | 0x200)  # rays sorted by the traversal kernel; plain one-phase (fused claimed pixels); two-phase
NO_LISTS = 0x2000
NO_CLAIMS = 0x800
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
# (samples per pixel, early stop, samples per pass, world, rank): 64; 100 (ragged chunks: a wave straddles two pixels, no
# fused pass); 128 in two passes of 64; 3600 with early stop on a quarter of the frame (the plane is reused by passes over
# shrinking pixel lists); one stripe call
CASES = [(64, False, 0, 1, 0), (100, False, 0, 1, 0), (128, False, 64, 1, 0), (3600, True, 0, 1, 0), (64, False, 0, 2, 1)]
CASE_IDS = ["64", "100", "128x2", "3600es", "stripe"]


class Loaded:
    def __init__(self, name):
        (pos, nrm, uv), self.cam_desc = SCENES[name][0]()
        self.name, self.pos, self.size = name, pos, SCENES[name][1]
        self.gpu = va.Scene(pos, nrm, uv, device=0)
        self.cpu = O.OracleScene(pos, nrm, uv)
        self.refs = {}

    def camera(self, spp):
        W, H = self.size
        if spp > 1024:
            W, H = W // 2, H // 2
        return va.make_camera(self.cam_desc["position"], self.cam_desc["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))

    def reference(self, case):
        """the oracle's frame of a case, rendered once, shared and never written to"""
        if case not in self.refs:
            spp, es, _, world, rank = case
            img, st = self.cpu.render(self.camera(spp), va.make_opts(seed=4, early_stop=es, world=world, rank=rank))
            img.setflags(write=False)
            self.refs[case] = (img, st)
        return self.refs[case]

    def settled(self, spp, **kw):
        self.gpu.render(self.camera(spp), va.make_opts(seed=4, early_stop=False, **kw))
        return self.gpu.list_settled_rays()


@pytest.fixture(scope="module", params=list(SCENES))
def loaded(request):
    s = Loaded(request.param)
    yield s
    s.gpu.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_frames_and_counts_with_and_without_lists(loaded, case):
    spp, es, batch, world, rank = case
    cam = loaded.camera(spp)
    ref, rst = loaded.reference(case)
    for form in FORMS:
        out = []
        for off in (0, NO_LISTS):
            opts = va.make_opts(seed=4, early_stop=es, pipeline=form | off, samples_per_batch=batch, world=world, rank=rank)
            img, st = loaded.gpu.render(cam, opts)
            out.append((img, st, loaded.gpu.timings()["other"]["launches"], loaded.gpu.list_settled_rays()))
        (a, sa, la, na), (b, sb, lb, nb) = out
        assert np.array_equal(bits(a), bits(b)), (hex(form), "lists on / off differ")
        assert np.array_equal(bits(a), bits(ref)), (hex(form), "frame differs from the oracle's")
        for k in COUNT_KEYS:
            assert sa[k] == sb[k], (hex(form), k)
        for stage in ("primary", "bounce"):
            for k in STAGE_KEYS:
                assert sa[stage][k] == sb[stage][k], (hex(form), stage, k)
        assert sa["samples"] == rst["samples"]
        assert la == lb == 1, (hex(form), la, lb)  # still one launch under `other`: the claim kernel fills both planes
        print("form %s: %d of %d camera rays settled by a list" % (hex(form), na, sa["rays_primary"]))
        assert nb == 0
        assert na < sa["rays_primary"]
        if loaded.name != "soup":
            assert na > 0, hex(form)


def test_device_plane_is_the_host_programs(loaded):
    tree = loaded.gpu.bvh()
    cam = loaded.camera(64)
    hclaims, hlists, _, _ = LS.host_lists(loaded.pos, tree, [cam])[0]
    claims, lists, n = loaded.gpu.pixel_claim_lists(cam, va.make_opts(seed=4))
    assert np.array_equal(claims, hclaims) and n == int(np.sum(hclaims != LS.NONE))
    assert np.array_equal(lists, hlists)
    # the single-claim entry is what it was
    only, n0 = loaded.gpu.pixel_claims(cam, va.make_opts(seed=4))
    assert np.array_equal(only, hclaims) and n0 == n
    print("%d of %d pixels with a list" % (int(np.sum(LS.list_lengths(hlists) > 0)), hclaims.size))
    rows = va.local_row_indices(cam.image_res[1], 16, 1, 2)
    c1, l1, n1 = loaded.gpu.pixel_claim_lists(cam, va.make_opts(seed=4, world=2, rank=1))
    assert np.array_equal(c1, hclaims[rows]) and np.array_equal(l1, hlists[rows]) and n1 == int(np.sum(hclaims[rows] != LS.NONE))


def test_the_settled_count_in_the_other_forms(loaded):
    if loaded.name != "soup":
        for form in FORMS:
            assert loaded.settled(64, pipeline=form) > 0
    for form in FORMS:
        assert loaded.settled(64, pipeline=form | NO_LISTS) == 0
        assert loaded.settled(64, pipeline=form | NO_CLAIMS) == 0
        assert loaded.settled(16, pipeline=form) == 0                       # below the claims' sample threshold: no planes
        assert loaded.settled(64, pipeline=form, collect_counters=True) == 0  # the counting build traces every ray
    # a frame of this size in form 0 runs in the fused kernel: no split pass, no claims
    assert loaded.settled(64) == 0
    # the live list of ELIDE_DEAD takes neither claims nor lists
    assert loaded.settled(64, pipeline=4, sampling=va.VMX_SAMPLING_ELIDE_DEAD) == 0
