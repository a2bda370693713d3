"""Per-pixel claims in the split passes (pixel_claim.h, k_pixel_claims, the refill path of k_trace_w<0>): frames are
bit-identical with claims on and off (vmx_opts.reserved[0] bit 11) and identical to the oracle's, the counts of vmx_stats
do not change, the device's claim table is the host program's, and a frame below the sample threshold builds none."""
import os

import numpy as np
import pytest

import oracle_lib as O
import pixel_claim_spec as S
import vermilion_amd as va
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NO_CLAIMS = 0x800
FORMS = [4, 4 | 0x100, 4 | 0x200]  # sorted camera rays (k_trace_w<0, .., SORT>), one-phase, two-phase through k_shade_ends


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
# (samples per pixel, early stop, samples per pass, world, rank): 64; 100 (ragged chunks: a wave straddles two pixels);
# 256 with early stop (most pixels take 20 samples: below the threshold, no table); 3600 with early stop, on a quarter
# of the frame (64 samples before the rule can fire: a table is built and every later pass reuses it — shrinking
# compacted pixel lists, speculative samples, padded sample slots); 128 in two passes of 64; one stripe call
CASES = [(64, False, 0, 1, 0), (100, False, 0, 1, 0), (256, True, 0, 1, 0), (3600, True, 0, 1, 0), (128, False, 64, 1, 0),
         (64, False, 0, 2, 1)]
COUNT_KEYS = ("rays_primary", "rays_secondary", "samples", "samples_discarded", "passes")
STAGE_KEYS = ("rays", "inner_visits", "tri_tests", "tri_hits", "continued")


class Loaded:
    def __init__(self, name):
        (pos, nrm, uv), self.cam_desc = SCENES[name][0]()
        self.pos = pos
        self.size = SCENES[name][1]
        self.gpu = va.Scene(pos, nrm, uv, device=0)
        self.cpu = O.OracleScene(pos, nrm, uv)
        self.refs = {}

    def camera(self, spp):
        W, H = self.size
        if spp > 1024:
            W, H = W // 2, H // 2
        return va.make_camera(self.cam_desc["position"], self.cam_desc["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))

    def reference(self, case):
        """the oracle's frame of a case, rendered once and shared by the forms"""
        if case not in self.refs:
            spp, es, _, world, rank = case
            self.refs[case] = self.cpu.render(self.camera(spp), va.make_opts(seed=4, early_stop=es, world=world, rank=rank))
        return self.refs[case]


@pytest.fixture(scope="module", params=list(SCENES))
def loaded(request):
    s = Loaded(request.param)
    yield s
    s.gpu.close()


@pytest.mark.parametrize("case", CASES, ids=["64", "100", "256es", "3600es", "128x2", "stripe"])
def test_frames_and_counts_with_and_without_claims(loaded, case):
    spp, es, batch, world, rank = case
    cam = loaded.camera(spp)
    ref, rst = loaded.reference(case)
    for form in FORMS:
        out = []
        for off in (0, NO_CLAIMS):
            opts = va.make_opts(seed=4, early_stop=es, pipeline=form | off, samples_per_batch=batch, world=world, rank=rank)
            img, st = loaded.gpu.render(cam, opts)
            out.append((img, st, loaded.gpu.timings()["other"]["launches"]))
        (a, sa, la), (b, sb, lb) = out
        assert np.array_equal(bits(a), bits(b)), (hex(form), "claims on / off differ")
        assert np.array_equal(bits(a), bits(ref)), (hex(form), "frame differs from the oracle's")
        for k in COUNT_KEYS:
            assert sa[k] == sb[k], (hex(form), k)
        for stage in ("primary", "bounce"):
            for k in STAGE_KEYS:
                assert sa[stage][k] == sb[stage][k], (hex(form), stage, k)
        assert sa["samples"] == rst["samples"]
        # one claim kernel per call where the samples most pixels take reach the threshold (early stop: floor(sqrt(spp))
        # + 1 and the first sample of the three later strata), none with the switch or below it
        expect = min(spp, int(spp ** 0.5) + 4) if es else spp
        assert lb == 0 and la == (1 if expect >= 64 else 0), (hex(form), la, lb)
        if case[0] == 3600:
            assert sa["passes"] > 1  # the table was reused by passes over shrunken pixel lists


def test_device_table_is_the_host_programs(loaded):
    tree = loaded.gpu.bvh()
    cam = loaded.camera(64)
    host = S.host_claims(loaded.pos, tree, [cam])[0]
    dev, n = loaded.gpu.pixel_claims(cam, va.make_opts(seed=4))
    assert np.array_equal(dev, host)
    assert n == int(np.sum(host != S.NONE))
    print("claimed %d of %d pixels" % (n, host.size))
    rows = va.local_row_indices(cam.image_res[1], 16, 1, 2)
    part, n1 = loaded.gpu.pixel_claims(cam, va.make_opts(seed=4, world=2, rank=1))
    assert np.array_equal(part, host[rows]) and n1 == int(np.sum(host[rows] != S.NONE))


def test_no_claim_kernel_below_the_sample_threshold(loaded):
    cam = loaded.camera(16)
    for form in FORMS:
        loaded.gpu.render(cam, va.make_opts(seed=4, early_stop=False, pipeline=form))
        assert loaded.gpu.timings()["other"]["launches"] == 0
    loaded.gpu.render(loaded.camera(64), va.make_opts(seed=4, early_stop=False, pipeline=4))
    assert loaded.gpu.timings()["other"]["launches"] == 1
    # form 0 runs a frame of this size in the fused kernel: no split pass, no claims
    loaded.gpu.render(loaded.camera(64), va.make_opts(seed=4, early_stop=False))
    assert loaded.gpu.timings()["other"]["launches"] == 0
