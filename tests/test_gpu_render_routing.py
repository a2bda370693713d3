"""Which kernels a call runs: per form of the render host loop, the passes, the launch count, the per-kernel launches of
Scene.timings() and the route counters (fused camera paths, list-settled rays, guide rays) of one call on cornell8 at
32 x 24 with seed 3, compared with literals.

The literals were recorded by this file's recorder (`python tests/test_gpu_render_routing.py`) on a build of the commit
BEFORE the host loop was cut by form, on an MI355X with and without VMX_CU_LIMIT = 3 (profiles/render_routing.txt keeps
the record).  The two outputs were identical, so no count depends on the number of compute units and every count is
compared as recorded."""
import json

import pytest

import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

W, H, SEED = 32, 24, 3
ONE_PHASE, KEEP_ENDS, NO_CLAIMS, NO_FUSE, NO_LISTS, NO_GUIDE = 0x100, 0x200, 0x800, 0x1000, 0x2000, 0x4000
CORRECTED, ELIDE = L.VMX_SAMPLING_CORRECTED, L.VMX_SAMPLING_ELIDE_DEAD


def _camera(spp):
    c = scenes.cornell_camera()
    return va.make_camera(c["position"], c["rotation_deg"], W, H, spp)


def _render(spp, **kw):
    kw.setdefault("early_stop", False)
    return lambda sc: sc.render(_camera(spp), va.make_opts(seed=SEED, **kw))[1]


def _render_nee(sc):
    return sc.render_nee(_camera(16), va.make_opts(seed=SEED, early_stop=False, sampling=CORRECTED))[1]


def _bruteforce(sc):
    return sc.render_bruteforce(_camera(16), va.make_opts(seed=SEED, early_stop=False))[1]


def _radiance(sc):
    opts = va.make_opts(seed=SEED, early_stop=False, tail_threshold=1)
    o, d = O.primary_rays(_camera(16), opts, 0)
    assert len(o) == 768
    return sc.radiance(o, d, opts)[1]


CASES = [("default 16", _render(16)),
         ("pipeline 1, 16", _render(16, pipeline=1)),
         ("pipeline 4, 64", _render(64, pipeline=4))]
CASES += [("pipeline 4, 64, bit %d" % b, _render(64, pipeline=4 | (1 << b))) for b in (8, 9, 11, 12, 13, 14)]
CASES += [("pipeline 4, 64, tail_threshold 1", _render(64, pipeline=4, tail_threshold=1)),
          ("pipeline 4, 16, elide dead", _render(16, pipeline=4, sampling=ELIDE)),
          ("pipeline 4, 64, early stop", _render(64, pipeline=4, early_stop=True)),
          ("pipeline 4, 64, counters", _render(64, pipeline=4, collect_counters=True)),
          ("render_nee 16", _render_nee),
          ("render_bruteforce 16", _bruteforce),
          ("radiance 768, tail_threshold 1", _radiance)]
assert (ONE_PHASE, KEEP_ENDS, NO_CLAIMS, NO_FUSE, NO_LISTS, NO_GUIDE) == tuple(1 << b for b in (8, 9, 11, 12, 13, 14))


def route(sc, run):
    """what one call ran: a fresh dict of plain ints"""
    st = run(sc)
    launches = {k: int(v["launches"]) for k, v in sc.timings().items() if v["launches"]}
    return {"passes": int(st["passes"]), "kernel_launches": int(st["kernel_launches"]), "launches": launches,
            "fused_camera_paths": sc.fused_camera_paths(), "list_settled_rays": sc.list_settled_rays(),
            "guide_rays": list(sc.guide_rays())}


def record():
    pos, nrm, uv = scenes.cornell8()
    out = {}
    for name, run in CASES:
        with va.Scene(pos, nrm, uv) as sc:  # a scene per case: no workspace of an earlier form
            out[name] = route(sc, run)
    return out


# the recorder's output on the parent build (see the docstring); "launches" lists the kernels that ran at all
EXPECTED = {
    "default 16": {"passes": 1, "kernel_launches": 5, "launches": {"fused": 1, "resolve": 1}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
    "pipeline 1, 16": {"passes": 1, "kernel_launches": 4, "launches": {"fused": 1, "resolve": 1}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
    "pipeline 4, 64": {"passes": 1, "kernel_launches": 10, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "tail": 1, "resolve": 1, "other": 1}, "fused_camera_paths": 0, "list_settled_rays": 9510, "guide_rays": [0, 0]},
    "pipeline 4, 64, bit 8": {"passes": 1, "kernel_launches": 16, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "tail": 1, "resolve": 1, "other": 1}, "fused_camera_paths": 30464, "list_settled_rays": 9510, "guide_rays": [0, 0]},
    "pipeline 4, 64, bit 9": {"passes": 1, "kernel_launches": 10, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "tail": 1, "resolve": 1, "other": 1}, "fused_camera_paths": 0, "list_settled_rays": 9510, "guide_rays": [0, 0]},
    "pipeline 4, 64, bit 11": {"passes": 1, "kernel_launches": 9, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "tail": 1, "resolve": 1}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
    "pipeline 4, 64, bit 12": {"passes": 1, "kernel_launches": 10, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "tail": 1, "resolve": 1, "other": 1}, "fused_camera_paths": 0, "list_settled_rays": 9510, "guide_rays": [0, 0]},
    "pipeline 4, 64, bit 13": {"passes": 1, "kernel_launches": 10, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "tail": 1, "resolve": 1, "other": 1}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
    "pipeline 4, 64, bit 14": {"passes": 1, "kernel_launches": 10, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "tail": 1, "resolve": 1, "other": 1}, "fused_camera_paths": 0, "list_settled_rays": 9510, "guide_rays": [0, 0]},
    "pipeline 4, 64, tail_threshold 1": {"passes": 1, "kernel_launches": 35, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "trace_bounce": 5, "shade_bounce": 5, "tail": 1, "resolve": 1, "other": 1}, "fused_camera_paths": 0, "list_settled_rays": 9510, "guide_rays": [6955, 0]},
    "pipeline 4, 16, elide dead": {"passes": 1, "kernel_launches": 9, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "tail": 1, "resolve": 1}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
    "pipeline 4, 64, early stop": {"passes": 2, "kernel_launches": 16, "launches": {"raygen": 2, "trace_camera": 2, "shade_camera": 2, "tail": 2, "resolve": 2}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
    "pipeline 4, 64, counters": {"passes": 1, "kernel_launches": 9, "launches": {"raygen": 1, "trace_camera": 1, "shade_camera": 1, "tail": 1, "resolve": 1}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
    "render_nee 16": {"passes": 1, "kernel_launches": 3, "launches": {"resolve": 1, "other": 1}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
    "render_bruteforce 16": {"passes": 2, "kernel_launches": 1, "launches": {"bruteforce": 2}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
    "radiance 768, tail_threshold 1": {"passes": 1, "kernel_launches": 16, "launches": {"trace_bounce": 3, "shade_bounce": 3, "tail": 1}, "fused_camera_paths": 0, "list_settled_rays": 0, "guide_rays": [0, 0]},
}


@pytest.fixture(scope="module")
def cornell():
    return scenes.cornell8()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_a_call_runs_the_recorded_kernels(cornell, name):
    with va.Scene(*cornell) as sc:
        got = route(sc, dict(CASES)[name])
    assert got == EXPECTED[name], (name, got)


def test_every_form_has_a_record():
    assert sorted(EXPECTED) == sorted(n for n, _ in CASES)
    for name, want in EXPECTED.items():
        assert want["passes"] >= 1 and want["kernel_launches"] >= 1 and want["launches"], name
    # the switches do switch: what each bit turns off is on beside it and off under the bit
    one_phase = EXPECTED["pipeline 4, 64, bit 8"]  # (claimed pixels are fused where the camera pass is the plain one-phase form)
    assert one_phase["fused_camera_paths"] > 0 and EXPECTED["pipeline 4, 64"]["fused_camera_paths"] == 0
    assert EXPECTED["pipeline 4, 64"]["list_settled_rays"] > 0
    assert EXPECTED["pipeline 4, 64, bit 11"]["list_settled_rays"] == EXPECTED["pipeline 4, 64, bit 13"]["list_settled_rays"] == 0
    assert sum(EXPECTED["pipeline 4, 64, tail_threshold 1"]["guide_rays"]) > 0  # (bounce generations before the tail)
    assert EXPECTED["pipeline 4, 64, bit 14"]["guide_rays"] == [0, 0]

if __name__ == "__main__":
    for name, got in record().items():
        print("    %s: %s," % (json.dumps(name), json.dumps(got)))
