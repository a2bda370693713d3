"""tests/nee_mesh_spec.py itself, without a device: it is nee_spec where there is no table, its derived table is the exact one
on integer coordinates, and its estimator is unbiased — the light-sampled mean agrees with the mean of the same paths with
sampling off (override on: emitters are found by chance), case by case."""
import math

import numpy as np
import pytest

import nee_cases as K
import nee_mesh_cases as MC
import nee_mesh_spec as M
import nee_spec as N
import oracle_lib as O

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- pins ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["default", "overlap"])
@pytest.mark.parametrize("scene", ["cornell8", "lattice"])
def test_without_a_table_it_is_nee_spec(scene, table):
    pos, nrm, uv, o, d, _ = K.golden(scene)
    tb = K.table(table)
    osc = O.OracleScene(pos, nrm, uv, spheres=tb)
    for light_sampling in (True, False):
        want, wst = N.radiance(osc, o, d, 7, tb, K.CORRECTED, light_sampling)
        got, st = M.radiance(osc, o, d, 7, tb, K.CORRECTED, light_sampling)
        assert np.array_equal(bits(got), bits(want)) and st == wst, (scene, table, light_sampling)
        empty = M.table(pos, [], np.zeros((0, 3), F))
        again, _ = M.radiance(osc, o, d, 7, tb, K.CORRECTED, light_sampling, emitters=empty)
        assert np.array_equal(bits(again), bits(want))
    osc.close()


def test_the_table_on_integer_coordinates():
    """the lattice's coordinates are small integers: edges and cross products are exact in int64, so area = 0.5 sqrt(nn) with
    one correctly rounded square root, the weight one product and the cdf one addition each — computed here with Python
    integers and floats, not with the spec's arrays"""
    pos = K.golden("lattice")[0]
    assert (pos == np.round(pos)).all()
    ids, rad = MC.lattice_table(65)
    t = M.table(pos, ids, rad)
    run = 0.0
    for e, tri in enumerate(ids):
        p = [int(v) for v in pos[tri]]
        a = [p[3 + i] - p[i] for i in range(3)]
        b = [p[6 + i] - p[i] for i in range(3)]
        n = (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])
        nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
        assert nn < 2 ** 53
        area = 0.5 * math.sqrt(nn)
        lum = F(F(F(0.2126) * rad[e, 0]) + F(F(0.7152) * rad[e, 1])) + F(F(0.0722) * rad[e, 2])
        weight = area * float(F(lum))
        run = run + weight
        assert (t["area"][e], t["weight"][e], t["cdf"][e]) == (area, weight, run), e
        assert np.allclose(t["normal"][e], np.array(n, np.float64) / math.sqrt(nn), rtol=1e-15, atol=0)
        assert t["id_em"][tri] == e
    assert t["weight"][1] == 0.0 and t["cdf"][1] == t["cdf"][0] and (t["id_em"] >= 0).sum() == 65
    # a triangle collapsed to a point has area 0 and weight 0
    moved = MC.case("lattice_65")["moved"]
    assert M.table(moved, ids, rad)["area"][2] == 0.0 and M.table(moved, ids, rad)["weight"][2] == 0.0


def test_selection_is_the_smallest_index_above_u():
    """the search the area sample uses against a plain scan, flat stretches (zero weights) and the clamp included"""
    cdf = np.array([0.0, 2.0, 2.0, 2.0, 5.0, 5.0, 9.0])
    for u in (0.0, 1.9999, 2.0, 4.0, 5.0, 8.9999, 9.0, 10.0):
        want = next((e for e in range(len(cdf)) if cdf[e] > u), len(cdf) - 1)
        assert min(int(np.searchsorted(cdf, u, side="right")), len(cdf) - 1) == want, u


# ---- unbiasedness ----------------------------------------------------------------------------------------------------------
# Paths per case: the case's 1536 golden camera rays, each REPEATS times on its own stream.  Chosen so that the brute-force
# side's standard error is under 1 % of its mean in every channel (measured: 0.81 - 0.88 % for the quad cases at 73,728
# paths, 0.90 % for block_top at 270,336); the test asserts that it is.
REPEATS = {"quad_none": 48, "quad_single": 48, "quad_overlap": 48, "block_top": 176}


@pytest.mark.parametrize("name", MC.LIT)
def test_light_sampling_is_unbiased(name):
    c = MC.case(name)
    tb = K.table(c["spheres"])
    osc = O.OracleScene(c["pos"], c["nrm"], c["uv"], spheres=tb)
    et = M.table(c["pos"], c["ids"], c["radiance"])
    r = REPEATS[name]
    o, d = np.tile(c["o"], (r, 1)), np.tile(c["d"], (r, 1))
    n = len(o)
    nee, st = M.radiance(osc, o, d, 11, tb, emitters=et)
    brute, _ = M.radiance(osc, o, d, 12, tb, light_sampling=False, emitters=et)
    osc.close()
    a, b = nee[:, :3].astype(np.float64), brute[:, :3].astype(np.float64)
    assert np.isfinite(a).all() and np.isfinite(b).all() and st["rays_shadow"] > 0
    va_, vb = a.var(0, ddof=1), b.var(0, ddof=1)
    se = np.sqrt(va_ / n + vb / n)
    z = (a.mean(0) - b.mean(0)) / se
    print("unbiasedness %s: %d paths, mean nee %s brute %s, per-path variance nee %s brute %s, z %s" %
          (name, n, a.mean(0), b.mean(0), va_, vb, z))
    assert (np.sqrt(vb / n) < 0.01 * b.mean(0)).all(), "the brute-force side is not settled: more paths"
    assert (np.abs(z) <= 4.0).all(), (name, z)
