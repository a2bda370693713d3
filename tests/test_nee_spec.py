"""tests/nee_spec.py, the definition of light sampling (vmx_render_nee*, vmx_radiance_nee), without a GPU: pinned to the CPU
oracle where light sampling is off, unbiased against the oracle's `corrected` estimator where it is on, and the cone
arithmetic, the ownership rule's premise and the inside rule on their own."""
import numpy as np
import pytest

import nee_cases as K
import nee_spec as N
import oracle_lib as O
from vermilion_amd import _lib as L

LIBM = L.VMX_SAMPLING_LIBM_DOUBLE


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _oracle(scene, tb, tex):
    pos, nrm, uv, o, d, _ = K.golden(scene)
    osc = O.OracleScene(pos, nrm, uv, spheres=tb)
    if tex is not None:
        osc.bind_texture(tex)
    return osc, o, d


# ---- pinned to the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cornell8", "lattice"])
@pytest.mark.parametrize("channels", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("sampling", [K.CORRECTED, K.CORRECTED | LIBM])
def test_spec_without_light_sampling_is_the_oracles_corrected(scene, channels, sampling):
    """light_sampling=False: orc_radiance with VMX_SAMPLING_CORRECTED, bit for bit, on the golden camera rays — untextured and
    with a 1-4 channel texture (the lattice's uv leave [0, 1]: the wrap is exercised), both readings of cos / sin"""
    tex = K.texture(channels) if channels else None
    osc, o, d = _oracle(scene, None, tex)
    ref, rst = osc.radiance(o, d, K.opts(11, sampling))
    got, gst = N.radiance(osc, o, d, 11, None, sampling, light_sampling=False, tex=tex)
    assert np.array_equal(_bits(ref), _bits(got))
    assert gst["rays_primary"] == rst["rays_primary"] and gst["rays_secondary"] == rst["rays_secondary"]
    assert gst["rays_shadow"] == 0


@pytest.mark.parametrize("scene", ["cornell8", "lattice"])
def test_spec_with_no_emitter_is_the_oracles_corrected(scene):
    """a table without emitters: the emitter loop draws nothing and casts nothing, so light sampling changes no bit"""
    tb = K.table("none")
    osc, o, d = _oracle(scene, tb, None)
    ref, rst = osc.radiance(o, d, K.opts(12))
    got, gst = N.radiance(osc, o, d, 12, tb, K.CORRECTED, light_sampling=True)
    assert np.array_equal(_bits(ref), _bits(got))
    assert gst["rays_shadow"] == 0 and gst["rays_secondary"] == rst["rays_secondary"]


# ---- unbiased against the reference estimator ----------------------------------------------------------------------------
# every 7th golden camera ray of cornell8 (220 of them), repeated: path i runs on stream (seed, i, 0), so a repeat is a new
# path.  10^6 oracle paths put the reference's standard error below 1 % of its mean on every table (0.4 - 0.7 %); light
# sampling needs far fewer for a smaller one
REPEATS_REF, REPEATS_NEE, SEED = 4546, 100, 21
TABLES = {"default": ("default", 0), "single": ("single", 0), "overlap": ("overlap", 0), "default_textured": ("default", 3)}


@pytest.fixture(scope="module", params=sorted(TABLES))
def estimates(request):
    name, channels = TABLES[request.param]
    tb = K.table(name)
    tex = K.texture(channels) if channels else None
    osc, o, d = _oracle("cornell8", tb, tex)
    o7, d7 = o[::7], d[::7]
    oo, dd = np.tile(o7, (REPEATS_REF, 1)), np.tile(d7, (REPEATS_REF, 1))
    ref, _ = osc.radiance(oo, dd, K.opts(SEED))
    n = len(o7) * REPEATS_NEE
    nee, st = N.radiance(osc, oo[:n], dd[:n], SEED, tb, K.CORRECTED, light_sampling=True, tex=tex)
    return request.param, ref[:, :3].astype(np.float64), nee[:, :3].astype(np.float64), st


def test_light_sampling_has_the_reference_estimators_mean(estimates):
    """per channel |mean_ref - mean_nee| <= 4 sqrt(SE_ref^2 + SE_nee^2); the seeds are fixed, so the outcome is deterministic.
    Teeth: the reference's SE is at most 1 % of its mean, so a bias of a few per cent fails."""
    name, ref, nee, st = estimates
    mr, mn = ref.mean(0), nee.mean(0)
    ser, sen = ref.std(0, ddof=1) / np.sqrt(len(ref)), nee.std(0, ddof=1) / np.sqrt(len(nee))
    print(name, "ref", mr, "+-", ser, "nee", mn, "+-", sen, "shadow rays per path", st["rays_shadow"] / len(nee))
    assert (mr > 0).all() and (ser <= 0.01 * mr).all(), (name, ser / mr)
    assert (np.abs(mr - mn) <= 4.0 * np.sqrt(ser * ser + sen * sen)).all(), (name, mr, mn, ser, sen)


def test_light_sampling_lowers_the_variance(estimates):
    """the per-path sample variance, summed over rgb, is below `corrected`'s — which orders the variances of the two means
    at any equal path count.  The reference's is taken from all its paths: its variance is made by rare large samples, and
    a short run's estimate of it is the noisier one."""
    name, ref, nee, _ = estimates
    vr, vn = ref.var(0, ddof=1).sum(), nee.var(0, ddof=1).sum()
    print(name, "variance per path: corrected", vr, "light sampling", vn)
    assert vn < vr, (name, vr, vn)


# ---- the cone --------------------------------------------------------------------------------------------------------------
def test_cone_solid_angle_matches_extended_precision():
    """Omega = 2 pi s2 / (1 + sqrt(1 - s2)) in double against 2 pi (1 - sqrt(1 - s2)) in np.longdouble, relative difference
    <= 1e-12: light 1 (radius 3.5) from 2000, 500 and 140 units, light 2 (250) from 3500, a point one radius above a
    surface (D = 2 r) and one just outside (D = r (1 + 2^-10))"""
    assert np.finfo(np.longdouble).eps < 2e-19
    pairs = [(3.5, 2000.0), (3.5, 500.0), (3.5, 140.0), (250.0, 3500.0), (60.0, 120.0), (3.5, 7.0), (250.0, 250.0 * (1 + 2.0 ** -10))]
    r = np.float32([p[0] for p in pairs])
    D = np.float32([p[1] for p in pairs])
    rad2, C_ = (r * r).astype(np.float32), (D * D).astype(np.float32)
    q, omega = N.cone(rad2, C_)
    s2 = rad2.astype(np.longdouble) / C_.astype(np.longdouble)
    want = np.longdouble(2) * np.longdouble("3.14159265358979323846264338327950288") * (1 - np.sqrt(1 - s2))
    rel = np.abs(omega.astype(np.longdouble) - want) / want
    print("relative differences", rel.astype(np.float64))
    assert (rel <= 1e-12).all()


def test_sampled_directions_lie_in_their_emitters_cone():
    """every omega satisfies the ownership predicate of its own emitter, 0.5 |omega - a|^2 <= q, up to float32 rounding:
    omega and a are float32 unit vectors, each component within 8 float epsilons (three roundings of the normalisation, the
    float conversions of cos t / sin t, cosf / sinf: delta = 1e-6), so |omega - a| moves by at most delta and
    0.5 |omega - a|^2 by sqrt(2 q) delta + delta^2 / 2"""
    for name in ("default", "overlap"):
        tb = K.table(name)
        osc, o, d = _oracle("cornell8", tb, None)
        trace = {}
        N.radiance(osc, o[::3], d[::3], 31, tb, K.CORRECTED, light_sampling=True, trace=trace)
        n = 0
        for _, a, q, om, _, _ in trace["cone"]:
            e = om.astype(np.float64) - a.astype(np.float64)
            half = 0.5 * (e * e).sum(1)
            delta = 1e-6
            assert (half <= q + np.sqrt(2 * q) * delta + delta * delta).all()
            assert (np.abs(np.linalg.norm(om.astype(np.float64), axis=1) - 1) < 1e-6).all()
            n += len(q)
        assert n > 10000


# ---- the inside rule -------------------------------------------------------------------------------------------------------
def test_origin_inside_an_emitter_draws_nothing_and_is_not_lit():
    """64 rays that start inside an emitter and hit a triangle inside it: the step's new origin is inside, so the emitter
    loop consumes no draw — the stream stands where plain `corrected` leaves it after the step: the branch draw and the two
    of the diffuse arm, or the branch draw and the three unused ones of the specular arm — and lit stays false"""
    tb, o, d = K.inside_rays(64)
    pos, nrm, uv, _, _, _ = K.golden("cornell8")
    osc = O.OracleScene(pos, nrm, uv, spheres=tb)
    trace = {}
    got, st = N.radiance(osc, o, d, 41, tb, K.CORRECTED, light_sampling=True, trace=trace)
    ids, pos_after, lit = trace["inside"][0]  # the first step
    assert len(ids) >= 56  # (all 64 but the few that took the specular arm, 4 % each)
    assert (pos_after == 3).all() and not lit.any()
    # the same paths elsewhere in the room do draw: two per emitter
    tb2 = K.table("overlap")
    osc2 = O.OracleScene(pos, nrm, uv, spheres=tb2)
    trace2 = {}
    N.radiance(osc2, o, d, 41, tb2, K.CORRECTED, light_sampling=True, trace=trace2)
    assert len(trace2["inside"][0][0]) == 0 and len(trace2["cone"][0][2]) >= 56
    # not lit: the bounce ray, which starts inside the emitter, adds the emitter's colour when it reaches its shell
    assert (got[:, :3] == np.float32([1.5, 1.25, 1.0])).all(axis=1).sum() >= 56 and st["rays_shadow"] == 0
