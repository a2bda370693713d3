"""Progressive rendering (vmx_progressive_*): a frame rendered in any number of steps is vmx_render's and the oracle's,
bit for bit; previews of the unfinished state obey the conditions an unfinished frame can be held to; the handle's
frames do not depend on what else the scene serves between its steps.

Shapes: the 8-triangle Cornell set at 70x41 (2,870 pixels: the last wave of every pixel list is partial) at 16 and 64
spp (quarter 4 / 16, nmin 4 / 8: the early-stop lead pass exists at 64 spp with an allowance of 12 or more and is cut
by a smaller one), and the lattice at 64x48x16 for bounce generations that are not empty."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 70, 41
ELIDE = va.VMX_SAMPLING_ELIDE_DEAD


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cornell_cam(spp, w=W, h=H):
    c = scenes.cornell_camera()
    return va.make_camera(c["position"], c["rotation_deg"], w, h, spp)


@pytest.fixture(scope="module")
def sc():
    with va.Scene(*scenes.cornell8()) as s:
        yield s


@pytest.fixture(scope="module")
def oracle():
    """oracle frames of the Cornell set, computed once per (camera, options) and never written to"""
    osc = O.OracleScene(*scenes.cornell8())
    cache = {}

    def render(spp, w=W, h=H, **kw):
        key = (spp, w, h, tuple(sorted(kw.items())))
        if key not in cache:
            img, st = osc.render(cornell_cam(spp, w, h), va.make_opts(**kw))
            img.setflags(write=False)
            cache[key] = (img, st)
        return cache[key]

    yield render
    osc.close()


def run(scene, cam, opts, samples, each=None):
    """steps of `samples` until the frame is complete; returns the final preview, the summed per-step stats, the info"""
    total = dict(rays_primary=0, rays_secondary=0, samples=0, passes=0)
    with scene.progressive(cam, opts) as p:
        kmax = p.info()["kmax"]
        for _ in range(kmax + 1):
            if p.info()["pixels_active"] == 0:
                break
            st = p.step(samples)
            for k in total:
                total[k] += st[k]
            if each:
                each(p)
        info = p.info()
        assert info["pixels_active"] == 0, "not complete after kmax steps: some step gave an active pixel no sample"
        assert p.step(samples)["samples"] == 0 and p.info() == info  # a step of a complete frame does nothing
        return p.preview(), total, info


@pytest.mark.parametrize("sampling", [va.VMX_SAMPLING_PARITY, va.VMX_SAMPLING_CORRECTED, ELIDE], ids=["parity", "corrected", "elide"])
@pytest.mark.parametrize("early_stop", [0, 1])
@pytest.mark.parametrize("spp", [16, 64])
def test_final_frame_is_the_oracles_whatever_the_steps(sc, oracle, spp, early_stop, sampling):
    """Every step size in {1, 3, 5, 7, kmax, 0}, in the default routing and with every pass fused (1) or split (4).
    Ray counters: the oracle's when every ray is traced; under VMX_SAMPLING_ELIDE_DEAD the counters hold the traced rays
    only (include/vermilion_hip.h), which the oracle does not model, so there the sums are held to the one-call
    render's counters (whether a ray is elided depends on its path's draws and the ray alone, not on the pass)."""
    cam = cornell_cam(spp)
    ref, ost = oracle(spp, seed=11, early_stop=bool(early_stop), sampling=sampling)
    kmax = 4 * (spp // 4)
    for pipeline in (0, 1, 4):
        opts = va.make_opts(seed=11, early_stop=bool(early_stop), sampling=sampling, pipeline=pipeline)
        one, rst = sc.render(cam, opts)
        assert np.array_equal(bits(one), bits(ref)), pipeline
        for samples in (1, 3, 5, 7, kmax, 0):
            img, tot, info = run(sc, cam, opts, samples)
            tag = (pipeline, samples)
            assert np.array_equal(bits(img), bits(ref)), (tag, int((bits(img) != bits(ref)).any(axis=2).sum()))
            assert tot["samples"] == ost["samples"] == info["samples"], tag
            assert info["passes"] == tot["passes"] and info["width"] == W and info["rows"] == H and info["kmax"] == kmax
            if samples == 0:
                assert info["steps"] == 1
            if not early_stop:
                want = rst if sampling & ELIDE else ost
                assert tot["rays_primary"] == want["rays_primary"] and tot["rays_secondary"] == want["rays_secondary"], tag
                assert info["steps"] == (1 if samples == 0 else -(-kmax // samples)), tag


def test_lattice_frames_with_live_bounce_generations():
    pos, nrm, uv = scenes.lattice()
    c = scenes.lattice_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 64, 48, 16)
    osc = O.OracleScene(pos, nrm, uv)
    with va.Scene(pos, nrm, uv) as s:
        for early_stop in (False, True):
            ref, ost = osc.render(cam, va.make_opts(seed=5, early_stop=early_stop))
            assert ost["rays_secondary"] > 0
            for pipeline in (0, 4):
                opts = va.make_opts(seed=5, early_stop=early_stop, pipeline=pipeline)
                for samples in (3, 7, 0):
                    img, tot, _ = run(s, cam, opts, samples)
                    assert np.array_equal(bits(img), bits(ref)), (early_stop, pipeline, samples)
                    assert tot["samples"] == ost["samples"]
                    if not early_stop:
                        assert tot["rays_primary"] == ost["rays_primary"] and tot["rays_secondary"] == ost["rays_secondary"]
    osc.close()


@pytest.mark.parametrize("spp", [16, 64])
def test_stripes_of_one_rank(sc, oracle, spp):
    sub = dict(world=3, rank=1, stripe_rows=4)
    rows = va.local_rows(H, 4, 1, 3)
    for early_stop in (False, True):
        ref, ost = oracle(spp, seed=4, early_stop=early_stop, **sub)
        assert ref.shape == (rows, W, 5)
        for samples in (5, 0):
            img, tot, info = run(sc, cornell_cam(spp), va.make_opts(seed=4, early_stop=early_stop, **sub), samples)
            assert info["rows"] == rows and img.shape == ref.shape
            assert np.array_equal(bits(img), bits(ref)), (early_stop, samples)
            assert tot["samples"] == ost["samples"]


@pytest.mark.parametrize("early_stop", [0, 1])
@pytest.mark.parametrize("spp", [16, 64])
def test_intermediate_frames(sc, oracle, spp, early_stop):
    """The oracle renders whole frames only (sample keys and strata depend on the total spp), so a prefix of a pixel's
    samples has no reference: these are the conditions every intermediate frame must meet.  A pixel is finished exactly
    when its depth has reached the final frame's: an active pixel takes at least one sample in every step."""
    import torch
    cam = cornell_cam(spp)
    ref, _ = oracle(spp, seed=9, early_stop=bool(early_stop))
    final_depth = ref[:, :, 4]
    opts = va.make_opts(seed=9, early_stop=bool(early_stop))
    empty = np.tile(np.float32([0, 0, 0, 1, 0]), (H, W, 1))
    for samples in (3, 5):
        with sc.progressive(cam, opts) as p:
            prev, q = p.preview(rgba8=True)
            assert np.array_equal(bits(prev), bits(empty)) and np.array_equal(q.reshape(-1, 4), O.quantize(prev)[0])
            assert p.info()["pixels_active"] == W * H and p.info()["steps"] == 0
            for step in range(4 * (spp // 4)):
                active = prev[:, :, 4] != final_depth
                if not active.any():
                    break
                p.step(samples)
                cur, q = p.preview(rgba8=True)
                again = p.preview()
                assert np.array_equal(bits(cur), bits(again))  # a preview changes nothing
                rise = cur[:, :, 4] - prev[:, :, 4]
                assert rise[active].min() >= 1 and rise[active].max() <= samples, (samples, step)
                assert np.array_equal(bits(cur[~active]), bits(prev[~active]))   # a finished pixel never changes again
                assert np.array_equal(bits(cur[~active]), bits(ref[~active]))    # ... and is the final frame's
                assert (cur[:, :, 3] == 1).all() and (cur[:, :, :3] >= 0).all() and (cur[:, :, :3] <= 1).all()
                assert np.array_equal(q.reshape(-1, 4), O.quantize(cur)[0])
                assert p.info()["pixels_active"] == int((cur[:, :, 4] != final_depth).sum())
                if step == 1:
                    # the device entry writes the same bytes, both outputs or either one alone
                    d5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
                    d4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
                    e5, e4 = torch.empty_like(d5), torch.empty_like(d4)
                    torch.cuda.synchronize()
                    p.preview_device(d5, d4)
                    p.preview_device(rgbaz=e5)
                    p.preview_device(rgba8=e4)
                    p.preview()  # (the host entry synchronises the handle's stream)
                    for t5 in (d5, e5):
                        assert np.array_equal(bits(t5.cpu().numpy()), bits(cur))
                    for t4 in (d4, e4):
                        assert np.array_equal(t4.cpu().numpy(), q)
                prev = cur
            assert np.array_equal(bits(prev), bits(ref))
    # steps of 2 and 3 leave the state one step of 5 leaves
    with sc.progressive(cam, opts) as a, sc.progressive(cam, opts) as b:
        a.step(2), a.step(3), b.step(5)
        pa, pb = a.preview(), b.preview()
        assert np.array_equal(bits(pa), bits(pb)) and (pa[:, :, 4] == 5).all()
        assert a.info()["samples"] == b.info()["samples"] == 5 * W * H


def test_interleaving_with_other_work_on_the_scene(sc, oracle):
    import torch
    cam = cornell_cam(64)
    other = cornell_cam(16, 33, 17)
    other.position[0] = 150.0  # another origin: the shared camera tables are rewritten between the handle's steps
    oa = va.make_opts(seed=21, early_stop=True)
    ob = va.make_opts(seed=22, early_stop=False, pipeline=4)
    ref_a, _ = oracle(64, seed=21, early_stop=True)
    ref_b, _ = oracle(64, seed=22, early_stop=False)
    ref_other, _ = sc.render(other, va.make_opts(seed=3))
    rng = np.random.RandomState(1)
    o = rng.uniform((-500, 50, 100), (500, 800, 1500), (257, 3)).astype(np.float32)
    d = np.tile(np.float32([0, -0.6, -0.8]), (257, 1))
    want_q = sc.query(o, d)
    want_g = sc.raycast_camera(cam, oa, 0)["raw"].cpu().numpy()
    with sc.progressive(cam, oa) as a, sc.progressive(cam, ob) as b:
        for step in range(64):
            if a.info()["pixels_active"] == 0 and b.info()["pixels_active"] == 0:
                break
            a.step(4 if step % 2 else 12)  # (12: the lead pass fits)
            img, _ = sc.render(other, va.make_opts(seed=3))
            assert np.array_equal(bits(img), bits(ref_other))
            pa = a.preview()
            got = sc.query(o, d)
            assert all(np.array_equal(x, y) for x, y in zip(got, want_q))
            b.step(5)
            assert np.array_equal(bits(a.preview()), bits(pa))  # the other handle's step left this one alone
            b.preview()
            g = sc.raycast_camera(cam, oa, 0)["raw"].cpu().numpy()
            assert np.array_equal(bits(g), bits(want_g))
        assert a.info()["pixels_active"] == 0 and b.info()["pixels_active"] == 0
        assert np.array_equal(bits(a.preview()), bits(ref_a))
        assert np.array_equal(bits(b.preview()), bits(ref_b))


def test_refusals():
    pos, nrm, uv = scenes.cornell8()
    cam = cornell_cam(16)
    opts = va.make_opts(seed=2)
    s = va.Scene(pos, nrm, uv)
    p = s.progressive(cam, opts)
    p.step(2)
    before = p.preview()
    s.update(pos=pos)  # a refit to the same positions is still an update
    with pytest.raises(va.VmxError, match="scene updated since vmx_progressive_begin") as e:
        p.step(2)
    assert e.value.code == L.VMX_ERR_INVALID
    with pytest.raises(va.VmxError, match="scene updated since vmx_progressive_begin"):
        p.step(0)
    assert np.array_equal(bits(p.preview()), bits(before)) and p.info()["steps"] == 1
    # a handle begun after the update works, next to the refused one
    q = s.progressive(cam, opts)
    q.step(0)
    assert np.array_equal(bits(q.preview()), bits(s.render(cam, opts)[0]))
    q.close()
    with pytest.raises(va.VmxError, match="open vmx_progressive") as e:
        s.close()
    assert e.value.code == L.VMX_ERR_INVALID
    assert s.describe()["ntris"] == 8  # the scene is intact
    p.close()
    p.close()  # (idempotent)
    s.close()
    assert s._h is None


def test_cpp_host_steps_through_the_c_abi(sc, tmp_path):
    """examples/render_progressive.cpp: steps of 4 samples through the C ABI alone; its last frame is Scene.render's"""
    exe = os.path.join(ROOT, "examples", "render_progressive")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    ppm, raw = tmp_path / "p.ppm", tmp_path / "p.f32"
    r = subprocess.run([exe, str(ppm), "70", "41", "64", "5", "4", str(raw)], capture_output=True, text=True, check=True)
    c = scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 70, 41, 64, back_size=(3.6, np.float32(3.6) * np.float32(41) / np.float32(70)))
    ref, rst = sc.render(cam, va.make_opts(seed=5))
    got = np.fromfile(raw, np.float32).reshape(41, 70, 5)
    assert np.array_equal(bits(got), bits(ref))
    head = b"P6\n70 41\n255\n"
    data = ppm.read_bytes()
    assert data[:len(head)] == head and data[len(head):] == O.quantize(ref)[0][:, :3].tobytes()
    lines = [l for l in r.stdout.splitlines() if l.startswith("step ")]
    active = [int(l.split("pixels_active ")[1].split(",")[0]) for l in lines]
    assert len(lines) >= 2 and active[-1] == 0 and all(x >= y for x, y in zip(active, active[1:]))
    assert f"samples {rst['samples']}," in r.stdout.splitlines()[-1]
