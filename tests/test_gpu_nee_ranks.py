"""Light sampling across ranks and devices, and on device batches, on the device: vmx_render_nee_rank*,
vmx_progressive_begin_nee_rank, vmx_multi_render_nee* and vmx_radiance_nee_device against tests/nee_spec.py, bit for bit.

A rank's expected rows are the rows vmx_local_rows names, taken from the whole spec frame (N.frame through
test_gpu_nee.spec_frame, whose cache the two files share).  For the rank handle the whole 48 x 32 x 16 spec frame would take
a quarter of a minute on the host, so its reference is the spec's radiance of sample k of the rank's own pixels — N.radiance
on the streams (seed, GLOBAL pixel, k), 576 pixels — folded as tests/sampling_spec.py folds; that this fold of N.radiance is
N.frame is test_gpu_nee_progressive.test_the_frame_from_the_shared_samples_is_nee_specs_frame.  Budgets are
tests/budget_spec.py's on the rank's local state and local image shape, uint32 for uint32."""
import functools

import numpy as np
import pytest

import budget_spec as BS
import nee_cases as K
import nee_spec as N
import oracle_lib as O
import sampling_spec as SS
import vermilion_amd as va
from test_gpu_nee import bits, camera, device_scene, same, spec_frame, spec_radiance
from test_gpu_nee_progressive import Spec, budgets_of, state
from vermilion_amd import dist as vdist
from vermilion_amd import scene as vscene

pytestmark = pytest.mark.gpu
F = np.float32
SEED = 5
COUNTS = ("rays_primary", "rays_secondary", "samples")


def rows_of(H, stripe, rank, world):
    rows = vscene.local_row_indices(H, stripe, rank, world)
    assert len(rows) == va.local_rows(H, stripe, rank, world)
    return rows


def zeroed(st):
    """a vmx_stats in which every count and every time is 0"""
    return all(zeroed(v) if isinstance(v, dict) else v == 0 for v in st.values())


def rank_device(sc, cam, opts, stream=None):
    """render_nee_rank_device into a tensor pre-filled with -7 that is one row longer than the rank's share: (rows, stats);
    the spare row must stay as it was"""
    import torch
    W = cam.image_res[0]
    n = va.local_rows(cam.image_res[1], opts.stripe_rows, opts.rank, opts.world)
    out = torch.full((n + 1, W, 5), -7.0, dtype=torch.float32, device="cuda")
    st = sc.render_nee_rank_device(cam, opts, out.data_ptr(), stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == -7).all()
    return got[:n], st


# ---- rank frames ---------------------------------------------------------------------------------------------------------------
def test_three_ranks_of_a_frame():
    """cornell8 48 x 32 x 8, stripes of 4 rows, world 3: the ranks own 3, 3 and 2 stripes"""
    W, H, spp, stripe, world = 48, 32, 8, 4, 3
    want, wst = spec_frame("cornell8", "default", 0, W, H, spp, SEED)
    cam = camera("cornell8", W, H, spp)
    tot = dict.fromkeys(COUNTS, 0)
    with device_scene("cornell8", "default", 0) as sc:
        for rank in range(world):
            opts = K.opts(SEED, rank=rank, world=world, stripe_rows=stripe)
            rows = rows_of(H, stripe, rank, world)
            assert len(rows) == (12, 12, 8)[rank]
            got, st = sc.render_nee_rank(cam, opts)
            assert got.shape == (len(rows), W, 5)
            same(got, want[rows], "rank %d" % rank)
            dgot, dst = rank_device(sc, cam, opts)
            same(dgot, want[rows], "rank %d, device form" % rank)
            assert st["samples"] == len(rows) * W * spp and all(st[k] == dst[k] for k in COUNTS)
            for k in COUNTS:
                tot[k] += st[k]
        assert all(tot[k] == wst[k] for k in COUNTS)
        # world 0 and 1: the whole frame
        for world1 in (0, 1):
            got, st = sc.render_nee_rank(cam, K.opts(SEED, rank=0, world=world1, stripe_rows=stripe))
            same(got, want, "world %d" % world1)
            assert all(st[k] == wst[k] for k in COUNTS)


@pytest.mark.parametrize("table,channels,batch", [("default", 0, 0), ("default", 0, 1), ("three", 3, 0)])
def test_ranks_of_a_small_odd_frame(table, channels, batch):
    """cornell8 37 x 5 x 4, stripes of 2 rows: the last stripe is a single row and the width is no multiple of 64.  World 2,
    and world 8, whose ranks 3 .. 7 own no row; samples_per_batch = 1 (a pass per sample); a 3-channel texture"""
    import torch
    W, H, spp, stripe = 37, 5, 4, 2
    want, wst = spec_frame("cornell8", table, channels, W, H, spp, SEED)
    cam = camera("cornell8", W, H, spp)
    with device_scene("cornell8", table, channels) as sc:
        for world in (2, 8):
            tot = dict.fromkeys(COUNTS, 0)
            seen = []
            for rank in range(world):
                opts = K.opts(SEED, rank=rank, world=world, stripe_rows=stripe, samples_per_batch=batch)
                rows = rows_of(H, stripe, rank, world)
                got, st = sc.render_nee_rank(cam, opts)
                dgot, dst = rank_device(sc, cam, opts, torch.cuda.Stream() if rank == 1 else None)
                assert got.shape == dgot.shape == (len(rows), W, 5)
                if len(rows):
                    same(got, want[rows], "world %d rank %d" % (world, rank))
                    same(dgot, want[rows], "world %d rank %d, device form" % (world, rank))
                    assert st["passes"] == dst["passes"] == (spp if batch else 1)
                else:  # no row: VMX_OK, nothing launched or written, the statistics zeroed
                    assert rank >= 3 and zeroed(st) and zeroed(dst)
                seen.extend(rows.tolist())
                for k in COUNTS:
                    tot[k] += st[k]
                    assert st[k] == dst[k]
            assert sorted(seen) == list(range(H)) and all(tot[k] == wst[k] for k in COUNTS)
        assert [len(rows_of(H, stripe, r, 2)) for r in range(2)] == [3, 2]


def test_two_rank_renders_assembled_on_the_host():
    """the process-per-GPU helper's render (dist.render_nee_local) for both ranks of a world of 2 on one device, assembled with
    assemble_host: the whole frame"""
    W, H, spp, stripe = 48, 32, 8, 4
    want, _ = spec_frame("cornell8", "default", 0, W, H, spp, SEED)
    cam = camera("cornell8", W, H, spp)
    with device_scene("cornell8", "default", 0) as sc:
        parts = [vdist.render_nee_local(sc, cam, K.opts(SEED, rank=r, world=2, stripe_rows=stripe))[0].cpu().numpy() for r in range(2)]
        whole, _ = sc.render_nee(cam, K.opts(SEED))
        none, st = vdist.render_nee_local(sc, cam, K.opts(SEED, rank=9, world=10, stripe_rows=stripe))
        assert tuple(none.shape) == (0, W, 5) and zeroed(st)
    frame = vdist.assemble_host(parts, W, H, stripe, 2)
    same(frame, whole, "against render_nee")
    same(frame, want, "against the spec")


# ---- rank handles --------------------------------------------------------------------------------------------------------------
HW, HH, HSPP, HSTRIPE, HWORLD, HRANK = 48, 32, 16, 4, 3, 1


class RankSpec(Spec):
    """test_gpu_nee_progressive.Spec for the packed rows of one rank: samples [kmax, rows, W, 4] of the rank's pixels, each on
    the streams of its GLOBAL pixel index; sums() and frame() then work in the rank's local shape"""

    def __init__(self, scene, table, W, H, spp, stripe, rank, world):
        pos, nrm, uv, _, _, _ = K.golden(scene)
        self.tb, self.tex = K.table(table), None
        self.osc = O.OracleScene(pos, nrm, uv, spheres=self.tb)
        self.cam, self.opts = camera(scene, W, H, spp), K.opts(SEED)
        rows = rows_of(H, stripe, rank, world)
        self.W, self.H, self.kmax = W, len(rows), 4 * (spp // 4)
        pix = (rows[:, None] * W + np.arange(W)[None, :]).reshape(-1).astype(np.int64)
        self.samples = np.empty((self.kmax, self.H, W, 4), F)
        self.stats = []
        for k in range(self.kmax):
            o, d = O.primary_rays(self.cam, self.opts, k)
            s, st = N.radiance(self.osc, o[pix], d[pix], SEED, self.tb, self.opts.sampling, True, None, pix, np.full(pix.size, k, np.int64))
            self.samples[k] = s.reshape(self.H, W, 4)
            self.stats.append(st)
        self.samples.setflags(write=False)


@functools.lru_cache(maxsize=None)
def rank_spec():
    return RankSpec("cornell8", "default", HW, HH, HSPP, HSTRIPE, HRANK, HWORLD)


def rank_opts(**kw):
    return K.opts(SEED, rank=HRANK, world=HWORLD, stripe_rows=HSTRIPE, **kw)


def test_a_rank_handle_in_steps_of_four():
    sp = rank_spec()
    kmax, npix = sp.kmax, sp.W * sp.H
    assert (sp.H, kmax) == (12, 16)
    with device_scene("cornell8", "default", 0) as sc:
        one, ost = sc.render_nee_rank(sp.cam, rank_opts())
        same(one, sp.frame(kmax), "render_nee_rank")
        assert all(ost[k] == sp.total(k) for k in COUNTS)
        with sc.progressive_nee(sp.cam, rank_opts(), moments=True, rank=True) as p:
            assert p.shape == (sp.H, sp.W)
            info = p.info()
            assert (info["width"], info["rows"], info["kmax"], info["pixels_active"]) == (sp.W, sp.H, kmax, npix)
            tot = dict.fromkeys(COUNTS, 0)
            for done in (4, 8, 12, 16):
                st = p.step(4)
                assert st["samples"] == 4 * npix
                for k in COUNTS:
                    tot[k] += st[k]
                sums, counts = state(p)
                assert (counts == done).all()
                same(sums, sp.sums(counts), "sums and m2 at %d" % done)
                same(p.preview(), sp.frame(done), "preview at %d" % done)
            assert p.info()["pixels_active"] == 0 and all(tot[k] == sp.total(k) for k in COUNTS)
            same(p.preview(), one, "the completed handle")
        # the plain begin still refuses a rank of a world; the rank form takes a whole image too
        with pytest.raises(va.VmxError, match="world > 1 is not supported"):
            sc.progressive_nee(sp.cam, rank_opts())


def threshold_with_a_mixed_plane(sp, counts, kmax, min_samples, radius):
    """a threshold, chosen on the CPU spec's state, at which the budget plane of that state holds zeros and non-zeros"""
    sums = sp.sums(counts)
    e, _ = SS.error_variance(sums, counts, BS.DEFAULTS["floor"])
    for q in (0.5, 0.75, 0.9, 0.97):
        thr = float(np.quantile(e[np.isfinite(e)], q))
        b = BS.budget(sums, counts, kmax, kmax, thr, BS.DEFAULTS["floor"], min_samples, radius, 0)
        if thr > 0 and (b == 0).any() and (b != 0).any():
            return thr
    raise AssertionError("no quantile of the spec's errors gives a plane with zeros and non-zeros")


def test_a_rank_handle_budgets_and_a_mixed_schedule():
    """one uniform step, one adaptive step, budgeted steps until nothing is selected, plain steps to the end: the rank's rows
    of the spec's frame; along the way budget_device's plane is budget_spec's on the rank's local state and shape"""
    sp = rank_spec()
    kmax, npix = sp.kmax, sp.W * sp.H
    first = np.full((sp.H, sp.W), 4, np.int64)
    thr = threshold_with_a_mixed_plane(sp, first, kmax, 4, 1)
    kw = dict(threshold=thr, min_samples=4, radius=1)
    bprm, sprm = va.make_sampling_budget_params(**kw), va.make_sampling_params(**kw)
    with device_scene("cornell8", "default", 0) as sc, sc.progressive_nee(sp.cam, rank_opts(), moments=True, rank=True) as p:
        p.step(4)
        sums, counts = state(p)
        same(sums, sp.sums(first), "state after the uniform step")
        # the budget plane used: the restatement fed the LOCAL state and shape, with zeros and non-zeros
        got, total = budgets_of(p, bprm)
        want = BS.budget(sums, counts, kmax, kmax, **dict(BS.DEFAULTS, **kw))
        assert got.shape == (sp.H, sp.W) and np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
        assert total == int(want.sum(dtype=np.int64))
        assert (want == 0).any() and (want != 0).any()
        assert np.array_equal(got != 0, SS.select(sums, counts, kmax, **kw) == 1)
        # the window stops at the rank's own rows: local rows 3 and 4 are global rows 7 and 16, no neighbours
        wide = BS.budget(sums, counts, kmax, kmax, **dict(BS.DEFAULTS, **dict(kw, radius=3)))
        got3, _ = budgets_of(p, va.make_sampling_budget_params(**dict(kw, radius=3)))
        assert np.array_equal(got3, wide)
        # one adaptive step
        sel = SS.select(sums, counts, kmax, **kw)
        st, nsel = p.step_adaptive(2, sprm)
        n = counts.astype(np.int64) + 2 * (sel == 1)
        assert nsel == int(sel.sum()) and 0 < nsel < npix and st["samples"] == 2 * nsel
        # budgeted steps until nothing is selected
        steps = 0
        while True:
            sums, counts = state(p)
            assert np.array_equal(counts, n)
            same(sums, sp.sums(n), "state before budgeted step %d" % steps)
            want = BS.budget(sums, counts, kmax, kmax, **dict(BS.DEFAULTS, **kw))
            got, _ = budgets_of(p, bprm)
            assert np.array_equal(got, want), steps
            st, nsel = p.step_budgeted(bprm)
            take = BS.step_counts(counts, want, kmax, kmax)
            assert nsel == int((take > 0).sum()) and st["samples"] == int(take.sum())
            if nsel == 0:
                break
            n = n + take
            steps += 1
            assert steps <= 32
        assert steps >= 1 and len(np.unique(n)) >= 2
        same(p.preview(), sp.frame(n), "preview of the ragged handle")
        # plain steps to the end
        while p.info()["pixels_active"]:
            p.step(3)
            n = np.minimum(n + 3, kmax)
            assert np.array_equal(state(p)[1], n)
        same(p.preview(), sp.frame(kmax), "complete: the rank's rows of the spec's frame")
        same(p.preview(), sc.render_nee_rank(sp.cam, rank_opts())[0], "render_nee_rank")


# ---- device lists --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0, 0], [0]], ids=["three", "one"])
@pytest.mark.parametrize("scene,W,H,spp", [("cornell8", 48, 32, 8), ("lattice", 40, 24, 4)])
def test_multi_render_nee(scene, W, H, spp, devices):
    import torch
    want, wst = spec_frame(scene, "default", 0, W, H, spp, SEED)
    cam = camera(scene, W, H, spp)
    pos, nrm, uv, _, _, _ = K.golden(scene)
    opts = K.opts(SEED, stripe_rows=4)
    with device_scene(scene, "default", 0) as one, va.MultiScene(pos, nrm, uv, spheres=K.table("default"), devices=devices) as multi:
        ref, rst = one.render_nee(cam, opts)
        got, st = multi.render_nee(cam, opts)
        same(got, ref, "against Scene.render_nee")
        same(got, want, "against the spec")
        assert all(st[k] == rst[k] == wst[k] for k in COUNTS)  # summed over the replicas
        tm = multi.timings()
        assert tm["world"] == len(devices) and all(t > 0 for t in tm["render_ms"]) and tm["assemble_ms"] > 0
        out = torch.full((H, W, 5), -7.0, dtype=torch.float32, device="cuda")
        dst = multi.render_nee_device(cam, opts, out.data_ptr())
        torch.cuda.synchronize()
        same(out.cpu().numpy(), want, "device form")
        assert all(dst[k] == wst[k] for k in COUNTS)
        with pytest.raises(va.VmxError, match="world > 1 is not supported"):
            multi.render_nee(cam, K.opts(SEED, world=2, rank=1))


@pytest.mark.parametrize("channels", [0, 3], ids=["set_spheres", "set_spheres_and_bind_texture"])
def test_multi_render_nee_follows_the_replicas_state(channels):
    """after set_spheres with another emitter count (and after bind_texture) every replica renders the new state"""
    W, H, spp = 48, 32, 8
    want, wst = spec_frame("cornell8", "three", channels, W, H, spp, SEED)
    cam, opts = camera("cornell8", W, H, spp), K.opts(SEED, stripe_rows=4)
    pos, nrm, uv, _, _, _ = K.golden("cornell8")
    with va.MultiScene(pos, nrm, uv, spheres=K.table("default"), devices=[0, 0, 0]) as multi:
        first, _ = multi.render_nee(cam, opts)
        multi.set_spheres(K.table("three"))
        if channels:
            multi.bind_texture(K.texture(channels))
        got, st = multi.render_nee(cam, opts)
        with device_scene("cornell8", "three", channels) as one:
            ref, rst = one.render_nee(cam, opts)
        same(got, ref, "against Scene.render_nee")
        same(got, want, "against the spec")
        assert all(st[k] == rst[k] == wst[k] for k in COUNTS)
        assert not np.array_equal(bits(got), bits(first))


def test_multi_render_nee_after_an_update():
    """vmx_multi_update moves the block on every replica: the frame of one scene updated the same way"""
    pos, nrm, uv, _, _, _ = K.golden("cornell8")
    cam, opts = camera("cornell8", 37, 5, 4), K.opts(SEED, stripe_rows=2)
    moved = pos.copy().reshape(-1, 3, 3)
    moved[4:] += np.float32([64.0, 32.0, -16.0])
    moved = moved.reshape(-1, 9)
    with va.Scene(pos, nrm, uv) as one, va.MultiScene(pos, nrm, uv, devices=[0, 0]) as multi:
        one.update(pos=moved), multi.update(pos=moved)
        ref, rst = one.render_nee(cam, opts)
        got, st = multi.render_nee(cam, opts)
        same(got, ref, "after update")
        assert all(st[k] == rst[k] for k in COUNTS)
        same(one.render_nee(cam, opts)[0], ref, "the scene again")


# ---- device batches ------------------------------------------------------------------------------------------------------------
def test_radiance_nee_device():
    """the golden cornell8 rays, n = 1, 63, 65 and all 1536: radiance_nee's answer and the spec's; once on a caller's side
    stream into a tensor pre-filled with -7; n = 0"""
    import torch
    _, _, _, o, d, _ = K.golden("cornell8")
    want, wst = spec_radiance("cornell8", "default", 0, K.CORRECTED, 7)
    opts = K.opts(7)
    with device_scene("cornell8", "default", 0) as sc:
        d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        for n in (1, 63, 65, len(o)):
            host, hst = sc.radiance_nee(o[:n], d[:n], opts)
            out = torch.full((n + 1, 4), -7.0, dtype=torch.float32, device="cuda")
            side = torch.cuda.Stream() if n == 65 else None
            if side is not None:
                side.wait_stream(torch.cuda.current_stream())
            st = sc.radiance_nee_device(d_o.data_ptr(), d_d.data_ptr(), n, opts, out.data_ptr(), side.cuda_stream if side else None)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            same(got[:n], host, "n = %d against radiance_nee" % n)
            same(got[:n], want[:n], "n = %d against the spec" % n)
            assert (got[n:] == -7).all()
            assert st["samples"] == n and all(st[k] == hst[k] for k in COUNTS)
        assert st["rays_primary"] == wst["rays_primary"] and st["rays_secondary"] == wst["rays_secondary"]
        out = torch.full((4, 4), -7.0, dtype=torch.float32, device="cuda")
        assert sc.radiance_nee_device(d_o.data_ptr(), d_d.data_ptr(), 0, opts, out.data_ptr())["samples"] == 0
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7).all()
        # the pointer kinds and the overlap are refused before anything is launched
        lib = sc._lib
        import ctypes as C
        hostbuf = np.zeros((8, 4), np.float32)
        hp = (hostbuf.ctypes.data + 15) & ~15
        for args, word in (((hp, d_d.data_ptr(), out.data_ptr()), "origin is not device memory"),
                           ((d_o.data_ptr(), hp, out.data_ptr()), "dir is not device memory"),
                           ((d_o.data_ptr(), d_d.data_ptr(), hp), "d_out4 is not device memory"),
                           ((d_o.data_ptr(), d_d.data_ptr(), d_o.data_ptr()), "d_out4 overlaps the rays")):
            rc = lib.vmx_radiance_nee_device(sc._h, C.c_void_p(args[0]), C.c_void_p(args[1]), 1, C.byref(opts), C.c_void_p(args[2]), None, None)
            assert rc == va._lib.VMX_ERR_INVALID and word in lib.vmx_last_error().decode(), (word, lib.vmx_last_error())
        same(sc.radiance_nee(o[:65], d[:65], opts)[0], want[:65], "the scene still works")


# ---- the C++ host ----------------------------------------------------------------------------------------------------------------
def test_cpp_host_multi_device_light_sampling(tmp_path):
    """examples/render_multi --nee: the picture does not depend on the device list and is render_nee's, quantised"""
    import os
    import subprocess
    from vermilion_amd import scenes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "render_multi")
    out1, out3 = tmp_path / "a.ppm", tmp_path / "b.ppm"
    subprocess.run([exe, str(out1), "48", "32", "8", "5", "0", "--nee"], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "--nee", str(out3), "48", "32", "8", "5", "0,0,0"], check=True, capture_output=True, text=True)
    assert out1.read_bytes() == out3.read_bytes() and "3 device(s), light sampling" in r.stdout
    pos, nrm, uv = scenes.cornell8()
    c = scenes.cornell_camera()
    # the sensor's height as the example forms it, in float32: 3.6f * H / W is one ulp below float32(2.4), and a light-sampled
    # path — unlike the nearly always black paths of the reference's sampling — carries an ulp of its camera ray into the picture
    height = np.float32(np.float32(3.6) * np.float32(32)) / np.float32(48)
    cam = va.make_camera(c["position"], c["rotation_deg"], 48, 32, 8, back_size=(3.6, float(height)))
    with va.Scene(pos, nrm, uv) as sc:
        ref, _ = sc.render_nee(cam, K.opts(5))
    want = np.floor(ref[:, :, :3] * np.float32(255.0)).astype(np.uint8).tobytes()
    assert out3.read_bytes()[len(b"P6\n48 32\n255\n"):] == want
