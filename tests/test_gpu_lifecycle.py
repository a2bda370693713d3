"""Handles of every kind, made, used and destroyed three times in one process: what a handle owns goes with it, in an
order in which nothing is freed twice, freed while work still uses it, or outlived by something that points into it.
Not a leak test: free-memory readings are device-wide and other processes share the device."""
import numpy as np
import pytest

import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def one_cycle():
    """name -> host array of everything one cycle computes.  The wrappers raise VmxError on any return code other than
    VMX_OK, so a cycle that returns had VMX_OK from every call but the one refusal it asks for."""
    import torch
    out = {}
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(11)
    c = scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 32, 32, 16)
    opts = va.make_opts(seed=5, early_stop=False)
    pos, nrm, uv = scenes.cornell8()
    assert len(np.asarray(pos).reshape(-1, 9)) == 8
    sc = va.Scene(pos, nrm, uv)
    out["frame"], _ = sc.render(cam, opts)

    # a NEAREST query of 64 rays on the caller's own stream
    o = np.tile(np.float32(c["position"]), (64, 1))
    d = np.stack([rng.uniform(-0.4, 0.4, 64), rng.uniform(-0.3, 0.1, 64), -np.ones(64)], axis=1).astype(np.float32)
    side = torch.cuda.Stream(dev)
    o_t, d_t = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    tri, t, hit = sc.query(o_t, d_t, mode="nearest", stream=side)
    side.synchronize()
    out["query_tri"], out["query_t"], out["query_hit"] = tri.cpu().numpy(), t.cpu().numpy(), hit.cpu().numpy().view(np.uint8)
    assert out["query_hit"].any()

    raw = sc.raycast_camera(cam, opts, 0)["raw"]
    out["raycast"] = raw.cpu().numpy()

    # one iteration in place (the filter stages a copy of the frame in its planes), and the filter destroyed while
    # that call may still run
    frame_t = torch.from_numpy(out["frame"]).to(dev)
    f = va.Filter(32, 32)
    f.set_guide(raw)
    f.apply(frame_t, out=frame_t, params=va.make_filter_params(iterations=1))
    f.close()
    out["filtered"] = frame_t.cpu().numpy()
    assert not np.array_equal(bits(out["filtered"]), bits(out["frame"]))

    # a progressive handle that owns a filter when it ends; the scene refuses to go before it
    p = sc.progressive(cam, opts)
    p.step(4)
    out["preview_filtered"] = p.preview_filtered()
    with pytest.raises(va.VmxError, match="open vmx_progressive") as e:
        sc.close()
    assert e.value.code == L.VMX_ERR_INVALID
    assert sc.describe()["ntris"] == 8 and p.info()["steps"] == 1  # both are intact
    p.step(4)
    out["preview_after_refusal"] = p.preview()
    out["frame_after_refusal"], _ = sc.render(cam, opts)
    p.close()
    sc.close()

    # a REFIT on one stream, a query on another at once, then the scene destroyed
    pos, nrm, uv = scenes.lattice()
    pos = np.asarray(pos, np.float32).reshape(-1, 9)
    assert len(pos) == 200
    ls = va.Scene(pos, nrm, uv)
    moved = pos.copy()
    moved[:, 1::3] += np.float32(25.0) * (np.arange(200, dtype=np.float32)[:, None] % 3)
    lo = np.stack([rng.uniform(-850, 850, 64), np.full(64, 500.0), rng.uniform(-650, 650, 64)], axis=1).astype(np.float32)
    ld = np.stack([rng.uniform(-0.2, 0.2, 64), -np.ones(64), rng.uniform(-0.2, 0.2, 64)], axis=1).astype(np.float32)
    moved_t, lo_t, ld_t = (torch.from_numpy(a).to(dev) for a in (moved, lo, ld))
    s_update, s_query = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    s_update.wait_stream(torch.cuda.current_stream(dev))
    s_query.wait_stream(torch.cuda.current_stream(dev))
    ls.update(pos=moved_t, stream=s_update)
    tri, t, hit = ls.query(lo_t, ld_t, mode="nearest", stream=s_query)
    s_query.synchronize()
    out["refit_tri"], out["refit_t"], out["refit_hit"] = tri.cpu().numpy(), t.cpu().numpy(), hit.cpu().numpy().view(np.uint8)
    assert out["refit_hit"].any()
    s_update.synchronize()
    ls.close()
    return out


def test_handles_of_every_kind_three_times():
    first = one_cycle()
    assert np.array_equal(bits(first["frame_after_refusal"]), bits(first["frame"]))
    for cycle in (2, 3):
        again = one_cycle()
        assert again.keys() == first.keys()
        for name in first:
            assert np.array_equal(bits(again[name]), bits(first[name])), (cycle, name)
