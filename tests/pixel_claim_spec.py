"""Shared by test_pixel_claims.py (CPU) and test_gpu_pixel_claims.py: the stand-alone host program of
vermilion_amd/csrc/pixel_claim.h (tests/cpp/pixel_claim_test.cpp), built once per session, and the oracle's verdict on
a claim table."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

NONE = 0xFFFFFFFF
MISS = 0xFFFFFFFE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_exe = None


def host_program():
    """path of the built program (g++, the library's own flags for the arithmetic: no FMA contraction)"""
    global _exe
    if _exe is None:
        if shutil.which("g++") is None:
            import pytest
            pytest.skip("no g++")
        d = tempfile.mkdtemp(prefix="pixel_claim_")
        exe = os.path.join(d, "pixel_claim_test")
        csrc = os.path.join(ROOT, "vermilion_amd", "csrc")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "pixel_claim_test.cpp"), os.path.join(csrc, "bvh_build.cpp"),
                        "-o", exe], check=True)
        _exe = exe
    return _exe


def host_claims(pos, tree, cams):
    """claim tables [H, W] (uint32) of the cameras (vmx_camera descriptors) over the flat tree `tree` (Scene.bvh() /
    OracleScene.bvh()) of the triangles pos [ntris, 9]"""
    import oracle_lib as O
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    d = tempfile.mkdtemp(prefix="pixel_claim_io_")
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    try:
        with open(fin, "wb") as f:
            n_nodes = len(tree["start"])
            f.write(np.array([pos.shape[0], n_nodes, len(cams)], np.uint32).tobytes())
            f.write(pos.tobytes())
            for k in ("start", "nprims", "right_offset"):
                f.write(np.ascontiguousarray(tree[k], np.uint32).tobytes())
            f.write(np.ascontiguousarray(tree["bbox"], np.float32).tobytes())
            f.write(np.ascontiguousarray(tree["prim_order"], np.uint32).tobytes())
            for cam in cams:
                f.write(np.ascontiguousarray(O.camera_matrix(cam), np.float32).tobytes())  # [col][row]
                f.write(np.array(list(cam.position), np.float32).tobytes())
                f.write(np.array([cam.back_size[0], cam.back_size[1], cam.back_distance], np.float32).tobytes())
                f.write(np.array([cam.image_res[0], cam.image_res[1]], np.uint32).tobytes())
        subprocess.run([host_program(), fin, fout], check=True)
        raw = np.fromfile(fout, np.uint32)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out, at = [], 0
    for cam in cams:
        W, H = cam.image_res[0], cam.image_res[1]
        out.append(raw[at:at + W * H].reshape(H, W).copy())
        at += W * H
    assert at == raw.size
    return out


def footprint_directions(cam, q):
    """corners, edge midpoints and centre of the sample footprint of the pixels q: offsets [-0.75, 0.25]"""
    import oracle_lib as O
    from test_pixel_sphere_bounds import footprint_directions as fd
    M = O.camera_matrix(cam).T
    W, H = cam.image_res[0], cam.image_res[1]
    return fd(M, None, (cam.back_size[0], cam.back_size[1]), cam.back_distance, W, H, q)


def oracle_verdict(osc, tree, cam, claims, spp=64, seed=3, only_claimed=False):
    """Traces every sample k < spp of every claimed pixel and the nine footprint points with the oracle.
    Returns (rays whose triangle differs from the slot claim, hits on MISS pixels, oracle's own share of one-triangle
    pixels, of all-miss pixels): the shares over ALL pixels, from the same spp samples — or, only_claimed, over the
    claimed pixels, the only ones then traced."""
    import oracle_lib as O
    import vermilion_amd as va
    W, H = cam.image_res[0], cam.image_res[1]
    flat = claims.reshape(-1)
    order = np.asarray(tree["prim_order"])
    want = np.where(flat < MISS, order[np.minimum(flat, order.size - 1)].astype(np.int64), -1)  # triangle id per pixel
    claimed = np.flatnonzero(flat != NONE)
    bad_slot = bad_miss = 0
    first = None
    same = np.ones(W * H, bool)
    opts = va.make_opts(seed=seed)
    pos = np.repeat(np.array(list(cam.position), np.float32)[None, :], W * H, axis=0)
    sel = claimed if only_claimed else np.arange(W * H)
    for k in range(spp):
        o, d = O.primary_rays(cam, opts, k)
        tri = np.full(W * H, -2, np.int32)
        if sel.size:
            tri[sel] = osc.trace(o[sel], d[sel])[0]
        if first is None:
            first = tri.copy()
        same &= tri == first
        bad_slot += int(np.sum((flat < MISS) & (tri != want)))
        bad_miss += int(np.sum((flat == MISS) & (tri != -1)))
    if claimed.size:
        for d in footprint_directions(cam, claimed):
            tri, _ = osc.trace(pos[claimed], d)
            bad_slot += int(np.sum((flat[claimed] < MISS) & (tri != want[claimed])))
            bad_miss += int(np.sum((flat[claimed] == MISS) & (tri != -1)))
    one = float(np.mean((same & (first >= 0))[sel])) if sel.size else 0.0
    miss = float(np.mean((same & (first == -1))[sel])) if sel.size else 0.0
    return bad_slot, bad_miss, one, miss
