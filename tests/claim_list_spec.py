"""Shared by test_claim_lists.py (CPU) and test_gpu_claim_lists.py: the stand-alone host program of the list claims of
vermilion_amd/csrc/pixel_claim.h (tests/cpp/pixel_claim_list_test.cpp), built once per session, and the oracle's verdict
on what the per-ray rule settles."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

import pixel_claim_spec as S

NONE, MISS, ROOT = S.NONE, S.MISS, S.ROOT
WORDS = 4  # kListWords = kListK: four slots
_exe = {}


def host_program(sanitize=False, why=False):
    """path of the built program (g++, the library's own flags for the arithmetic: no FMA contraction)"""
    key = (sanitize, why)
    if key not in _exe:
        if shutil.which("g++") is None:
            import pytest
            pytest.skip("no g++")
        d = tempfile.mkdtemp(prefix="pixel_claim_list_")
        exe = os.path.join(d, "pixel_claim_list_test")
        csrc = os.path.join(ROOT, "vermilion_amd", "csrc")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else (["-O2", "-DVMX_PC_DIAG"] if why else ["-O2"])
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "pixel_claim_list_test.cpp"), os.path.join(csrc, "bvh_build.cpp"),
                        "-o", exe], check=True)
        _exe[key] = exe
    return _exe[key]


def host_lists(pos, tree, cams, rays=None, sanitize=False, why=False):
    """Per camera (single claims [H, W], list records [H, W, WORDS], settled slot [n] (NONE: the ray walks), t [n]) over
    the flat tree `tree` of the triangles pos.  rays: per camera (pixel [n] uint32, direction [n, 3] float32) or None."""
    import oracle_lib as O
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    d = tempfile.mkdtemp(prefix="pixel_claim_list_io_")
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    try:
        with open(fin, "wb") as f:
            f.write(np.array([pos.shape[0], len(tree["start"]), len(cams)], np.uint32).tobytes())
            f.write(pos.tobytes())
            for k in ("start", "nprims", "right_offset"):
                f.write(np.ascontiguousarray(tree[k], np.uint32).tobytes())
            f.write(np.ascontiguousarray(tree["bbox"], np.float32).tobytes())
            f.write(np.ascontiguousarray(tree["prim_order"], np.uint32).tobytes())
            for i, cam in enumerate(cams):
                f.write(np.ascontiguousarray(O.camera_matrix(cam), np.float32).tobytes())  # [col][row]
                f.write(np.array(list(cam.position), np.float32).tobytes())
                f.write(np.array([cam.back_size[0], cam.back_size[1], cam.back_distance], np.float32).tobytes())
                f.write(np.array([cam.image_res[0], cam.image_res[1]], np.uint32).tobytes())
                pix, dirs = (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32)) if rays is None else rays[i]
                rec = np.zeros(len(pix), np.dtype([("p", np.uint32), ("d", np.float32, 3)]))
                rec["p"], rec["d"] = pix, dirs
                f.write(np.array([len(pix)], np.uint32).tobytes())
                f.write(rec.tobytes())
        subprocess.run([host_program(sanitize, why), fin, fout], check=True)
        raw = np.fromfile(fout, np.uint32)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out, at = [], 0
    for i, cam in enumerate(cams):
        W, H = cam.image_res[0], cam.image_res[1]
        n = 0 if rays is None else len(rays[i][0])
        claims = raw[at:at + W * H].reshape(H, W).copy()
        at += W * H
        lists = raw[at:at + W * H * WORDS].reshape(H, W, WORDS).copy()
        at += W * H * WORDS
        res = raw[at:at + 2 * n].reshape(n, 2)
        at += 2 * n
        out.append((claims, lists, res[:, 0].copy(), res[:, 1].copy().view(np.float32)))
    assert at == raw.size
    return out


def list_lengths(lists):
    """members per pixel [H * W]"""
    return np.sum(lists.reshape(-1, WORDS)!= NONE, axis=1)


def sample_rays(cam, pixels, spp, seed, footprint=True):
    """(pixel, direction) of the samples k < spp of `pixels` and, footprint, of the nine points of their sample footprint"""
    import oracle_lib as O
    import vermilion_amd as va
    opts = va.make_opts(seed=seed)
    pix, dirs = [], []
    for k in range(spp):
        _, d = O.primary_rays(cam, opts, k)
        pix.append(pixels), dirs.append(d[pixels])
    if footprint and pixels.size:
        for d in S.footprint_directions(cam, pixels):
            pix.append(pixels), dirs.append(np.asarray(d, np.float32))
    if not pix:
        return np.zeros(0, np.uint32), np.zeros((0, 3), np.float32)
    return np.concatenate(pix).astype(np.uint32), np.ascontiguousarray(np.concatenate(dirs), np.float32)


def verdict(osc, tree, cam, pix, dirs, slot, t):
    """(rays the rule settled wrongly, rays it settled): a settled ray must carry the oracle's triangle and the bits of its t"""
    settled = slot != NONE
    if not settled.any():
        return 0, 0
    o = np.repeat(np.array(list(cam.position), np.float32)[None, :], int(settled.sum()), axis=0)
    tri, rt = osc.trace(o, dirs[settled])
    want = np.asarray(tree["prim_order"])[np.minimum(slot[settled], len(tree["prim_order"]) - 1)].astype(np.int64)
    bad = (tri != want) | (rt.view(np.uint32) != t[settled].view(np.uint32))
    return int(bad.sum()), int(settled.sum())
