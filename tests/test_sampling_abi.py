"""Adaptive sampling (vmx_progressive_begin_ex / state / step_selected / error / select / step_adaptive,
vmx_sampling_default_params) without a GPU: the symbols, the struct layout against the header, the defaults, the argument
checks that come before any device work — and the conditions the restatement itself (tests/sampling_spec.py, what the GPU
tests compare with) is held to on synthetic samples.  (The refusals by kind of handle need a handle, hence a device:
tests/test_gpu_sampling.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import sampling_spec as SS
import vermilion_amd as va
from vermilion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_progressive_begin_ex", "vmx_progressive_state_device", "vmx_progressive_step_selected_device",
           "vmx_sampling_default_params", "vmx_progressive_error_device", "vmx_progressive_select_device",
           "vmx_progressive_step_adaptive")
F = np.float32


def _err(lib):
    return lib.vmx_last_error().decode()


def test_sampling_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, re.S)
        assert decl, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")) == len(L.SYMBOLS[name][1]), name
    # additive: no new ABI version
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    assert re.search(r"#define VMX_PROGRESSIVE_MOMENTS 1u\b", src) and L.VMX_PROGRESSIVE_MOMENTS == 1
    assert "make_sampling_params" in va.__all__ and hasattr(va, "make_sampling_params")
    for name in ("state_device", "step_selected", "error_device", "select_device", "step_adaptive"):
        assert hasattr(va.Progressive, name), name


def test_sampling_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in L.SamplingParams._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vermilion_hip.h"\nint main(void){\n'
    prog += 'printf("size %zu\\n", sizeof(vmx_sampling_params));\n'
    for n in fields:
        prog += f'printf("{n} %zu\\n", offsetof(vmx_sampling_params, {n}));\n'
    prog += "return 0;}\n"
    src = tmp_path / "sz.c"
    src.write_text(prog)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.SamplingParams) == 32
    assert [int(out[n]) for n in fields] == [getattr(L.SamplingParams, n).offset for n in fields] == [0, 4, 8, 12, 16]


def test_default_params(hip_lib):
    p = L.SamplingParams(9.0, 9.0, 9, 9, (C.c_uint32 * 4)(1, 2, 3, 4))
    assert hip_lib.vmx_sampling_default_params(C.byref(p)) == L.VMX_OK
    d = SS.DEFAULTS
    assert (F(p.threshold), F(p.floor), p.min_samples, p.radius) == (F(d["threshold"]), F(d["floor"]), 8, 1)
    assert list(p.reserved) == [0, 0, 0, 0]
    # threshold and floor come from the measured grid (profiles/sampling_quality.txt), and the header states them
    assert F(p.threshold) in [F(x) for x in (0.25, 0.5, 1, 2)] and F(p.floor) in [F(x) for x in (0.01, 0.05, 0.2)]
    src = open(HEADER).read()
    m = re.search(r"Defaults \(vmx_sampling_default_params\): threshold ([0-9.]+)f, floor ([0-9.]+)f, min_samples 8, radius 1", src)
    assert m and F(m.group(1)) == F(p.threshold) and F(m.group(2)) == F(p.floor)
    assert hip_lib.vmx_sampling_default_params(None) == L.VMX_ERR_INVALID
    q = va.make_sampling_params(threshold=2, radius=3)
    assert (q.threshold, F(q.floor), q.min_samples, q.radius) == (2.0, F(d["floor"]), 8, 3)
    assert SS.params_of(va.make_sampling_params()) == {k: (F(v) if isinstance(v, float) else v) for k, v in d.items()}


def test_checks_do_not_need_a_gpu(hip_lib):
    """every refusal that comes before the handle is looked at, each seen alone: parameters first, then the pointers"""
    buf = np.zeros(64, np.float32)
    ptr = (buf.ctypes.data + 15) & ~15
    N = None

    def refused(fn, args, what):
        assert getattr(hip_lib, fn)(*args) == L.VMX_ERR_INVALID, (fn, what)
        assert what in _err(hip_lib), (fn, what, _err(hip_lib))

    cam = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 16)
    opts = va.make_opts(seed=1, early_stop=False)
    out = C.c_void_p()
    cb, ob = C.byref(cam), C.byref(opts)
    for flags in (2, 3, 1 << 31):
        refused("vmx_progressive_begin_ex", (N, cb, ob, flags, N, C.byref(out)), "unknown flag")
    for flags in (0, 1):
        refused("vmx_progressive_begin_ex", (N, cb, ob, flags, N, C.byref(out)), "NULL scene")
        refused("vmx_progressive_begin_ex", (N, N, ob, flags, N, C.byref(out)), "NULL argument")
        refused("vmx_progressive_begin_ex", (N, cb, ob, flags, N, N), "NULL out")
    refused("vmx_progressive_state_device", (N, N, N), "no output")
    refused("vmx_progressive_state_device", (N, ptr, ptr + 16), "NULL handle")
    refused("vmx_progressive_state_device", (N, ptr + 2, N), "4-byte aligned")
    refused("vmx_progressive_state_device", (N, N, ptr + 1), "4-byte aligned")
    refused("vmx_progressive_state_device", (N, ptr, ptr + 12), "d_sums and d_counts overlap")
    refused("vmx_progressive_step_selected_device", (N, 1, N, N, N), "NULL d_select")
    refused("vmx_progressive_step_selected_device", (N, 1, ptr, N, N), "NULL handle")
    refused("vmx_progressive_error_device", (N, N, N, N), "no output")
    refused("vmx_progressive_error_device", (N, N, ptr, ptr + 4), "NULL handle")
    refused("vmx_progressive_error_device", (N, N, ptr + 3, N), "4-byte aligned")
    refused("vmx_progressive_error_device", (N, N, N, ptr + 2), "4-byte aligned")
    refused("vmx_progressive_error_device", (N, N, ptr, ptr), "d_error and d_variance overlap")
    refused("vmx_progressive_select_device", (N, N, N, N), "NULL d_select")
    refused("vmx_progressive_select_device", (N, N, ptr, N), "NULL handle")
    refused("vmx_progressive_select_device", (N, N, ptr, ptr + 6), "d_count must be 4-byte aligned")
    refused("vmx_progressive_select_device", (N, N, ptr + 5, ptr + 4), "d_select and d_count overlap")
    refused("vmx_progressive_step_adaptive", (N, 1, N, N, N), "NULL handle")
    bad = [dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=-0.5),
           dict(floor=float("nan")), dict(floor=float("inf")), dict(floor=0.0), dict(floor=-0.1),
           dict(min_samples=0), dict(min_samples=1), dict(radius=4), dict(radius=1 << 31)]
    for kw in bad:
        p = va.make_sampling_params(**kw)
        for fn, args in (("vmx_progressive_error_device", (N, C.byref(p), N, N)), ("vmx_progressive_select_device", (N, C.byref(p), N, N)),
                         ("vmx_progressive_step_adaptive", (N, 1, C.byref(p), N, N))):
            refused(fn, args, "vmx_sampling_params")
            assert list(kw)[0] in _err(hip_lib), (kw, _err(hip_lib))
    for i in range(4):
        p = va.make_sampling_params()
        p.reserved[i] = 1
        refused("vmx_progressive_select_device", (N, C.byref(p), ptr, N), "vmx_sampling_params: reserved")
    ok = va.make_sampling_params(threshold=0.0, min_samples=2, radius=0)
    refused("vmx_progressive_select_device", (N, C.byref(ok), ptr, N), "NULL handle")


def test_args_program_builds_and_passes(tmp_path):
    """tests/cpp/sampling_args.cpp, the program to run under the host sanitizers (against a library built with them), built
    plainly: the same checks through the C header, from C++"""
    exe = tmp_path / "sampling_args"
    so_dir = os.path.join(ROOT, "vermilion_amd")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "sampling_args.cpp"), os.path.join(so_dir, "libvermilion_hip.so"),
                    "-Wl,-rpath," + so_dir, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "clean" in run.stdout, run.stderr


# ---- the restatement on synthetic samples ---------------------------------------------------------------------------------
KMAX = 64


def synthetic(seed=3, rows=12, w=17, n=16):
    """n samples per pixel of a rows x w image: a constant pixel, a black one, and noise of mixed amplitude elsewhere"""
    rng = np.random.RandomState(seed)
    s = (rng.uniform(0, 1, (n, rows, w, 3)) * rng.uniform(0, 2, (1, rows, w, 1))).astype(F)
    s[:, 2, 3] = F(0.25)
    s[:, 5, 5] = 0
    return s


def test_fold_is_the_sum_of_squared_luminances():
    s = synthetic()
    acc = SS.fold(s)
    assert acc.dtype == F and acc.shape == (12, 17, 4)
    l = SS.luminance(s[..., 0], s[..., 1], s[..., 2]).astype(np.float64)
    want = (l * l).sum(axis=0)
    # n adds and n squares of one rounding each: (2n) half-ulps of the running sum at most
    assert np.all(np.abs(acc[..., 3] - want) <= 2 * 16 * 0.5 * np.spacing(acc[..., 3]) + 1e-30)
    assert np.array_equal(SS.fold(s[8:], SS.fold(s[:8])).view(np.uint32), acc.view(np.uint32))  # resumable, bit for bit
    # a black sample adds an exact +0
    z = np.concatenate([s[:4], np.zeros_like(s[:1]), s[4:]])
    assert np.array_equal(SS.fold(z).view(np.uint32), acc.view(np.uint32))


def test_constant_and_black_pixels_have_no_error():
    s = synthetic()
    e, var = SS.error_variance(SS.fold(s), np.full((12, 17), 16), 0.05)
    assert e[5, 5] == 0 and var[5, 5] == 0
    # a constant pixel: m2/n - m1^2 is rounding noise, clamped at 0 or tiny against the mean
    assert e[2, 3] < 1e-3
    c = np.zeros((2, 1, 1, 3), F)
    c[:] = 0.5  # two equal samples: every sum is a doubling, m2/2 and m1*m1 are the same product
    e1, v1 = SS.error_variance(SS.fold(c), np.full((1, 1), 2), 0.05)
    assert e1[0, 0] == 0 and v1[0, 0] == 0
    noisy = np.ones((12, 17), bool)
    noisy[2, 3] = noisy[5, 5] = False
    assert (e[noisy] > 1e-3).all() and (var[noisy] > 0).all()


def test_fewer_than_two_samples_has_no_estimate():
    s = synthetic(n=1)
    for n in (0, 1):
        e, var = SS.error_variance(SS.fold(s[:n]), np.full((12, 17), n), 0.05)
        assert (e == SS.NO_ESTIMATE).all() and (var == 0).all()


def test_selection_properties():
    s = synthetic()
    acc = SS.fold(s)
    n = np.full((12, 17), 16)
    e, _ = SS.error_variance(acc, n, 0.05)
    # threshold 0 selects every unfinished pixel with a nonzero error, and with radius 0 no other
    sel = SS.select(acc, n, KMAX, threshold=0.0, floor=0.05, min_samples=2, radius=0)
    assert np.array_equal(sel.astype(bool), e > 0) and not sel[5, 5]
    # n < min_samples always selects, whatever the error
    assert SS.select(acc, n, KMAX, threshold=1e30, min_samples=17, radius=0).all()
    assert not SS.select(acc, n, KMAX, threshold=1e30, min_samples=16, radius=0).any()
    # a finished pixel is never selected
    done = n.copy()
    done[3:6, 4:9] = KMAX
    sel = SS.select(acc, done, KMAX, threshold=0.0, min_samples=KMAX + 1, radius=3)
    assert not sel[3:6, 4:9].any() and sel[done < KMAX].all()
    # the radius dilates by exactly that many pixels: one pixel above the threshold
    one = np.zeros((12, 17, 4), F)
    one[6, 8] = SS.fold(np.float32([[1, 1, 1], [0, 0, 0]]).reshape(2, 1, 3))[0]
    cnt = np.full((12, 17), 2)
    for r in (0, 1, 2, 3):
        sel = SS.select(one, cnt, KMAX, threshold=0.5, floor=0.05, min_samples=2, radius=r).astype(bool)
        want = np.zeros((12, 17), bool)
        want[6 - r:6 + r + 1, 8 - r:8 + r + 1] = True
        assert np.array_equal(sel, want), r
    # ... clipped at the image's border
    one[:] = 0
    one[0, 0] = SS.fold(np.float32([[1, 1, 1], [0, 0, 0]]).reshape(2, 1, 3))[0]
    sel = SS.select(one, cnt, KMAX, threshold=0.5, min_samples=2, radius=2).astype(bool)
    assert sel[:3, :3].all() and sel.sum() == 9
    # an error equal to the threshold is not above it
    e1, _ = SS.error_variance(one, cnt, 0.05)
    assert not SS.select(one, cnt, KMAX, threshold=float(e1[0, 0]), min_samples=2, radius=0).any()


def test_nan_sums_select_nothing_beyond_the_min_samples_rule():
    s = synthetic()
    acc = SS.fold(s)
    acc[4, 4] = np.nan
    acc[7, 2, 3] = np.nan
    acc[9, 9, 0] = np.inf
    n = np.full((12, 17), 16)
    e, var = SS.error_variance(acc, n, 0.05)
    assert var[7, 2] == 0 and e[7, 2] == 0  # a NaN second moment gives variance 0
    sel = SS.select(acc, n, KMAX, threshold=1e30, min_samples=8, radius=3)
    assert not sel.any()
    few = n.copy()
    few[4, 4] = 3
    sel = SS.select(acc, few, KMAX, threshold=1e30, min_samples=8, radius=3)
    assert sel.sum() == 1 and sel[4, 4]


def test_simulated_allocation_terminates_and_respects_kmax():
    """Bernoulli-times-constant pixels: pixel p returns a[p] with probability q[p], else 0.  8 uniform samples, then adaptive
    steps of 4 by the restatement's own map until nothing is selected: the loop ends, no count passes kmax, and the
    samples went to the pixels whose mean is the least certain."""
    rng = np.random.RandomState(11)
    rows, w = 16, 20
    q = np.where(np.arange(w)[None, :] < 10, 0.2, 0.999) * np.ones((rows, 1))
    a = F(0.8)
    acc = np.zeros((rows, w, 4), F)
    n = np.zeros((rows, w), np.int64)

    def take(mask, k):
        nonlocal acc, n
        k = np.minimum(k, KMAX - n) * mask
        for _ in range(int(k.max())):
            live = k > 0
            s = np.where(rng.uniform(size=(rows, w)) < q, a, F(0)).astype(F) * live
            smp = np.repeat(s[None, :, :, None], 3, axis=3)
            acc = np.where(live[..., None], SS.fold(smp, acc), acc)
            n = n + live
            k = k - live

    take(np.ones((rows, w), bool), 8)
    steps = 0
    while True:
        sel = SS.select(acc, n, KMAX, **SS.DEFAULTS).astype(bool)
        if not sel.any():
            break
        assert not sel[n >= KMAX].any()
        take(sel, 4)
        steps += 1
        assert steps <= rows * w * (KMAX - 8) // 4, "every step gives some pixel samples, and none passes kmax: the loop is bounded"
    assert n.max() <= KMAX and n.min() >= 8
    assert n[:, :9].mean() > n[:, 12:].mean()
