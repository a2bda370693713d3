"""Light sampling across ranks and devices, and on device batches (vmx_render_nee_rank*, vmx_progressive_begin_nee_rank,
vmx_multi_render_nee*, vmx_radiance_nee_device) without a GPU: the symbols, the header, and the argument checks that come
before any device work, each seen alone and in the order the header states.  The entries these are built beside keep their
contract: they still refuse world > 1 with their message."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import dist as vdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_render_nee_rank", "vmx_render_nee_rank_device", "vmx_progressive_begin_nee_rank", "vmx_multi_render_nee",
           "vmx_multi_render_nee_device", "vmx_radiance_nee_device")
CORRECTED = L.VMX_SAMPLING_CORRECTED
WORLD_MESSAGE = "light sampling: world > 1 is not supported"
N = None
P = C.byref


def _err(lib):
    return lib.vmx_last_error().decode()


def _opts(**kw):
    kw.setdefault("sampling", CORRECTED)
    kw.setdefault("early_stop", False)
    return va.make_opts(seed=3, **kw)


def _cam(spp=8):
    return va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, spp)


def refused(lib, call, what, exact=False):
    assert call() == L.VMX_ERR_INVALID, what
    assert (_err(lib) == what) if exact else (what in _err(lib)), (what, _err(lib))


class Args:
    """valid buffers for every entry; a NULL scene / vmx_multi"""

    def __init__(self):
        self.frame = np.zeros((8, 16, 5), np.float32)
        self.o, self.d = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
        self.out = np.zeros(4 * 4 + 4, np.float32)
        self.out4 = (self.out.ctypes.data + 15) & ~15
        self.st = L.Stats()
        self.h = C.c_void_p()

    def rank_calls(self, lib, cam, opts):
        """the entries that take a rank: (name, call)"""
        f, st = self.frame.ctypes.data, P(self.st)
        return [
            ("vmx_render_nee_rank", lambda: lib.vmx_render_nee_rank(N, P(cam), P(opts), f, st)),
            ("vmx_render_nee_rank_device", lambda: lib.vmx_render_nee_rank_device(N, P(cam), P(opts), f, st, N)),
            ("vmx_progressive_begin_nee_rank", lambda: lib.vmx_progressive_begin_nee_rank(N, P(cam), P(opts), 0, N, P(self.h))),
        ]

    def whole_calls(self, lib, cam, opts):
        """the new entries that take whole frames or rays only"""
        f, st = self.frame.ctypes.data, P(self.st)
        return [
            ("vmx_multi_render_nee", lambda: lib.vmx_multi_render_nee(N, P(cam), P(opts), f, st)),
            ("vmx_multi_render_nee_device", lambda: lib.vmx_multi_render_nee_device(N, P(cam), P(opts), f, st)),
            ("vmx_radiance_nee_device", lambda: lib.vmx_radiance_nee_device(N, self.o.ctypes.data, self.d.ctypes.data, 4, P(opts),
                                                                            self.out4, st, N)),
        ]

    def old_calls(self, lib, cam, opts):
        f, st = self.frame.ctypes.data, P(self.st)
        return [
            ("vmx_render_nee", lambda: lib.vmx_render_nee(N, P(cam), P(opts), f, st)),
            ("vmx_render_nee_device", lambda: lib.vmx_render_nee_device(N, P(cam), P(opts), f, st, N)),
            ("vmx_radiance_nee", lambda: lib.vmx_radiance_nee(N, self.o.ctypes.data, self.d.ctypes.data, 4, P(opts),
                                                              self.out.ctypes.data, st)),
            ("vmx_progressive_begin_nee", lambda: lib.vmx_progressive_begin_nee(N, P(cam), P(opts), 0, N, P(self.h))),
        ]


def test_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, re.S)
        assert decl, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")) == len(L.SYMBOLS[name][1]), name
    for name in ("render_nee_rank", "render_nee_rank_device", "radiance_nee_device", "progressive_nee"):
        assert callable(getattr(va.Scene, name)), name
    for name in ("render_nee", "render_nee_device"):
        assert callable(getattr(va.MultiScene, name)), name
    assert callable(vdist.render_nee_local) and callable(vdist.render_nee_gathered)
    # additive: no new ABI version, no new kernel slot in vmx_timings
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    assert re.search(r"#define VMX_K_COUNT 10\b", src) and len(L.K_NAMES) == 10
    # the header states what a rank without rows does, where the windows stop and what was not measured
    assert "A rank that owns no row" in src and "stop at the rank's own rows" in src
    assert "no node with several GPUs has run this project" in src.replace("\n * ", " ")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)


def test_null_arguments_then_the_scene_last(hip_lib):
    lib, a = hip_lib, Args()
    cam, opts = _cam(), _opts(world=3, rank=1, stripe_rows=2)
    f, st = a.frame.ctypes.data, P(a.st)
    for c, o, out in ((N, P(opts), f), (P(cam), N, f), (P(cam), P(opts), N)):
        refused(lib, lambda: lib.vmx_render_nee_rank(N, c, o, out, st), "NULL argument")
        refused(lib, lambda: lib.vmx_render_nee_rank_device(N, c, o, out, st, N), "NULL argument")
        refused(lib, lambda: lib.vmx_multi_render_nee(N, c, o, out, st), "NULL argument")
        refused(lib, lambda: lib.vmx_multi_render_nee_device(N, c, o, out, st), "NULL argument")
    for c, o in ((N, P(opts)), (P(cam), N)):
        refused(lib, lambda: lib.vmx_progressive_begin_nee_rank(N, c, o, 0, N, P(a.h)), "NULL argument")
    refused(lib, lambda: lib.vmx_progressive_begin_nee_rank(N, P(cam), P(opts), 0, N, N), "NULL out")
    for flags in (2, 3, 1 << 31):
        refused(lib, lambda: lib.vmx_progressive_begin_nee_rank(N, P(cam), P(opts), flags, N, P(a.h)), "unknown flag")
    po, pd = a.o.ctypes.data, a.d.ctypes.data
    whole = _opts()
    for o_, d_, op, out in ((N, pd, P(whole), a.out4), (po, N, P(whole), a.out4), (po, pd, N, a.out4), (po, pd, P(whole), N)):
        refused(lib, lambda: lib.vmx_radiance_nee_device(N, o_, d_, 4, op, out, N, N), "NULL argument")
    # everything else valid — a rank of a world among it: the scene is the last thing looked at
    for flags in (0, L.VMX_PROGRESSIVE_MOMENTS):
        refused(lib, lambda: lib.vmx_progressive_begin_nee_rank(N, P(cam), P(opts), flags, N, P(a.h)), "NULL scene")
    for name, call in a.rank_calls(lib, cam, opts):
        refused(lib, call, "NULL scene")
    for name, call in a.whole_calls(lib, cam, whole):
        refused(lib, call, "NULL vmx_multi" if "multi" in name else "NULL scene")


REJECTED = [
    ("parity", dict(sampling=L.VMX_SAMPLING_PARITY), "light sampling: sampling must be VMX_SAMPLING_CORRECTED"),
    ("unknown_mode", dict(sampling=2), "unknown sampling mode"),
    ("unknown_bit", dict(sampling=CORRECTED | 0x400), "unknown sampling mode"),
    ("elide_dead", dict(sampling=CORRECTED | L.VMX_SAMPLING_ELIDE_DEAD), "light sampling: VMX_SAMPLING_ELIDE_DEAD does not apply"),
    ("early_stop", dict(early_stop=True), "light sampling: early_stop is not supported"),
    ("collect_counters", dict(collect_counters=True), "light sampling: collect_counters is not supported"),
    ("reserved0", dict(pipeline=1), "light sampling: reserved[0] must be 0"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_every_other_refusal_keeps_its_message(hip_lib, case):
    """with and without a rank of a world in the same opts: the message is vmx_render_nee's"""
    _, kw, message = case
    a, cam = Args(), _cam()
    refused(hip_lib, a.old_calls(hip_lib, cam, _opts(**kw))[0][1], message, exact=True)
    for extra in (dict(), dict(world=3, rank=2, stripe_rows=2)):
        for name, call in a.rank_calls(hip_lib, cam, _opts(**kw, **extra)):
            refused(hip_lib, call, message, exact=True)
    for name, call in a.whole_calls(hip_lib, cam, _opts(**kw)):
        refused(hip_lib, call, message, exact=True)


def test_the_order_of_refusals(hip_lib):
    """opts contents in vmx_render_nee's order (the world check's place is the frame's "rank must be < world", which comes
    after all of them), then the frame, then the scene"""
    lib, a, cam = hip_lib, Args(), _cam()
    bad_rank = dict(world=2, rank=2)
    order = [(dict(sampling=2), "unknown sampling mode"),
             (dict(sampling=CORRECTED | L.VMX_SAMPLING_ELIDE_DEAD), "VMX_SAMPLING_ELIDE_DEAD"),
             (dict(early_stop=True), "early_stop"), (dict(collect_counters=True), "collect_counters"), (dict(pipeline=1), "reserved[0]")]
    for i, (kw, word) in enumerate(order):
        later = {}
        for k, _ in order[i + 1:]:
            later.update({x: y for x, y in k.items() if x != "sampling"})
        for name, call in a.rank_calls(lib, _cam(2), _opts(**dict(later, **kw), **bad_rank)):
            refused(lib, call, word)
    for name, call in a.rank_calls(lib, cam, _opts(**bad_rank)):
        refused(lib, call, "rank must be < world", exact=True)
    for name, call in a.rank_calls(lib, cam, _opts(world=2, rank=7)):
        refused(lib, call, "rank must be < world", exact=True)
    for name, call in a.rank_calls(lib, _cam(2), _opts(world=2, rank=1)):
        refused(lib, call, "rays_per_pixel < 4")
    # vmx_multi_render_nee*: opts before the vmx_multi; the old entries: opts before the scene, as they were
    for name, call in a.whole_calls(lib, cam, _opts(early_stop=True)):
        refused(lib, call, "early_stop")


def test_what_is_accepted_reaches_the_scene_check(hip_lib):
    a, cam = Args(), _cam()
    for kw in (dict(), dict(world=1), dict(world=0, rank=5), dict(world=2, rank=0), dict(world=2, rank=1, stripe_rows=1),
               dict(world=64, rank=63, stripe_rows=4), dict(world=3, rank=1, samples_per_batch=1),
               dict(world=2, rank=1, sampling=CORRECTED | L.VMX_SAMPLING_LIBM_DOUBLE)):
        for name, call in a.rank_calls(hip_lib, cam, _opts(**kw)):
            refused(hip_lib, call, "NULL scene")


def test_the_old_entries_and_the_device_list_still_refuse_a_world(hip_lib):
    a, cam = Args(), _cam()
    for kw in (dict(world=2), dict(world=2, rank=1), dict(world=8, rank=3, stripe_rows=2)):
        for name, call in a.old_calls(hip_lib, cam, _opts(**kw)) + a.whole_calls(hip_lib, cam, _opts(**kw)):
            refused(hip_lib, call, WORLD_MESSAGE, exact=True)


def test_radiance_nee_device_checks_in_the_stated_order(hip_lib):
    lib, a, opts = hip_lib, Args(), _opts()
    po, pd, out = a.o.ctypes.data, a.d.ctypes.data, a.out4

    def call(o=po, d=pd, n=4, op=opts, out4=out):
        return lambda: lib.vmx_radiance_nee_device(N, o, d, n, P(op), out4, N, N)

    # no rays: VMX_OK whatever the scene and the pointers' alignment, but the options are still checked
    assert call(n=0)() == L.VMX_OK and call(o=po + 1, out4=out + 4, n=0)() == L.VMX_OK
    refused(lib, call(n=0, op=_opts(early_stop=True)), "early_stop")
    refused(lib, call(o=po + 2), "the rays must be 4-byte aligned")
    refused(lib, call(d=pd + 1), "the rays must be 4-byte aligned")
    refused(lib, call(out4=out + 4), "d_out4 must be 16-byte aligned")
    refused(lib, call(o=po + 2, out4=out + 4), "the rays must be 4-byte aligned")  # (the rays before the output)
    # overlaps: [out, out + 16 n) against [rays, rays + 12 n), either array, from either side
    big = np.zeros(64, np.float32)
    base = (big.ctypes.data + 15) & ~15
    refused(lib, call(o=base, out4=base), "d_out4 overlaps the rays")
    refused(lib, call(d=base + 60, out4=base), "d_out4 overlaps the rays")       # the rays begin inside the output
    refused(lib, call(o=base, out4=base + 32), "d_out4 overlaps the rays")       # the output begins inside the rays
    refused(lib, call(o=base, out4=base + 48), "NULL scene")                     # 4 rays end at +48
    refused(lib, call(d=base + 64, out4=base), "NULL scene")                     # 4 results end at +64
    refused(lib, call(out4=out + 4, o=base, d=base), "d_out4 must be 16-byte aligned")  # (alignment before overlap)
    refused(lib, call(), "NULL scene")
