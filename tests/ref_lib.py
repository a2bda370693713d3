"""ctypes binding of oracle/_ref/libvmx_ref*.so: the reference's OWN translation units, compiled unmodified against
the stand-in headers of oracle/ref_standin/ and wrapped by oracle/ref_driver.cpp (`make -C oracle ref`).  Test
infrastructure only.  The libraries are never committed; a checkout that has the reference tree builds them."""
import ctypes as C
import os
import subprocess

import numpy as np

from vermilion_amd.scene import RAYHIT_DTYPE

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ODIR = os.path.join(_ROOT, "oracle")
_RDIR = os.path.join(_ODIR, "_ref")
REFERENCE_TREE = os.environ.get("VERMILION_REF", "/root/reference")

PARITY, LIBM_DOUBLE, FAST = "libvmx_ref.so", "libvmx_ref_libmdouble.so", "libvmx_ref_fast.so"
# the fields of vmx_rayhit that MeshEngine::RayCast returns; tri_id and tri_t are this project's additions to the
# record (RayCast does not report the BVH hit on its own) and exist on the oracle's and the kernels' side only
RAYHIT_REFERENCE_FIELDS = ("location", "distance", "normal", "uv", "flags", "colour")


def have_reference_tree():
    return os.path.isdir(os.path.join(REFERENCE_TREE, "core"))


def available():
    """True where the comparison can run: the library is there, or the reference tree to build it from is"""
    return os.path.exists(os.path.join(_RDIR, PARITY)) or have_reference_tree()


def build():
    subprocess.run(["make", "-C", _ODIR, "ref", "VERMILION_REF=" + REFERENCE_TREE], check=True, stdout=subprocess.DEVNULL)


_libs = {}


def lib(name=PARITY):
    """raises where the library is missing and cannot be built: a missing reference build is an error, not a skip"""
    if name in _libs:
        return _libs[name]
    path = os.path.join(_RDIR, name)
    if not os.path.exists(path):
        if not have_reference_tree():
            raise RuntimeError(f"{path} is missing and there is no reference tree at {REFERENCE_TREE} to build it from")
        build()
    l = C.CDLL(path)
    P = C.c_void_p
    l.ref_build_flags.restype = C.c_char_p
    l.ref_scene_create.restype = P
    l.ref_scene_create.argtypes = [P, P, P, C.c_uint32, C.c_uint32, P, P, C.c_uint32]
    l.ref_scene_destroy.argtypes = [P]
    l.ref_scene_bind_texture.argtypes = [P, P, C.c_uint32, C.c_uint32, C.c_uint32]
    l.ref_scene_describe.argtypes = [P, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    l.ref_scene_bvh.argtypes = [P, C.c_int, P, P, P, P, P]
    l.ref_trace.argtypes = [P, P, P, C.c_uint32, P, P]
    l.ref_raycast.argtypes = [P, P, P, C.c_uint32, P]
    l.ref_collision.argtypes = [P, P, P, C.c_uint32, P]
    l.ref_texture_sample.argtypes = [P, C.c_uint32, C.c_uint32, C.c_uint32, P, C.c_uint32, P]
    l.ref_radiance_mt.argtypes = [P, P, P, C.c_uint32, P, P]
    l.ref_quantize.argtypes = [P, C.c_uint32, C.c_uint32, P, P]
    _libs[name] = l
    return l


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


class RefScene:
    """pos / nrm / uv as OracleScene takes them.  mesh_sizes: consecutive triangle ranges, one aiMesh each;
    mesh_has_uv: per mesh, False leaves that mesh without texture coordinates.  leaf_size applies to the tree built
    through BVH(objects, leaf) — trace() and bvh() use it; raycast / collision / radiance_mt go through
    MeshEngine::load -> createBVH, which always takes the default of 4."""

    def __init__(self, pos, nrm, uv=None, leaf_size=4, mesh_sizes=None, mesh_has_uv=None, which=PARITY):
        self.l = lib(which)
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
        nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 9)
        uvp = None
        if uv is not None:
            uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 6)
            uvp = uv.ctypes.data
        self.ntris = pos.shape[0]
        ms = mh = None
        nm = 0
        if mesh_sizes is not None:
            ms = np.ascontiguousarray(mesh_sizes, np.uint32)
            nm = len(ms)
            if mesh_has_uv is not None:
                mh = np.ascontiguousarray(mesh_has_uv, np.uint8)
                assert len(mh) == nm
        self.h = self.l.ref_scene_create(pos.ctypes.data, nrm.ctypes.data, uvp, self.ntris, leaf_size,
                                         None if ms is None else ms.ctypes.data, None if mh is None else mh.ctypes.data, nm)
        if not self.h:
            raise RuntimeError("ref_scene_create failed")

    def close(self):
        if self.h:
            self.l.ref_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind_texture(self, data):
        data = np.ascontiguousarray(data, np.float32)
        h, w = data.shape[0], data.shape[1]
        c = 1 if data.ndim == 2 else data.shape[2]
        if self.l.ref_scene_bind_texture(self.h, data.ctypes.data, w, h, c) != 0:
            raise ValueError("bad texture")

    def describe(self, engine_tree=False):
        a, b = C.c_uint32(), C.c_uint32()
        self.l.ref_scene_describe(self.h, int(engine_tree), C.byref(a), C.byref(b))
        return {"n_nodes": a.value, "n_leaves": b.value}

    def bvh(self, engine_tree=False):
        """the flat tree in OracleScene.bvh()'s layout; the engine's tree comes without prim_order"""
        n = self.describe(engine_tree)["n_nodes"]
        start, nprims, roff = (np.zeros(n, np.uint32) for _ in range(3))
        bbox = np.zeros((n, 6), np.float32)
        order = np.zeros(self.ntris, np.uint32)
        self.l.ref_scene_bvh(self.h, int(engine_tree), start.ctypes.data, nprims.ctypes.data, roff.ctypes.data,
                             bbox.ctypes.data, None if engine_tree else order.ctypes.data)
        out = {"start": start, "nprims": nprims, "right_offset": roff, "bbox": bbox}
        if not engine_tree:
            out["prim_order"] = order
        return out

    def trace(self, o, d):
        o, d = _f32(o), _f32(d)
        n = o.shape[0]
        tri = np.empty(n, np.int32)
        t = np.empty(n, np.float32)
        self.l.ref_trace(self.h, o.ctypes.data, d.ctypes.data, n, tri.ctypes.data, t.ctypes.data)
        return tri, t

    def raycast(self, o, d):
        o, d = _f32(o), _f32(d)
        out = np.zeros(o.shape[0], dtype=RAYHIT_DTYPE)
        self.l.ref_raycast(self.h, o.ctypes.data, d.ctypes.data, o.shape[0], out.ctypes.data)
        return out

    def collision(self, o, d):
        o, d = _f32(o), _f32(d)
        out = np.zeros(o.shape[0], np.uint8)
        self.l.ref_collision(self.h, o.ctypes.data, d.ctypes.data, o.shape[0], out.ctypes.data)
        return out.astype(bool)

    def radiance_mt(self, o, d, seeds):
        o, d = _f32(o), _f32(d)
        seeds = np.ascontiguousarray(seeds, np.uint64)
        out = np.empty((o.shape[0], 4), np.float32)
        self.l.ref_radiance_mt(self.h, o.ctypes.data, d.ctypes.data, o.shape[0], seeds.ctypes.data, out.ctypes.data)
        return out


def texture_sample(data, uv, which=PARITY):
    """VermiTexture::Sample of the [H, W(, C)] float texture at uv[n, 2]; components Sample leaves alone read -1"""
    data = np.ascontiguousarray(data, np.float32)
    h, w = data.shape[0], data.shape[1]
    c = 1 if data.ndim == 2 else data.shape[2]
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    out = np.empty((uv.shape[0], 4), np.float32)
    lib(which).ref_texture_sample(data.ctypes.data, w, h, c, uv.ctypes.data, uv.shape[0], out.ctypes.data)
    return out


def quantize(frame, W, H, which=PARITY):
    """Camera::saveFrame's conversion of an RGBAZ frame: (rgba8 [W*H, 4], depth [W*H])"""
    frame = np.ascontiguousarray(frame, np.float32).reshape(-1, 5)
    assert frame.shape[0] == W * H
    rgba = np.zeros((W * H, 4), np.uint8)
    depth = np.zeros(W * H, np.float32)
    lib(which).ref_quantize(frame.ctypes.data, W, H, rgba.ctypes.data, depth.ctypes.data)
    return rgba, depth
