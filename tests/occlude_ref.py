"""ctypes binding of the occluded frames' checker (tests/occlude/occlude_ref.c; TEST INFRASTRUCTURE).

The C file includes the composite's checker and, through it, the oracle's translation unit, so the shared
library is rebuilt (gcc, the oracle's flags) whenever it or one of those sources is newer.
__graft_entry__.build() builds it too.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "occlude", "occlude_ref.c")
_LIB_PATH = os.path.join(_HERE, "occlude", "libocclude_ref.so")
_DEPS = [_SRC, os.path.join(_HERE, "compose", "compose_ref.c")] + \
    [os.path.join(_ROOT, "oracle", f) for f in ("gsm_oracle.c", "gsm_oracle.h", "gsm_oracle_math.h")]
# oracle/Makefile's flags: every fp op rounds on its own (DESIGN.md numeric contract)
_CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra",
           "-Wno-unused-function"]

# the columns of "records": the oracle's per-gaussian blend record, fp16 bits
RECORD_FIELDS = ("mx", "my", "cxx", "cyy", "cxy2", "op", "cr", "cg", "cb", "dep")


def build(force: bool = False) -> str:
    if force or not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < max(map(os.path.getmtime, _DEPS)):
        tmp = _LIB_PATH + f".{os.getpid()}.tmp"
        subprocess.run([os.environ.get("CC", "gcc")] + _CFLAGS + ["-shared", "-o", tmp, _SRC, "-lm", "-lpthread"],
                       check=True)
        os.replace(tmp, _LIB_PATH)
    return _LIB_PATH


_lib = None
_CrObject = None


def lib():
    global _lib, _CrObject
    if _lib is None:
        import oracle as O

        class CrObject(C.Structure):
            _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("camera", O.OgCamera)]

        L = C.CDLL(build())
        L.og_render.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                C.POINTER(O.OgCamera), C.c_uint32, C.c_uint32, C.c_int,
                                C.POINTER(C.POINTER(O.OgFrame))]
        L.og_render.restype = C.c_int
        L.cr_render.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                C.POINTER(CrObject), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                C.POINTER(C.POINTER(O.OgFrame))]
        L.cr_render.restype = C.c_int
        L.cr_frame_free.argtypes = [C.POINTER(O.OgFrame)]
        L.or_occlude.argtypes = [C.POINTER(O.OgFrame), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int]
        L.or_occlude.restype = C.c_long
        _CrObject = CrObject
        _lib = L
    return _lib


class Frame:
    """A finished oracle frame kept alive so that several occluders can be walked over it: `base` is the oracle's
    own frame as a dictionary (colour, depth, sorted list, headers, group_iters, records), occlude() the frame
    under an occluder.  close() frees it."""

    def __init__(self, L, out, width, height, extra=None):
        import oracle as O
        self._L, self._out, self.width, self.height = L, out, width, height
        f = out.contents
        tot = f.total_assignments
        self.base = {
            "status": 0, "count": f.count, "tiles_x": f.tiles_x, "tiles_y": f.tiles_y, "tile_count": f.tile_count,
            "total_assignments": tot, "overflow": f.overflow, "active_tiles": f.active_tiles,
            "sorted_values": O._arr(f.sorted_values, np.int32, tot),
            "headers": O._arr(f.headers, np.uint32, f.tile_count * 2).reshape(-1, 2),
            "color": O._arr(f.color, np.uint16, width * height * 4).reshape(height, width, 4),
            "depth": O._arr(f.depth, np.uint16, width * height).reshape(height, width),
            "group_iters": O._arr(f.group_iters, np.uint32, f.tile_count * 64).reshape(-1, 8, 8),
        }
        self.base.update(extra or {})
        inf = np.full((height, width), np.inf, np.float32)
        self.base["records"] = self.occlude(inf, _records=True)["records"]

    def occlude(self, occluder, _records=False, half_model=False) -> dict:
        """or_occlude under `occluder`, a float32 array of shape (H, W) (any row stride).  Returns "color",
        "depth", "group_iters", the counts "closed_pixels", "closure_breaks", "mixed_groups", and "differ": the
        values that differ from the oracle's own frame (0 under an occluder of all +inf).  half_model: the frame of
        the wrong model a blend over half-tile lists would compute (occlude_ref.c), to be compared with the
        contract's -- where they differ, the scene tells the two apart."""
        f = self._out.contents
        w, h = self.width, self.height
        occ = np.asarray(occluder)
        assert occ.dtype == np.float32 and occ.shape == (h, w) and occ.strides[1] == 4 and occ.strides[0] % 4 == 0
        color = np.zeros((h, w, 4), np.uint16)
        depth = np.zeros((h, w), np.uint16)
        iters = np.zeros((f.tile_count, 8, 8), np.uint32)
        counts = (C.c_long * 3)()
        records = np.zeros((max(f.count, 1), len(RECORD_FIELDS)), np.uint16) if _records else None
        differ = int(self._L.or_occlude(self._out, occ.ctypes.data, occ.strides[0] // 4, color.ctypes.data,
                                        depth.ctypes.data, iters.ctypes.data, counts,
                                        records.ctypes.data if _records else None, 1 if half_model else 0))
        assert differ >= 0, "or_occlude: out of memory"
        res = {"color": color, "depth": depth, "group_iters": iters, "differ": differ,
               "closed_pixels": int(counts[0]), "closure_breaks": int(counts[1]), "mixed_groups": int(counts[2])}
        if _records:
            res["records"] = records[:f.count]
        return res

    def active_pixels(self) -> np.ndarray:
        """(H, W) bool: the pixels of tiles that have list entries."""
        h, w = self.height, self.width
        tiles = (np.arange(h)[:, None] // 16) * self.base["tiles_x"] + np.arange(w)[None, :] // 32
        return self.base["headers"][:, 1][tiles] > 0

    def close(self):
        if self._out is not None:
            self._L.cr_frame_free(self._out)
            self._out = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def frame(world, harmonics, sh_components: int, camera: dict, width: int, height: int,
          max_gaussians: int | None = None, max_width: int | None = None, max_height: int | None = None,
          color_space: int = 0, nthreads: int = 0) -> Frame:
    """og_render, kept as a Frame."""
    import oracle as O
    L = lib()
    world = np.ascontiguousarray(world)
    harmonics = np.ascontiguousarray(harmonics).reshape(-1)
    n = len(world)
    cfg = O.OgConfig(max_gaussians if max_gaussians is not None else max(n, 1), max_width or width,
                     max_height or height, 1 if world.dtype == O.WORLD16 else 0, color_space)
    cam = O.dict_to_camera(camera)
    out = C.POINTER(O.OgFrame)()
    rc = L.og_render(C.byref(cfg), world.ctypes.data if world.size else None,
                     harmonics.ctypes.data if harmonics.size else None, n, sh_components, C.byref(cam), width,
                     height, O._nthreads(nthreads), C.byref(out))
    assert rc == 0, f"og_render: {rc}"
    return Frame(L, out, width, height)


def frame_composite(objects, sh_components: int, width: int, height: int, max_gaussians: int | None = None,
                    max_width: int | None = None, max_height: int | None = None, color_space: int = 0,
                    nthreads: int = 0) -> Frame:
    """cr_render of [(world, harmonics, camera dict)], kept as a Frame (ids = concatenated ids; base["first"],
    base["counts"])."""
    import oracle as O
    L = lib()
    worlds = [np.ascontiguousarray(w) for w, _, _ in objects]
    harms = [np.ascontiguousarray(h).reshape(-1) for _, h, _ in objects]
    world, harm = np.concatenate(worlds), np.concatenate(harms)
    n = len(world)
    cfg = O.OgConfig(max_gaussians if max_gaussians is not None else max(n, 1), max_width or width,
                     max_height or height, 1 if world.dtype == O.WORLD16 else 0, color_space)
    arr = (_CrObject * len(objects))()
    first, at = [], 0
    for a, w, (_, _, cam) in zip(arr, worlds, objects):
        a.first, a.count, a.camera = at, len(w), O.dict_to_camera(cam)
        first.append(at)
        at += len(w)
    out = C.POINTER(O.OgFrame)()
    rc = L.cr_render(C.byref(cfg), world.ctypes.data if world.size else None, harm.ctypes.data if harm.size else None,
                     n, sh_components, arr, len(objects), width, height, O._nthreads(nthreads), C.byref(out))
    assert rc == 0, f"cr_render: {rc}"
    return Frame(L, out, width, height, {"first": first, "counts": [len(w) for w in worlds]})
