"""ctypes binding of the pick target's checker (tests/pick/pick_ref.c; TEST INFRASTRUCTURE).

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
_SRC = os.path.join(_HERE, "pick", "pick_ref.c")
_LIB_PATH = os.path.join(_HERE, "pick", "libpick_ref.so")
_DEPS = [_SRC, os.path.join(_HERE, "compose", "compose_ref.c")] + \
    [os.path.join(_ROOT, "oracle", f) for f in ("gsm_oracle.c", "gsm_oracle.h", "gsm_oracle_math.h")]
# oracle/Makefile's flags: every fp op rounds on its own (DESIGN.md numeric contract)
_CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra",
           "-Wno-unused-function"]

PICK_NONE = 0xFFFFFFFF
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
        L.pr_pick.argtypes = [C.POINTER(O.OgFrame), C.c_void_p, C.c_void_p, C.c_void_p]
        L.pr_pick.restype = C.c_long
        _CrObject = CrObject
        _lib = L
    return _lib


def _finish(L, out, width, height):
    """pr_pick over the finished frame `out`, then the frame as a dictionary; frees the frame."""
    import oracle as O
    f = out.contents
    try:
        tot = f.total_assignments
        pick = np.zeros((height, width), np.uint32)
        pos = np.zeros((height, width), np.uint32)
        records = np.zeros((max(f.count, 1), len(RECORD_FIELDS)), np.uint16)
        differ = int(L.pr_pick(out, pick.ctypes.data, pos.ctypes.data, records.ctypes.data))
        return {
            "status": 0, "count": f.count, "tiles_x": f.tiles_x, "tiles_y": f.tiles_y, "tile_count": f.tile_count,
            "total_assignments": tot, "overflow": f.overflow, "active_tiles": f.active_tiles,
            "sorted_values": O._arr(f.sorted_values, np.int32, tot),
            "headers": O._arr(f.headers, np.uint32, f.tile_count * 2).reshape(-1, 2),
            "color": O._arr(f.color, np.uint16, width * height * 4).reshape(height, width, 4),
            "depth": O._arr(f.depth, np.uint16, width * height).reshape(height, width),
            "group_iters": O._arr(f.group_iters, np.uint32, f.tile_count * 64).reshape(-1, 8, 8),
            "differ": differ, "pick": pick, "pick_pos": pos, "records": records[:f.count],
        }
    finally:
        L.cr_frame_free(out)


def render(world, harmonics, sh_components: int, camera: dict, width: int, height: int,
           max_gaussians: int | None = None, max_width: int | None = None, max_height: int | None = None,
           color_space: int = 0, nthreads: int = 0) -> dict:
    """og_render, then pr_pick.  Returns colour, depth, the sorted list, the headers and group_iters of the
    oracle's frame, plus "pick" (gaussian ids, PICK_NONE), "pick_pos" (the winner's list position), "records"
    (RECORD_FIELDS per gaussian) and "differ" (the checker's colour / depth values that differ from the oracle's:
    must be 0)."""
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
    if rc != 0:
        return {"status": rc}
    return _finish(L, out, width, height)


def render_composite(objects, sh_components: int, width: int, height: int, max_gaussians: int | None = None,
                     max_width: int | None = None, max_height: int | None = None, color_space: int = 0,
                     nthreads: int = 0) -> dict:
    """cr_render of [(world, harmonics, camera dict)], then pr_pick: as render(), ids = concatenated ids, plus
    "first" (every object's first id) and "counts"."""
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
    if rc != 0:
        return {"status": rc}
    res = _finish(L, out, width, height)
    res["first"], res["counts"] = first, [len(w) for w in worlds]
    return res
