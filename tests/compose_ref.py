"""ctypes binding of the composite's checker (tests/compose/compose_ref.c; TEST INFRASTRUCTURE).

The C file includes the oracle's translation unit, so the shared library is rebuilt (gcc, the
oracle's flags) whenever it or one of the oracle's sources is newer.  __graft_entry__.build()
builds it too.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "compose", "compose_ref.c")
_LIB_PATH = os.path.join(_HERE, "compose", "libcompose_ref.so")
_DEPS = [_SRC] + [os.path.join(_ROOT, "oracle", f) for f in ("gsm_oracle.c", "gsm_oracle.h", "gsm_oracle_math.h")]
# oracle/Makefile's flags: every fp op rounds on its own (DESIGN.md numeric contract)
_CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra",
           "-Wno-unused-function"]


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
        L.cr_render.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                C.POINTER(CrObject), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                C.POINTER(C.POINTER(O.OgFrame))]
        L.cr_render.restype = C.c_int
        L.cr_frame_free.argtypes = [C.POINTER(O.OgFrame)]
        _CrObject = CrObject
        _lib = L
    return _lib


def render(objects, sh_components: int, width: int, height: int, max_gaussians: int | None = None,
           max_width: int | None = None, max_height: int | None = None, color_space: int = 0,
           nthreads: int = 0) -> dict:
    """One composite (cr_render).  objects: [(world, harmonics, camera dict)], all of one dtype; the buffers are
    concatenated here and ids are concatenated ids.  Returns the oracle's dictionary (oracle.render) plus
    "first": every object's first id."""
    import oracle as O
    L = lib()
    worlds = [np.ascontiguousarray(w) for w, _, _ in objects]
    harms = [np.ascontiguousarray(h).reshape(-1) for _, h, _ in objects]
    world = np.concatenate(worlds)
    harm = np.concatenate(harms)
    precision = 1 if world.dtype == O.WORLD16 else 0
    n = len(world)
    cfg = O.OgConfig(max_gaussians if max_gaussians is not None else max(n, 1), max_width or width,
                     max_height or height, precision, color_space)
    arr = (_CrObject * len(objects))()
    first = []
    at = 0
    for a, w, (_, _, cam) in zip(arr, worlds, objects):
        a.first, a.count, a.camera = at, len(w), O.dict_to_camera(cam)
        first.append(at)
        at += len(w)
    out = C.POINTER(O.OgFrame)()
    rc = L.cr_render(C.byref(cfg), world.ctypes.data if world.size else None,
                     harm.ctypes.data if harm.size else None, n, sh_components, arr, len(objects), width, height,
                     O._nthreads(nthreads), C.byref(out))
    if rc != 0:
        return {"status": rc}
    f = out.contents
    try:
        tot = f.total_assignments
        res = {
            "status": 0, "count": f.count, "first": first, "tiles_x": f.tiles_x, "tiles_y": f.tiles_y,
            "tile_count": f.tile_count, "max_assignments": f.max_assignments, "total_assignments": tot,
            "overflow": f.overflow, "visible": f.visible, "active_tiles": f.active_tiles,
            "render_data": O._arr(f.render_data, O.RENDER_DATA, f.count),
            "bounds": O._arr(f.bounds, np.int32, f.count * 4).reshape(-1, 4),
            "mask": O._arr(f.mask, np.uint8, f.count),
            "tile_counts": O._arr(f.tile_counts, np.uint32, f.count),
            "keys": O._arr(f.keys, np.uint32, tot), "values": O._arr(f.values, np.int32, tot),
            "sorted_keys": O._arr(f.sorted_keys, np.uint32, tot),
            "sorted_values": O._arr(f.sorted_values, np.int32, tot),
            "headers": O._arr(f.headers, np.uint32, f.tile_count * 2).reshape(-1, 2),
            "color": O._arr(f.color, np.uint16, width * height * 4).reshape(height, width, 4),
            "depth": O._arr(f.depth, np.uint16, width * height).reshape(height, width),
        }
    finally:
        L.cr_frame_free(out)
    return res
