"""ctypes binding of the DepthFirst mono restatement (tests/df_mono/df_mono_ref.c; TEST INFRASTRUCTURE).

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
_SRC = os.path.join(_HERE, "df_mono", "df_mono_ref.c")
_LIB_PATH = os.path.join(_HERE, "df_mono", "libdf_mono_ref.so")
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


class DfmFrame(C.Structure):
    _fields_ = [("count", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32), ("tile_count", C.c_uint32),
                ("max_instances", C.c_uint32), ("visible", C.c_uint32),
                ("total_instances", C.c_uint32), ("overflow", C.c_uint32), ("active_tiles", C.c_uint32),
                ("render_data", C.c_void_p), ("bounds", C.c_void_p), ("touched", C.c_void_p),
                ("depth_keys", C.c_void_p), ("depth_order", C.c_void_p),
                ("inst_tiles", C.c_void_p), ("inst_gids", C.c_void_p), ("headers", C.c_void_p),
                ("color", C.c_void_p), ("depth", C.c_void_p)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        import oracle as O
        L = C.CDLL(build())
        L.dfm_render.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                 C.POINTER(O.OgCamera), C.c_uint32, C.c_uint32, C.c_int,
                                 C.POINTER(C.POINTER(DfmFrame))]
        L.dfm_render.restype = C.c_int
        L.dfm_frame_free.argtypes = [C.POINTER(DfmFrame)]
        _lib = L
    return _lib


def render(world: np.ndarray, harmonics: np.ndarray, sh_components: int, camera: dict, width: int, height: int,
           max_gaussians: int | None = None, max_width: int | None = None, max_height: int | None = None,
           color_space: int = 0, nthreads: int = 0) -> dict:
    """One mono frame (dfm_render); every intermediate, the colour and the depth as numpy arrays."""
    import oracle as O
    L = lib()
    precision = 1 if world.dtype == O.WORLD16 else 0
    n = len(world)
    cfg = O.OgConfig(max_gaussians if max_gaussians is not None else max(n, 1), max_width or width,
                     max_height or height, precision, color_space)
    cam = O.dict_to_camera(camera)
    world = np.ascontiguousarray(world)
    harmonics = np.ascontiguousarray(harmonics)
    out = C.POINTER(DfmFrame)()
    rc = L.dfm_render(C.byref(cfg), world.ctypes.data if world.size else None,
                      harmonics.ctypes.data if harmonics.size else None, n, sh_components, C.byref(cam),
                      width, height, O._nthreads(nthreads), C.byref(out))
    if rc != 0:
        return {"status": rc}
    f = out.contents
    try:
        tot, V = f.total_instances, f.visible
        res = {
            "status": 0, "count": f.count, "tiles_x": f.tiles_x, "tiles_y": f.tiles_y,
            "tile_count": f.tile_count, "max_instances": f.max_instances, "visible": V,
            "total_instances": tot, "overflow": f.overflow, "active_tiles": f.active_tiles,
            "render_data": O._arr(f.render_data, O.RENDER_DATA, f.count),
            "bounds": O._arr(f.bounds, np.int32, f.count * 4).reshape(-1, 4),
            "touched": O._arr(f.touched, np.uint32, f.count),
            "depth_keys": O._arr(f.depth_keys, np.uint32, f.count),
            "depth_order": O._arr(f.depth_order, np.int32, V),
            "inst_tiles": O._arr(f.inst_tiles, np.uint32, tot),
            "inst_gids": O._arr(f.inst_gids, np.int32, tot),
            "headers": O._arr(f.headers, np.uint32, f.tile_count * 2).reshape(-1, 2),
            "color": O._arr(f.color, np.uint16, width * height * 4).reshape(height, width, 4),
            "depth": O._arr(f.depth, np.uint16, width * height).reshape(height, width),
        }
    finally:
        L.dfm_frame_free(out)
    return res
