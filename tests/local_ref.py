"""ctypes binding of the LocalRenderer restatement (tests/local/local_ref.c; TEST INFRASTRUCTURE).

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
_SRC = os.path.join(_HERE, "local", "local_ref.c")
_LIB_PATH = os.path.join(_HERE, "local", "liblocal_ref.so")
_DEPS = [_SRC] + [os.path.join(_ROOT, "oracle", f) for f in ("gsm_oracle.c", "gsm_oracle.h", "gsm_oracle_math.h")]
# oracle/Makefile's flags: every fp op rounds on its own (DESIGN.md numeric contract)
_CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra",
           "-Wno-unused-function"]

MAX_PER_TILE = 2048
# ProjectedGaussian (BridgingTypes.h:106-114), 32 B: the same layout as gsm_amd.types.PROJECTED
PROJECTED = np.dtype([(f, "<u2") for f in ("posX", "posY", "conicA", "conicB", "conicC", "depth", "colorR",
                                            "colorG", "colorB", "opacity")] +
                     [("minTile", "<u2", (2,)), ("maxTile", "<u2", (2,)), ("obbExtentX", "<u2"),
                      ("obbExtentY", "<u2")])
assert PROJECTED.itemsize == 32


def build(force: bool = False) -> str:
    if force or not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < max(map(os.path.getmtime, _DEPS)):
        tmp = _LIB_PATH + f".{os.getpid()}.tmp"
        subprocess.run([os.environ.get("CC", "gcc")] + _CFLAGS + ["-shared", "-o", tmp, _SRC, "-lm", "-lpthread"],
                       check=True)
        os.replace(tmp, _LIB_PATH)
    return _LIB_PATH


class LrFrame(C.Structure):
    _fields_ = [("count", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32), ("tile_count", C.c_uint32),
                ("visible", C.c_uint32), ("active_tiles", C.c_uint32), ("total_entries", C.c_uint32),
                ("max_tile_count", C.c_uint32), ("max_per_tile", C.c_uint32), ("overflow", C.c_uint32),
                ("mask", C.c_void_p), ("pre", C.c_void_p), ("projected", C.c_void_p), ("source", C.c_void_p),
                ("tile_counts", C.c_void_p), ("tile_lists", C.c_void_p), ("walked", C.c_void_p),
                ("color", C.c_void_p), ("depth", C.c_void_p)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        import oracle as O
        L = C.CDLL(build())
        L.lr_render.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                C.POINTER(O.OgCamera), C.c_uint32, C.c_uint32, C.c_int,
                                C.POINTER(C.POINTER(LrFrame))]
        L.lr_render.restype = C.c_int
        L.lr_frame_free.argtypes = [C.POINTER(LrFrame)]
        L.lr_sort_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.lr_sort_tiles.restype = C.c_int
        L.lr_compute_power.argtypes = [C.c_float]
        L.lr_compute_power.restype = C.c_float
        _lib = L
    return _lib


def render(world: np.ndarray, harmonics: np.ndarray, sh_components: int, camera: dict, width: int, height: int,
           max_gaussians: int | None = None, max_width: int | None = None, max_height: int | None = None,
           color_space: int = 0, nthreads: int = 0) -> dict:
    """One LocalRenderer frame (lr_render); every intermediate, the colour and the depth as numpy arrays."""
    import oracle as O
    L = lib()
    precision = 1 if world.dtype == O.WORLD16 else 0
    n = len(world)
    cfg = O.OgConfig(max_gaussians if max_gaussians is not None else max(n, 1), max_width or width,
                     max_height or height, precision, color_space)
    cam = O.dict_to_camera(camera)
    world = np.ascontiguousarray(world)
    harmonics = np.ascontiguousarray(harmonics)
    out = C.POINTER(LrFrame)()
    rc = L.lr_render(C.byref(cfg), world.ctypes.data if world.size else None,
                     harmonics.ctypes.data if harmonics.size else None, n, sh_components, C.byref(cam),
                     width, height, O._nthreads(nthreads), C.byref(out))
    if rc != 0:
        return {"status": rc}
    f = out.contents
    try:
        V, tc = f.visible, f.tile_count
        res = {
            "status": 0, "count": f.count, "tiles_x": f.tiles_x, "tiles_y": f.tiles_y, "tile_count": tc,
            "visible": V, "active_tiles": f.active_tiles, "total_entries": f.total_entries,
            "max_tile_count": f.max_tile_count, "max_per_tile": f.max_per_tile, "overflow": f.overflow,
            "mask": O._arr(f.mask, np.uint8, f.count),
            "pre": O._arr(f.pre, np.float32, f.count * 5).reshape(-1, 5),
            "projected": O._arr(f.projected, PROJECTED, V),
            "source": O._arr(f.source, np.int32, V),
            "tile_counts": O._arr(f.tile_counts, np.uint32, tc),
            "tile_lists": O._arr(f.tile_lists, np.uint32, tc * MAX_PER_TILE).reshape(tc, MAX_PER_TILE),
            "walked": O._arr(f.walked, np.uint32, tc),
            "color": O._arr(f.color, np.uint16, width * height * 4).reshape(height, width, 4),
            "depth": O._arr(f.depth, np.uint16, width * height).reshape(height, width),
        }
    finally:
        L.lr_frame_free(out)
    return res


def sort_tiles(keys16: np.ndarray, indices: np.ndarray, counts: np.ndarray, max_per_tile: int) -> np.ndarray:
    """lr_sort_tiles: per tile, the slots of the first min(count, max_per_tile) entries by (key, index, slot)."""
    keys16 = np.ascontiguousarray(keys16, np.uint16)
    indices = np.ascontiguousarray(indices, np.uint32)
    counts = np.ascontiguousarray(counts, np.uint32)
    out = np.zeros(len(counts) * max_per_tile, np.uint16)
    rc = lib().lr_sort_tiles(keys16.ctypes.data, indices.ctypes.data, counts.ctypes.data, len(counts),
                             max_per_tile, out.ctypes.data)
    assert rc == 0, rc
    return out
