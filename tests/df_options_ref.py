"""ctypes binding of the DepthFirst options restatement (tests/df_options/df_options_ref.c; TEST INFRASTRUCTURE).

The C file includes tests/df_mono/df_mono_ref.c and through it the oracle's translation unit, so the
shared library is rebuilt (gcc, the oracle's flags) whenever it or one of those sources is newer.
__graft_entry__.build() builds it too.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "df_options", "df_options_ref.c")
_LIB_PATH = os.path.join(_HERE, "df_options", "libdf_options_ref.so")
_DEPS = [_SRC, os.path.join(_HERE, "df_mono", "df_mono_ref.c")] + \
    [os.path.join(_ROOT, "oracle", f) for f in ("gsm_oracle.c", "gsm_oracle.h", "gsm_oracle_math.h")]
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


def lib():
    global _lib
    if _lib is None:
        import oracle as O
        from df_mono_ref import DfmFrame
        L = C.CDLL(build())
        L.dfo_render_stereo.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                        C.POINTER(O.OgCamera), C.POINTER(O.OgCamera), C.c_void_p, C.c_uint32,
                                        C.c_uint32, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.POINTER(O.OgDfFrame)), C.POINTER(C.c_void_p)]
        L.dfo_render_stereo.restype = C.c_int
        L.dfo_render_mono.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.POINTER(O.OgCamera), C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.POINTER(DfmFrame)), C.POINTER(C.c_void_p)]
        L.dfo_render_mono.restype = C.c_int
        L.og_df_frame_free.argtypes = [C.POINTER(O.OgDfFrame)]
        L.dfm_frame_free.argtypes = [C.POINTER(DfmFrame)]
        L.dfo_free_keys.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _arr(ptr, dtype, n):
    """One copy out of the C buffer (the 8224 x 4096 target is 270 MB)."""
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n).copy()


def _common(f, V, tot, rd_dtype):
    return {
        "status": 0, "count": f.count, "tiles_x": f.tiles_x, "tiles_y": f.tiles_y,
        "tile_count": f.tile_count, "max_instances": f.max_instances, "visible": V,
        "total_instances": tot, "overflow": f.overflow, "active_tiles": f.active_tiles,
        "render_data": _arr(f.render_data, rd_dtype, f.count),
        "bounds": _arr(f.bounds, np.int32, f.count * 4).reshape(-1, 4),
        "touched": _arr(f.touched, np.uint32, f.count),
        "depth_keys": _arr(f.depth_keys, np.uint32, f.count),
        "depth_order": _arr(f.depth_order, np.int32, V),
        "inst_tiles": _arr(f.inst_tiles, np.uint32, tot),
        "inst_gids": _arr(f.inst_gids, np.int32, tot),
        "headers": _arr(f.headers, np.uint32, f.tile_count * 2).reshape(-1, 2),
    }


def render_stereo(world: np.ndarray, harmonics: np.ndarray, sh_components: int, left: dict, right: dict,
                  width: int, height: int, depth_key_bits: int = 32, tile_id_bits: int = 16, scene_transform=None,
                  max_gaussians: int | None = None, max_width: int | None = None, max_height: int | None = None,
                  color_space: int = 0, nthreads: int = 0, count: int | None = None,
                  eye_color: bool = True) -> dict:
    """One stereo side-by-side frame (dfo_render_stereo): the fields of oracle.df_render_stereo plus
    "sorted_keys", the compacted depth keys as the depth sort left them."""
    import oracle as O
    L = lib()
    precision = 1 if world.dtype == O.WORLD16 else 0
    n = len(world) if count is None else count
    cfg = O.OgConfig(max_gaussians if max_gaussians is not None else max(n, 1), max_width or width,
                     max_height or height, precision, color_space)
    cl, cr = O.dict_to_camera(left), O.dict_to_camera(right)
    world = np.ascontiguousarray(world)
    harmonics = np.ascontiguousarray(harmonics)
    st = None
    if scene_transform is not None:
        st = np.ascontiguousarray(np.asarray(scene_transform, np.float32).reshape(16))
    out = C.POINTER(O.OgDfFrame)()
    keys = C.c_void_p()
    rc = L.dfo_render_stereo(C.byref(cfg), world.ctypes.data if world.size else None,
                             harmonics.ctypes.data if harmonics.size else None, n, sh_components,
                             C.byref(cl), C.byref(cr), st.ctypes.data if st is not None else None,
                             width, height, O._nthreads(nthreads), depth_key_bits, tile_id_bits,
                             C.byref(out), C.byref(keys))
    if rc != 0:
        return {"status": rc}
    f = out.contents
    try:
        res = _common(f, f.visible, f.total_instances, O.STEREO_RENDER_DATA)
        res["sorted_keys"] = _arr(keys.value, np.uint32, f.visible)
        if eye_color:
            res["eye_color"] = _arr(f.eye_color, np.uint16, 2 * width * height * 4).reshape(2, height, width, 4)
        res["color"] = _arr(f.color, np.uint16, 2 * width * height * 4).reshape(height, 2 * width, 4)
    finally:
        L.og_df_frame_free(out)
        L.dfo_free_keys(keys)
    return res


def render_mono(world: np.ndarray, harmonics: np.ndarray, sh_components: int, camera: dict, width: int,
                height: int, depth_key_bits: int = 32, tile_id_bits: int = 16,
                max_gaussians: int | None = None, max_width: int | None = None, max_height: int | None = None,
                color_space: int = 0, nthreads: int = 0) -> dict:
    """One mono frame (dfo_render_mono): the fields of df_mono_ref.render plus "sorted_keys"."""
    import oracle as O
    from df_mono_ref import DfmFrame
    L = lib()
    precision = 1 if world.dtype == O.WORLD16 else 0
    n = len(world)
    cfg = O.OgConfig(max_gaussians if max_gaussians is not None else max(n, 1), max_width or width,
                     max_height or height, precision, color_space)
    cam = O.dict_to_camera(camera)
    world = np.ascontiguousarray(world)
    harmonics = np.ascontiguousarray(harmonics)
    out = C.POINTER(DfmFrame)()
    keys = C.c_void_p()
    rc = L.dfo_render_mono(C.byref(cfg), world.ctypes.data if world.size else None,
                           harmonics.ctypes.data if harmonics.size else None, n, sh_components, C.byref(cam),
                           width, height, O._nthreads(nthreads), depth_key_bits, tile_id_bits,
                           C.byref(out), C.byref(keys))
    if rc != 0:
        return {"status": rc}
    f = out.contents
    try:
        res = _common(f, f.visible, f.total_instances, O.RENDER_DATA)
        res["sorted_keys"] = _arr(keys.value, np.uint32, f.visible)
        res["color"] = _arr(f.color, np.uint16, width * height * 4).reshape(height, width, 4)
        res["depth"] = _arr(f.depth, np.uint16, width * height).reshape(height, width)
    finally:
        L.dfm_frame_free(out)
        L.dfo_free_keys(keys)
    return res
