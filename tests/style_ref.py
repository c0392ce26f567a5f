"""ctypes binding of the styled frames' checker (tests/style/style_ref.c; TEST INFRASTRUCTURE), and the numpy
reference of gsm_global_select_mask.

The C file includes the pick target's checker and, through it, the composite's and the oracle's translation unit,
so the shared library is rebuilt (gcc, the oracle's flags) whenever it or one of those sources is newer.
__graft_entry__.build() builds it too.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "style", "style_ref.c")
_LIB_PATH = os.path.join(_HERE, "style", "libstyle_ref.so")
_DEPS = [_SRC, os.path.join(_HERE, "pick", "pick_ref.c"), os.path.join(_HERE, "compose", "compose_ref.c")] + \
    [os.path.join(_ROOT, "oracle", f) for f in ("gsm_oracle.c", "gsm_oracle.h", "gsm_oracle_math.h")]
# oracle/Makefile's flags: every fp op rounds on its own (DESIGN.md numeric contract)
_CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra",
           "-Wno-unused-function"]

PICK_NONE = 0xFFFFFFFF
# gsm_global_style / sr_style
STYLE = np.dtype([("tint_r", "u1"), ("tint_g", "u1"), ("tint_b", "u1"), ("tint_amount", "u1"),
                  ("opacity_scale", "u1"), ("hidden", "u1"), ("pad", "u1", (2,))])
IDENTITY = (0, 0, 0, 0, 255, 0, (0, 0))


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
        L.sr_render.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                C.POINTER(CrObject), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                C.c_uint32, C.c_int, C.POINTER(C.POINTER(O.OgFrame))]
        L.sr_render.restype = C.c_int
        L.cr_frame_free.argtypes = [C.POINTER(O.OgFrame)]
        L.pr_pick.argtypes = [C.POINTER(O.OgFrame), C.c_void_p, C.c_void_p, C.c_void_p]
        L.pr_pick.restype = C.c_long
        L.sr_tint.argtypes = [C.c_uint32] * 3
        L.sr_tint.restype = C.c_uint32
        L.sr_fade.argtypes = [C.c_uint32] * 2
        L.sr_fade.restype = C.c_uint32
        _CrObject = CrObject
        _lib = L
    return _lib


def style_table(styles) -> np.ndarray:
    """A STYLE array of [(tint_r, tint_g, tint_b, tint_amount, opacity_scale, hidden)]."""
    t = np.zeros(len(styles), STYLE)
    for d, s in zip(t, styles):
        d["tint_r"], d["tint_g"], d["tint_b"], d["tint_amount"], d["opacity_scale"], d["hidden"] = s
    return t


def render_composite(objects, sh_components: int, width: int, height: int, styles: np.ndarray,
                     max_gaussians: int | None = None, max_width: int | None = None, max_height: int | None = None,
                     color_space: int = 0, nthreads: int = 0) -> dict:
    """sr_render of [(world, harmonics, camera dict, state)] -- state a uint8 array of the object's count or an int
    (every gaussian's state) -- then pr_pick.  Returns every intermediate of the oracle's frame (ids = concatenated
    ids), colour and depth, "pick", "differ" (must be 0), "first" and "counts"."""
    import oracle as O
    L = lib()
    worlds = [np.ascontiguousarray(o[0]) for o in objects]
    harms = [np.ascontiguousarray(o[1]).reshape(-1) for o in objects]
    world, harm = np.concatenate(worlds), np.concatenate(harms)
    states = np.concatenate([np.full(len(w), o[3], np.uint8) if np.isscalar(o[3]) else
                             np.ascontiguousarray(o[3], dtype=np.uint8) for w, o in zip(worlds, objects)])
    n = len(world)
    assert len(states) == n
    styles = np.ascontiguousarray(styles, dtype=STYLE)
    cfg = O.OgConfig(max_gaussians if max_gaussians is not None else max(n, 1), max_width or width,
                     max_height or height, 1 if world.dtype == O.WORLD16 else 0, color_space)
    arr = (_CrObject * len(objects))()
    first, at = [], 0
    for a, w, o in zip(arr, worlds, objects):
        a.first, a.count, a.camera = at, len(w), O.dict_to_camera(o[2])
        first.append(at)
        at += len(w)
    out = C.POINTER(O.OgFrame)()
    rc = L.sr_render(C.byref(cfg), world.ctypes.data if world.size else None, harm.ctypes.data if harm.size else None,
                     n, sh_components, arr, len(objects), width, height, states.ctypes.data if n else None,
                     styles.ctypes.data, len(styles), O._nthreads(nthreads), C.byref(out))
    if rc != 0:
        return {"status": rc}
    f = out.contents
    try:
        tot = f.total_assignments
        pick = np.zeros((height, width), np.uint32)
        differ = int(L.pr_pick(out, pick.ctypes.data, None, None))
        return {
            "status": 0, "count": f.count, "first": first, "counts": [len(w) for w in worlds],
            "tiles_x": f.tiles_x, "tiles_y": f.tiles_y, "tile_count": f.tile_count,
            "total_assignments": tot, "overflow": f.overflow, "visible": f.visible, "active_tiles": f.active_tiles,
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
            "differ": differ, "pick": pick, "states": states,
        }
    finally:
        L.cr_frame_free(out)


def render(world, harmonics, sh_components: int, camera: dict, width: int, height: int, state, styles, **kw) -> dict:
    """The single styled frame: render_composite of one object."""
    return render_composite([(world, harmonics, camera, state)], sh_components, width, height, styles, **kw)


def select_mask(render_data, visible, width: int, height: int, mask, state, and_mask: int, xor_mask: int,
                styles=None):
    """gsm_global_select_mask from its contract, in numpy, over the oracle's render_data and mask of the PLAIN
    frame (oracle.render: `visible` is its "mask").  mask: (height, >= width) uint8.  Returns (new state, matched).
    styles: a STYLE array or None."""
    state = np.asarray(state, np.uint8)
    n = len(render_data)
    match = np.asarray(visible[:n]) == 1
    if styles is not None:
        hidden = np.zeros(256, bool)
        hidden[:len(styles)] = np.asarray(styles)["hidden"] != 0
        match &= ~hidden[state[:n]]
    with np.errstate(invalid="ignore", over="ignore"):
        mx = render_data["meanX"].view(np.float16).astype(np.float64)
        my = render_data["meanY"].view(np.float16).astype(np.float64)
        match &= np.isfinite(mx) & np.isfinite(my)
        px, py = np.floor(mx + 0.5), np.floor(my + 0.5)
        inside = (px >= 0) & (px < width) & (py >= 0) & (py < height)
    match &= inside
    ix, iy = np.where(match, px, 0).astype(np.int64), np.where(match, py, 0).astype(np.int64)
    match &= np.asarray(mask)[iy, ix] != 0
    out = state.copy()
    sel = np.nonzero(match)[0]
    out[sel] = ((state[sel].astype(np.uint32) & (and_mask & 0xFFFFFFFF)) ^ (xor_mask & 0xFFFFFFFF)) & 0xFF
    return out, int(match.sum())
