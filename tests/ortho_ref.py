"""ctypes binding of the orthographic frames' checker (tests/ortho/ortho_ref.c; TEST INFRASTRUCTURE).

The C file includes gsm_global_render_frame's checker and, through it, the styled frames', the pick target's, the
composite's and the oracle's translation unit, so the shared library is rebuilt (gcc, the oracle's flags) whenever it
or one of those sources is newer.  __graft_entry__.build() builds it too.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import frame_ref as FR

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "ortho", "ortho_ref.c")
_LIB_PATH = os.path.join(_HERE, "ortho", "libortho_ref.so")
_DEPS = [_SRC, os.path.join(_HERE, "frame", "frame_ref.c"), os.path.join(_HERE, "style", "style_ref.c"),
         os.path.join(_HERE, "pick", "pick_ref.c"), os.path.join(_HERE, "compose", "compose_ref.c")] + \
    [os.path.join(_ROOT, "oracle", f) for f in ("gsm_oracle.c", "gsm_oracle.h", "gsm_oracle_math.h")]
# oracle/Makefile's flags: every fp op rounds on its own (DESIGN.md numeric contract)
_CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra",
           "-Wno-unused-function"]

PICK_NONE = FR.PICK_NONE
STYLE = FR.STYLE
style_table = FR.style_table
to_items = FR.to_items


def build(force: bool = False, src: str = _SRC, lib_path: str = _LIB_PATH) -> str:
    if force or not os.path.exists(lib_path) or os.path.getmtime(lib_path) < max(map(os.path.getmtime, _DEPS + [src])):
        tmp = lib_path + f".{os.getpid()}.tmp"
        subprocess.run([os.environ.get("CC", "gcc")] + _CFLAGS + ["-shared", "-o", tmp, src, "-lm", "-lpthread"],
                       check=True)
        os.replace(tmp, lib_path)
    return lib_path


_lib = None
_CrObject = None


def _bind(path):
    import oracle as O

    class CrObject(C.Structure):
        _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("camera", O.OgCamera)]

    L = C.CDLL(path)
    L.xr_render.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                            C.POINTER(CrObject), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                            C.c_uint32, C.c_int, C.c_int, C.POINTER(C.POINTER(O.OgFrame))]
    L.xr_render.restype = C.c_int
    L.cr_frame_free.argtypes = [C.POINTER(O.OgFrame)]
    L.fr_walk.argtypes = [C.POINTER(O.OgFrame), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_void_p, C.c_void_p]
    L.fr_walk.restype = C.c_long
    return L, CrObject


def lib():
    global _lib, _CrObject
    if _lib is None:
        _lib, _CrObject = _bind(build())
    return _lib


class Frame(FR.Frame):
    """A finished checker frame (xr_render): frame_ref.Frame -- walk(occluder) gives colour, depth, pick and items
    under an occluder or without one -- plus `data()`, every intermediate of the oracle's frame."""

    def data(self) -> dict:
        import oracle as O
        f = self._out.contents
        tot = f.total_assignments
        w, h = self.width, self.height
        return {
            "count": f.count, "tiles_x": f.tiles_x, "tiles_y": f.tiles_y, "tile_count": f.tile_count,
            "total_assignments": tot, "overflow": f.overflow, "visible": f.visible,
            "render_data": O._arr(f.render_data, O.RENDER_DATA, f.count),
            "bounds": O._arr(f.bounds, np.int32, f.count * 4).reshape(-1, 4),
            "mask": O._arr(f.mask, np.uint8, f.count),
            "tile_counts": O._arr(f.tile_counts, np.uint32, f.count),
            "keys": O._arr(f.keys, np.uint32, tot), "values": O._arr(f.values, np.int32, tot),
            "sorted_keys": O._arr(f.sorted_keys, np.uint32, tot),
            "sorted_values": O._arr(f.sorted_values, np.int32, tot),
            "headers": O._arr(f.headers, np.uint32, f.tile_count * 2).reshape(-1, 2),
            "color": O._arr(f.color, np.uint16, w * h * 4).reshape(h, w, 4),
            "depth": O._arr(f.depth, np.uint16, w * h).reshape(h, w),
        }


def frame(objects, sh_components: int, width: int, height: int, orthographic: bool = True, styles=None,
          max_gaussians: int | None = None, max_width: int | None = None, max_height: int | None = None,
          color_space: int = 0, nthreads: int = 0, _lib_override=None) -> Frame:
    """xr_render of [(world, harmonics, camera dict, state)] -- state a uint8 array of the object's count or an int;
    (world, harmonics, camera dict) for state 0 -- kept as a Frame.  orthographic: the frame's flag (False: the
    perspective rule through the same restated text).  styles: a STYLE array (None: the identity)."""
    import oracle as O
    L, Cr = _lib_override if _lib_override is not None else (lib(), _CrObject)
    objects = [tuple(o) + (0,) if len(o) == 3 else tuple(o) for o in objects]
    worlds = [np.ascontiguousarray(o[0]) for o in objects]
    harms = [np.ascontiguousarray(o[1]).reshape(-1) for o in objects]
    world, harm = np.concatenate(worlds), np.concatenate(harms)
    states = np.concatenate([np.full(len(w), o[3], np.uint8) if np.isscalar(o[3]) else
                             np.ascontiguousarray(o[3], dtype=np.uint8) for w, o in zip(worlds, objects)])
    n = len(world)
    assert len(states) == n
    styles = np.ascontiguousarray(FR.IDENTITY_TABLE if styles is None else styles, dtype=STYLE)
    cfg = O.OgConfig(max_gaussians if max_gaussians is not None else max(n, 1), max_width or width,
                     max_height or height, 1 if world.dtype == O.WORLD16 else 0, color_space)
    arr = (Cr * len(objects))()
    first, at = [], 0
    for a, w, o in zip(arr, worlds, objects):
        a.first, a.count, a.camera = at, len(w), O.dict_to_camera(o[2])
        first.append(at)
        at += len(w)
    out = C.POINTER(O.OgFrame)()
    rc = L.xr_render(C.byref(cfg), world.ctypes.data if world.size else None, harm.ctypes.data if harm.size else None,
                     n, sh_components, arr, len(objects), width, height, states.ctypes.data if n else None,
                     styles.ctypes.data, len(styles), 1 if orthographic else 0, O._nthreads(nthreads), C.byref(out))
    assert rc == 0, f"xr_render: {rc}"
    return Frame(L, out, width, height, first, [len(w) for w in worlds])


def render(world, harmonics, sh_components: int, camera: dict, width: int, height: int, orthographic: bool = True,
           **kw) -> dict:
    """One plain frame of one object: data() plus the unoccluded walk's "pick"."""
    with frame([(world, harmonics, camera)], sh_components, width, height, orthographic, **kw) as F:
        d = F.data()
        d["pick"] = F.walk()["pick"]
        return d
