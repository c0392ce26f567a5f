"""ctypes binding of gsm_global_render_frame's checker (tests/frame/frame_ref.c; TEST INFRASTRUCTURE), and the numpy
restatement of gsm_global_select_pick.

The C file includes the styled frames' checker and, through it, the pick target's, the composite's and the oracle's
translation unit, so the shared library is rebuilt (gcc, the oracle's flags) whenever it or one of those sources is
newer.  __graft_entry__.build() builds it too.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "frame", "frame_ref.c")
_LIB_PATH = os.path.join(_HERE, "frame", "libframe_ref.so")
_DEPS = [_SRC, os.path.join(_HERE, "style", "style_ref.c"), os.path.join(_HERE, "pick", "pick_ref.c"),
         os.path.join(_HERE, "compose", "compose_ref.c")] + \
    [os.path.join(_ROOT, "oracle", f) for f in ("gsm_oracle.c", "gsm_oracle.h", "gsm_oracle_math.h")]
# oracle/Makefile's flags: every fp op rounds on its own (DESIGN.md numeric contract)
_CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra",
           "-Wno-unused-function"]

PICK_NONE = 0xFFFFFFFF
# gsm_global_style / sr_style
STYLE = np.dtype([("tint_r", "u1"), ("tint_g", "u1"), ("tint_b", "u1"), ("tint_amount", "u1"),
                  ("opacity_scale", "u1"), ("hidden", "u1"), ("pad", "u1", (2,))])
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
        L.sr_render.argtypes = [C.POINTER(O.OgConfig), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                C.POINTER(CrObject), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                C.c_uint32, C.c_int, C.POINTER(C.POINTER(O.OgFrame))]
        L.sr_render.restype = C.c_int
        L.cr_frame_free.argtypes = [C.POINTER(O.OgFrame)]
        L.fr_walk.argtypes = [C.POINTER(O.OgFrame), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]
        L.fr_walk.restype = C.c_long
        _CrObject = CrObject
        _lib = L
    return _lib


def style_table(styles) -> np.ndarray:
    """A STYLE array of [(tint_r, tint_g, tint_b, tint_amount, opacity_scale, hidden)]."""
    t = np.zeros(len(styles), STYLE)
    for d, s in zip(t, styles):
        d["tint_r"], d["tint_g"], d["tint_b"], d["tint_amount"], d["opacity_scale"], d["hidden"] = s
    return t


IDENTITY_TABLE = style_table([(0, 0, 0, 0, 255, 0)])


class Frame:
    """A finished checker frame (sr_render) kept alive so that several occluders can be walked over it."""

    def __init__(self, L, out, width, height, first, counts):
        import oracle as O
        self._L, self._out, self.width, self.height = L, out, width, height
        self.first, self.counts = first, counts
        f = out.contents
        self.tiles_x = f.tiles_x
        self.headers = O._arr(f.headers, np.uint32, f.tile_count * 2).reshape(-1, 2)
        self.count = f.count
        self.overflow = f.overflow
        self.sorted_values = O._arr(f.sorted_values, np.int32, f.total_assignments)

    def walk(self, occluder=None) -> dict:
        """fr_walk under `occluder` (a float32 array of shape (H, W), any row stride; None: nothing occluded).
        Returns "color", "depth", "pick" (the frame's ids: concatenated over the objects), "items" (the composite
        layout's items, what the pick target holds), "closed" (bool per pixel) and "records"."""
        f = self._out.contents
        w, h = self.width, self.height
        occ = None
        if occluder is not None:
            occ = np.asarray(occluder)
            assert occ.dtype == np.float32 and occ.shape == (h, w) and occ.strides[1] == 4 and occ.strides[0] % 4 == 0
        color = np.zeros((h, w, 4), np.uint16)
        depth = np.zeros((h, w), np.uint16)
        pick = np.zeros((h, w), np.uint32)
        closed = np.zeros((h, w), np.uint8)
        records = np.zeros((max(f.count, 1), len(RECORD_FIELDS)), np.uint16)
        rc = self._L.fr_walk(self._out, occ.ctypes.data if occ is not None else None,
                             occ.strides[0] // 4 if occ is not None else 0, color.ctypes.data, depth.ctypes.data,
                             pick.ctypes.data, closed.ctypes.data, records.ctypes.data)
        assert rc == 0, "fr_walk failed"
        return {"color": color, "depth": depth, "pick": pick, "items": to_items(pick, self.first, self.counts),
                "closed": closed != 0, "records": records[:f.count]}

    def active_pixels(self) -> np.ndarray:
        """(H, W) bool: the pixels of tiles that have list entries."""
        h, w = self.height, self.width
        tiles = (np.arange(h)[:, None] // 16) * self.tiles_x + np.arange(w)[None, :] // 32
        return self.headers[:, 1][tiles] > 0

    def close(self):
        if self._out is not None:
            self._L.cr_frame_free(self._out)
            self._out = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def to_items(pick, first, counts) -> np.ndarray:
    """Concatenated ids -> items of the composite layout (include/gsm_renderer.h): object o's items start at
    256 * B_o, B_o = sum over u < o of ceil(count_u / 256).  PICK_NONE stays."""
    pick = np.asarray(pick, np.uint32)
    out = np.full(pick.shape, PICK_NONE, np.uint32)
    block = 0
    for f0, n in zip(first, counts):
        sel = (pick != PICK_NONE) & (pick >= f0) & (pick < f0 + n)
        out[sel] = pick[sel] - np.uint32(f0) + np.uint32(256 * block)
        block += (n + 255) // 256
    return out


def frame(objects, sh_components: int, width: int, height: int, styles=None, max_gaussians: int | None = None,
          max_width: int | None = None, max_height: int | None = None, color_space: int = 0,
          nthreads: int = 0) -> Frame:
    """sr_render of [(world, harmonics, camera dict, state)] -- state a uint8 array of the object's count or an int;
    (world, harmonics, camera dict) for state 0 -- kept as a Frame.  styles: a STYLE array (None: the identity, the
    unstyled frame)."""
    import oracle as O
    L = lib()
    objects = [tuple(o) + (0,) if len(o) == 3 else tuple(o) for o in objects]
    worlds = [np.ascontiguousarray(o[0]) for o in objects]
    harms = [np.ascontiguousarray(o[1]).reshape(-1) for o in objects]
    world, harm = np.concatenate(worlds), np.concatenate(harms)
    states = np.concatenate([np.full(len(w), o[3], np.uint8) if np.isscalar(o[3]) else
                             np.ascontiguousarray(o[3], dtype=np.uint8) for w, o in zip(worlds, objects)])
    n = len(world)
    assert len(states) == n
    styles = np.ascontiguousarray(IDENTITY_TABLE if styles is None else styles, dtype=STYLE)
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
    assert rc == 0, f"sr_render: {rc}"
    return Frame(L, out, width, height, first, [len(w) for w in worlds])


def select_pick(items, mask, base: int, count: int, state, gaussian_count: int, and_mask: int, xor_mask: int):
    """gsm_global_select_pick's set rule from its contract, in numpy.  items: the (H, W) pick image; mask: (H, >= W)
    uint8 or None; base = 256 * B_object and count = count_object of the pick frame's layout.  S = the ids
    item - base of the pixels under the mask whose item lies in [base, base + min(count, gaussian_count)); every id of
    S is updated once.  Returns (new state, |S|)."""
    items = np.asarray(items, np.uint32)
    h, w = items.shape
    under = np.ones((h, w), bool) if mask is None else np.asarray(mask)[:h, :w] != 0
    n = min(int(count), int(gaussian_count))
    it = items[under].astype(np.int64)
    ids = np.unique(it[(it >= base) & (it < base + n)] - base)
    out = np.asarray(state, np.uint8).copy()
    out[ids] = ((out[ids].astype(np.uint32) & (and_mask & 0xFFFFFFFF)) ^ (xor_mask & 0xFFFFFFFF)) & 0xFF
    return out, int(len(ids))
