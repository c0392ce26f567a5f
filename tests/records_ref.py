"""What gsm_global_render_records must compute from hand-made records, in plain numpy.

A frame here is a set of per-record arrays of fp16 bits, tile rects and tile masks (`Frame`).  This file
  * packs them as 48-byte SplatRecords (gsm_internal.h),
  * builds the per-tile lists the way the frame defines them (one entry per set mask bit, key
    tile << 16 | (depth bits ^ 0x8000), a stable sort, headers by searchsorted), and
  * restates the tile blend in numpy float16 -- a second derivation beside the C oracle's blend_tiles
    (oracle.blend_tiles), vectorised over a tile's 512 pixels, looping over its entries.
The half-tile skip flags are ignored: dropping an entry must never change a pixel.

numpy's float16 + - * compute in float32 and round once to nearest even: the correctly rounded fp16 operation
(24 >= 2 * 11 + 2), as the oracle's hadd / hsub / hmul.  The fused accumulate a * b + c is taken in float64 and
rounded once to float16 (`fma16`).  That is the correctly rounded fp16 fma: a * b is exact in float64 (22 bits);
the float64 sum can only round when one operand's last bit lies more than 53 bits below the other's first -- then
the small operand (<= 22 bits wide) lies more than 30 bits below the large one's first bit, far under its fp16
half ulp.  If the large operand is c it is an fp16 number and the sum rounds to c either way; if it is the product
its first bit is at least 2^29 (c's last bit is at least 2^-24) and both round to infinity.  test_records_ref.py
checks fma16 against og_hfma on the operands where a double rounding would show.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TILE_W, TILE_H, MASK_TILES = 32, 16, 32
F16, F32, F64 = np.float16, np.float32, np.float64

SPLAT_RECORD = np.dtype([("rd", "<u4", (4,)), ("ra", "<u4", (4,)), ("bounds", "<i2", (4,)), ("rb", "<u4"),
                         ("pad", "<u4")])
assert SPLAT_RECORD.itemsize == 48
FIELDS = ("mx", "my", "cxx", "cyy", "cxy2", "op", "cr", "cg", "cb", "dep")
BENDS = ("ties_reversed", "break_le", "no_zero_skip", "unfused", "key_no_xor")

_exp = None


def exp_table():
    """exp_h of every fp16 argument (tests/golden/exp_h_table.npy: the contract's table, indexed by the bits)"""
    global _exp
    if _exp is None:
        _exp = np.load(os.path.join(HERE, "golden", "exp_h_table.npy")).astype(np.uint16)
        assert _exp.shape == (65536,)
    return _exp


def h(x):
    """fp16 bits of a float (round to nearest even)"""
    return np.asarray(x, F64).astype(F16).view(np.uint16)


def f(bits):
    return np.asarray(bits, np.uint16).view(F16)


def unorm(k):
    """fp16(fp16(k) / 255): the 256 values a projected colour or opacity takes"""
    k = np.asarray(k)
    assert ((k >= 0) & (k <= 255)).all()
    return (k.astype(F16).astype(F32) / F32(255.0)).astype(F16).view(np.uint16)


def fma16(a, b, c):
    """fp16 a * b + c with one rounding (see the module docstring).  Which NaN comes out is stated here, not left
    to the host's arithmetic, the way the oracle's hfma has it (the product first, then the sum): a's bits if a is
    a NaN, else b's, else 0xFE00 for an invalid product (inf * 0), else c's, else 0xFE00 (inf - inf)."""
    with np.errstate(all="ignore"):
        r = (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F16)
        bad = np.isnan(r)
        if bad.any():
            a, b, c = (np.broadcast_to(v, r.shape) for v in (a, b, c))
            dflt = np.uint16(0xFE00)
            bits = np.where(np.isnan(a), a.view(np.uint16) | 0x0200,
                            np.where(np.isnan(b), b.view(np.uint16) | 0x0200,
                                     np.where(np.isnan(a.astype(F32) * b.astype(F32)), dflt,
                                              np.where(np.isnan(c), c.view(np.uint16) | 0x0200, dflt))))
            r = np.where(bad, bits.astype(np.uint16), r.view(np.uint16)).view(F16)
        return r


class Frame:
    """Records of one crafted frame.  width x height pixels on the renderer's grid of max_width x max_height."""

    def __init__(self, name, width, height, max_width=None, max_height=None):
        self.name, self.width, self.height = name, width, height
        self.max_width, self.max_height = max_width or width, max_height or height
        self.tiles_x = (self.max_width + TILE_W - 1) // TILE_W
        self.tiles_y = (self.max_height + TILE_H - 1) // TILE_H
        self.rows = []
        self.notes = {}  # what a case wants asserted about itself: tiles by role
        self._done = None

    def add(self, mx, my, cxx, cyy, cxy2=0.0, op=255, rgb=(255, 128, 64), dep=1.0, rect=None, mask=None,
            dep_bits=None):
        """one record: floats for mean / conic / depth (rounded to fp16), bytes for opacity and colour, rect
        (x0, x1, y0, y1) in tiles (default: the tile of the mean), mask over the rect (default: every tile)"""
        if rect is None:
            tx, ty = int(mx) // TILE_W, int(my) // TILE_H
            rect = (tx, tx, ty, ty)
        x0, x1, y0, y1 = rect
        area = (x1 - x0 + 1) * (y1 - y0 + 1)
        assert 0 <= x0 <= x1 < self.tiles_x and 0 <= y0 <= y1 < self.tiles_y and area <= MASK_TILES, rect
        full = (1 << area) - 1
        mask = full if mask is None else mask
        assert 0 <= mask <= full
        d = int(h(dep)) if dep_bits is None else int(dep_bits)
        vals = [int(h(v)) for v in (mx, my, cxx, cyy, cxy2)] + [int(unorm(v)) for v in (op,) + tuple(rgb)] + [d]
        self.rows.append(vals + list(rect) + [mask])
        self._done = None
        return len(self.rows) - 1

    def arrays(self):
        if self._done is None:
            a = np.array(self.rows, np.int64).reshape(-1, 15)
            d = {k: a[:, i].astype(np.uint16) for i, k in enumerate(FIELDS)}
            d["bounds"] = a[:, 10:14].astype(np.int16)
            d["mask"] = a[:, 14].astype(np.uint32)
            for k in ("mx", "my", "cxx", "cyy", "cxy2"):  # finite fp16
                assert np.isfinite(f(d[k]).astype(F32)).all(), k
            self._done = d
        return self._done

    @property
    def count(self):
        return len(self.rows)


def pack(frame):
    """SplatRecord[count]: rd (the mean word; the rest is only read for rects above 32 tiles), ra = mean,
    cxx | cyy, cxy2 | opacity, r | g; bounds as short4; rb = b | depth << 16; pad = the tile mask"""
    a = frame.arrays()
    u = {k: a[k].astype(np.uint32) for k in FIELDS}
    r = np.zeros(frame.count, SPLAT_RECORD)
    r["rd"][:, 0] = u["mx"] | (u["my"] << 16)
    r["rd"][:, 2] = u["dep"] << 16
    r["ra"][:, 0] = u["mx"] | (u["my"] << 16)
    r["ra"][:, 1] = u["cxx"] | (u["cyy"] << 16)
    r["ra"][:, 2] = u["cxy2"] | (u["op"] << 16)
    r["ra"][:, 3] = u["cr"] | (u["cg"] << 16)
    r["bounds"] = a["bounds"]
    r["rb"] = u["cb"] | (u["dep"] << 16)
    r["pad"] = a["mask"]
    return r


def blend_records(frame):
    """the records' blend values as the oracle's BLEND_REC rows (a plain structured array)"""
    a = frame.arrays()
    out = np.zeros(frame.count, np.dtype([(k, "<u2") for k in FIELDS]))
    for k in FIELDS:
        out[k] = a[k]
    return out


def assignments(frame, bend=None):
    """unsorted (keys, values) in slot order: ascending record, then the set mask bits in ascending order
    (bit = (ty - y0) * rw + (tx - x0): ty-major, tx-minor)"""
    a = frame.arrays()
    b = a["bounds"].astype(np.int64)
    rw = b[:, 1] - b[:, 0] + 1
    bits = np.arange(MASK_TILES, dtype=np.int64)
    on = ((a["mask"][:, None] >> bits[None, :].astype(np.uint32)) & 1).astype(bool)
    rec, bit = np.nonzero(on)  # row-major: ascending record, then ascending bit
    tx = b[rec, 0] + bit % rw[rec]
    ty = b[rec, 2] + bit // rw[rec]
    assert (tx <= b[rec, 1]).all() and (ty <= b[rec, 3]).all()
    tile = ty * frame.tiles_x + tx
    dep = a["dep"][rec].astype(np.int64)
    depth_field = dep if bend == "key_no_xor" else dep ^ 0x8000
    keys = ((tile << 16) | (depth_field & 0xFFFF)).astype(np.uint32)
    return keys, rec.astype(np.int32)


def sort_lists(keys, values, tile_count, bend=None):
    """sorted keys and values (stable: ties in ascending slot order) and headers {offset = lower bound, count}
    per tile (all zero for a frame without assignments, as the reference)"""
    order = np.argsort(keys, kind="stable")
    if bend == "ties_reversed":
        order = np.lexsort((-np.arange(keys.size), keys))
    sk, sv = keys[order], values[order]
    tiles = np.arange(tile_count, dtype=np.int64)
    lo = np.searchsorted(sk >> 16, tiles, "left")
    hi = np.searchsorted(sk >> 16, tiles, "right")
    headers = np.stack([lo, hi - lo], 1).astype(np.uint32)
    if keys.size == 0:
        headers[:] = 0
    return {"keys": keys, "values": values, "sorted_keys": sk, "sorted_values": sv, "headers": headers}


def lists(frame, bend=None):
    """the frame's per-tile lists"""
    keys, values = assignments(frame, bend)
    return sort_lists(keys, values, frame.tiles_x * frame.tiles_y, bend)


def tile_alphas(frame, tile, entries):
    """alpha bits [len(entries), 16, 32] of records `entries` at the pixels of `tile` (fp16 walk arithmetic)"""
    a = frame.arrays()
    tx, ty = tile % frame.tiles_x, tile // frame.tiles_x
    px = (np.arange(TILE_W) + tx * TILE_W).astype(F32).astype(F16)[None, None, :]
    py = (np.arange(TILE_H) + ty * TILE_H).astype(F32).astype(F16)[None, :, None]
    e = np.asarray(entries, np.int64)
    g = {k: f(a[k][e])[:, None, None] for k in ("mx", "my", "cxx", "cyy", "cxy2", "op")}
    with np.errstate(all="ignore"):
        dx, dy = px - g["mx"], py - g["my"]
        p = ((dx * dx) * g["cxx"] + (dy * dy) * g["cyy"]) + (dx * dy) * g["cxy2"]
        arg = (F32(-0.5) * p.astype(F32)).astype(F16)
        ex = exp_table()[arg.view(np.uint16)].view(F16)
        al = np.fmin(g["op"] * ex, F16(0.99))
    return al.view(np.uint16)


def blend(frame, L=None, bend=None):
    """the tile blend restated: colour [h, w, 4], depth [h, w] (fp16 bits) and group_iters [tiles, 8, 8]"""
    a = frame.arrays()
    L = lists(frame, bend) if L is None else L
    W, H = frame.width, frame.height
    color = np.zeros((H, W, 4), np.uint16)
    color[..., 3] = 0x3C00
    depth = np.zeros((H, W), np.uint16)
    iters = np.zeros((frame.tiles_x * frame.tiles_y, 8, 8), np.uint32)
    thr = (F32(1.0) / F32(255.0)).astype(F16)
    one = F16(1.0)
    col = {k: f(a[k]) for k in ("cr", "cg", "cb", "dep")}

    def groups(v):  # [16, 32] per pixel -> [8, 2, 8, 4]: group (ly, lx) holds pixels (2 ly + j, 4 lx + i)
        return v.reshape(8, 2, 8, 4)

    for tile in np.flatnonzero(L["headers"][:, 1]):
        start, count = (int(v) for v in L["headers"][tile])
        ids = L["sorted_values"][start:start + count]
        T = np.full((TILE_H, TILE_W), one, F16)
        C = np.zeros((3, TILE_H, TILE_W), F16)
        D = np.zeros((TILE_H, TILE_W), F16)
        alive = np.ones((8, 8), bool)
        it = np.full((8, 8), count, np.uint32)
        CH = 64
        for i in range(count):
            if i % CH == 0:
                al_chunk = tile_alphas(frame, tile, ids[i:i + CH]).view(F16)
            tmax = np.fmax.reduce(np.fmax.reduce(groups(T), axis=3), axis=1)
            dead = (tmax <= thr) if bend == "break_le" else (tmax < thr)
            newly = alive & dead
            it[newly] = i
            alive &= ~dead
            if not alive.any():
                break
            al = al_chunk[i % CH]
            anyg = (groups(al) != 0).any(axis=(1, 3))
            upd = alive if bend == "no_zero_skip" else (alive & anyg)
            if not upd.any():
                continue
            m = np.repeat(np.repeat(upd, 2, axis=0), 4, axis=1)
            g = int(ids[i])
            with np.errstate(all="ignore"):
                w = al * T
                if bend == "unfused":
                    nC = [col[k][g] * w + C[j] for j, k in enumerate(("cr", "cg", "cb"))]
                    nD = col["dep"][g] * w + D
                else:
                    nC = [fma16(np.broadcast_to(col[k][g], w.shape), w, C[j]) for j, k in enumerate(("cr", "cg", "cb"))]
                    nD = fma16(np.broadcast_to(col["dep"][g], w.shape), w, D)
                nT = T * (one - al)
            for j in range(3):
                C[j] = np.where(m, nC[j], C[j])
            D = np.where(m, nD, D)
            T = np.where(m, nT, T)
        iters[tile] = it
        tx, ty = tile % frame.tiles_x, tile // frame.tiles_x
        x0, y0 = tx * TILE_W, ty * TILE_H
        w_, h_ = min(TILE_W, W - x0), min(TILE_H, H - y0)
        if w_ <= 0 or h_ <= 0:
            continue
        for j in range(3):
            color[y0:y0 + h_, x0:x0 + w_, j] = C[j].view(np.uint16)[:h_, :w_]
        color[y0:y0 + h_, x0:x0 + w_, 3] = (one - T).view(np.uint16)[:h_, :w_]
        depth[y0:y0 + h_, x0:x0 + w_] = D.view(np.uint16)[:h_, :w_]
    return {"color": color, "depth": depth, "group_iters": iters}


# ---- the scatter's half-tile skip band, restated (band_skip_setup, band_rect_ok, half_skip_flags) ----
BLEND_ZERO_P = 34.65625


def coord_margin(c):
    return 0 if c < 2048 else (1 if c < 4096 else (2 if c < 8192 else -1))


def skip_band(frame, i):
    """(mean x, half width) of record i's skip band, or None where the scatter may not use one: float32
    arithmetic in the kernel's order, numpy's correctly rounded 1/x, sqrt for the hardware's ~1 ulp ones -- a
    model of which entries get flagged, good for counting them, not a bit-exact copy"""
    a = frame.arrays()
    mx, my, cxx, cyy, cxy = (F32(f(a[k][i])) for k in ("mx", "my", "cxx", "cyy", "cxy2"))
    lim = F32(65504.0)
    if not (cxx > 0 and cyy > 0 and cxx < lim and cyy < lim and abs(cxy) < lim and abs(mx) < lim and abs(my) < lim):
        return None
    with np.errstate(all="ignore"):
        rho = F32(0.5) * abs(cxy) / np.sqrt(cxx * cyy, dtype=F32)
        if not rho <= F32(15.0 / 16.0):
            return None
        u = F32(1.0 / 2048.0)
        factor = (F32(1) - u) * (F32(1) - F32(10) * u / (F32(1) - rho)) * (F32(1) - F32(1e-5))
        Lp = (F32(BLEND_ZERO_P) + F32(1e-3)) / factor * (F32(1) + F32(1e-5))
        det = cxx * cyy - F32(0.25) * cxy * cxy
        if not det > 0:
            return None
        ex = np.sqrt(Lp * cyy / det, dtype=F32) * (F32(1) + F32(1e-5)) + F32(1e-4)
    if not np.isfinite(ex):
        return None
    x0t, x1t, y0t, y1t = (int(v) for v in a["bounds"][i])
    x0, x1, y0, y1 = x0t * TILE_W, x1t * TILE_W + TILE_W - 1, y0t * TILE_H, y1t * TILE_H + TILE_H - 1
    mxm, mym = coord_margin(x1), coord_margin(y1)
    if mxm < 0 or mym < 0:
        return None
    ax = max(abs(F32(x0 - mxm) - mx), abs(F32(x1 + mxm) - mx))
    ay = max(abs(F32(y0 - mym) - my), abs(F32(y1 + mym) - my))
    if not (ax <= 200 and ay <= 200 and cxx * (ax * ax) + cyy * (ay * ay) <= 16000):
        return None
    return float(mx), float(ex)


def half_skip_flags(band, tx):
    """(left half flagged, right half flagged) of tile column tx for a band"""
    if band is None:
        return False, False
    mx, ex = F32(band[0]), F32(band[1])
    x0, hw = tx * TILE_W, TILE_W // 2
    m0, m1 = coord_margin(x0 + hw - 1), coord_margin(x0 + 2 * hw - 1)
    left = F32(x0 - m0) - mx > ex or F32(x0 + hw - 1 + m0) - mx < -ex
    right = F32(x0 + hw - m1) - mx > ex or F32(x0 + 2 * hw - 1 + m1) - mx < -ex
    return bool(left), bool(right)


def reference(frame, oracle):
    """the frame's lists and the oracle's blend of them, computed once per frame and read-only from then on"""
    if getattr(frame, "_ref", None) is None:
        L = lists(frame)
        o = oracle.blend_tiles(blend_records(frame), L["headers"], L["sorted_values"], frame.tiles_x, frame.tiles_y,
                               frame.width, frame.height)
        ref = dict(L, **o)
        for v in ref.values():
            v.setflags(write=False)
        frame._ref = ref
    return frame._ref


def canonical_nans(bits):
    """fp16 bits with every NaN as 0x7E00: the NaN a sum of two different NaNs keeps is the host's choice"""
    b = np.asarray(bits, np.uint16)
    return np.where((b & 0x7FFF) > 0x7C00, np.uint16(0x7E00), b)


def explain_pixel(frame, ref, y, x, got_pixel):
    """where a differing pixel sits and what the reference did there: tile, half-tile and quadrant unit, 4x2 group,
    the list's length and the group's break, the list positions whose alpha is nonzero at the pixel, those of a
    non-finite depth, and -- walking the group's 8 pixels alone -- after how many entries the reference held the
    value `got_pixel` (r, g, b, a, depth bits), if ever: the entry a walk stopped at or dropped"""
    tx, ty = x // TILE_W, y // TILE_H
    tile = ty * frame.tiles_x + tx
    lx, ly = (x % TILE_W) // 4, (y % TILE_H) // 2
    s, c = (int(v) for v in ref["headers"][tile])
    ids = ref["sorted_values"][s:s + c]
    a = frame.arrays()
    msg = ["pixel (x %d, y %d): tile %d (%d, %d), half %d, quadrant %d, group (lx %d, ly %d), list %d entries, "
           "group break at %d" % (x, y, tile, tx, ty, (x % TILE_W) // 16, ((y % TILE_H) // 8) * 2 + (x % TILE_W) // 16,
                                  lx, ly, c, int(ref["group_iters"][tile, ly, lx]))]
    if c == 0:
        return msg[0]
    al = tile_alphas(frame, tile, ids).view(F16)
    grp = al[:, 2 * ly:2 * ly + 2, 4 * lx:4 * lx + 4].reshape(c, 8)
    q = (y % 2) * 4 + x % 4
    nz = np.flatnonzero(grp[:, q] != 0)
    msg.append("nonzero alpha at the pixel at list positions %s%s" % (nz[:12].tolist(), " ..." if nz.size > 12 else ""))
    nf = np.flatnonzero((a["dep"][ids] & 0x7C00) == 0x7C00)
    msg.append("non-finite depths at list positions %s" % nf[:12].tolist())
    thr, one = (F32(1.0) / F32(255.0)).astype(F16), F16(1.0)
    T, C, D = np.full(8, one, F16), np.zeros((3, 8), F16), np.zeros(8, F16)
    held = []
    want = [int(v) for v in got_pixel]

    def now():
        return [int(C[j].view(np.uint16)[q]) for j in range(3)] + [int((one - T).view(np.uint16)[q]),
                                                                   int(D.view(np.uint16)[q])]
    if now()[:len(want)] == want:
        held.append(0)
    for i in range(c):
        if np.fmax.reduce(T) < thr:
            break
        if (grp[i] != 0).any():
            g = int(ids[i])
            with np.errstate(all="ignore"):
                w = grp[i] * T
                for j, k in enumerate(("cr", "cg", "cb")):
                    C[j] = fma16(np.broadcast_to(f(a[k][g]), w.shape), w, C[j])
                D = fma16(np.broadcast_to(f(a["dep"][g]), w.shape), w, D)
                T = T * (one - grp[i])
        if now()[:len(want)] == want:
            held.append(i + 1)
    msg.append("the reference held the got value after %s entries" % (held[:6] if held else "no number of"))
    return "; ".join(msg)
