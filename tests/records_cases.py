"""Crafted SplatRecord frames for gsm_global_render_records: every case is a function of the
frame geometry that returns a records_ref.Frame whose `notes` name the tiles each property is asserted on
(test_records_ref.py asserts them from the reference's alphas and group_iters, without a device).

Every record: a rect of at most 32 tiles inside the grid, full tile rows, colour and opacity from the 256 values
fp16(fp16(k) / 255), finite fp16 mean and conic.

The shapes the records are made of (X, Y: a tile's first pixel):
  flat    conic 2^-24 (the smallest fp16): alpha = min(opacity, 0.99) wherever |dx|, |dy| < 256, and 0 where
          a squared distance overflows fp16 (inf * 2^-24 = inf: the table's 0)
  column  cxx = 64, cyy = 0: alpha 0 but in pixel column mx (p = 64 > 34.65625 one pixel away)
  row     cyy = 64, cxx = 0: alpha 0 but in pixel row my
  point   cxx = cyy = 64: one pixel
Opacity 255 gives alpha 0.99: two such entries leave T = fp16(1 - 0.99)^2 < 1/255, so a pixel is saturated after
its second one and a 4x2 group breaks at the entry after the last of its 8 pixels got its second.
"""
import numpy as np

import records_ref as R

TINY = 2.0 ** -24
THR = float(np.float16(np.float32(1.0) / np.float32(255.0)))
LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
PREFIXES = (15, 16, 17, 31, 32, 33, 63, 64, 65)
NONFINITE_POSITIONS = (0, 1, 63, 64, 69)  # of a 70-entry list; 69: last
# name -> (width, height, max_width, max_height): neither size a multiple of 32 / 16 nor of 4 / 2.  `small` has
# 88 tiles (quadrant units on any device with 11 compute units or more), `wide` 2176 (half-tile units up to 271)
GEOMETRIES = {"small": (333, 117, 333, 117), "wide": (4093, 267, 4096, 272)}
TINY_SHAPES = ((1, 1), (3, 1), (5, 3), (33, 17), (63, 31), (65, 33))


def new_frame(name, geo):
    w, h, mw, mh = GEOMETRIES[geo] if isinstance(geo, str) else geo
    fr = R.Frame("%s/%s" % (name, geo if isinstance(geo, str) else "%dx%d" % (w, h)), w, h, mw, mh)
    fr.geo = geo
    return fr


class Tiles:
    """hands out distinct tiles: the grid's corners first (the last column and row are partial tiles), then a
    stride through the grid; low=True only tiles whose pixels lie below x = 2048 (exact fp16 coordinates)"""

    def __init__(self, fr):
        self.fr, self.used = fr, set()
        tx, ty = fr.tiles_x, fr.tiles_y
        self.first = [(tx - 1, ty - 1), (0, 0), (tx - 1, 0), (0, ty - 1)]
        self.i = 0

    def take(self, low=False):
        fr = self.fr
        while self.first:
            t = self.first.pop(0)
            if t not in self.used and not (low and t[0] >= 64):
                self.used.add(t)
                return t
        n = fr.tiles_x * fr.tiles_y
        for _ in range(n):
            self.i = (self.i + 37) % n  # (37 is coprime to 88 and to 2176)
            t = (self.i % fr.tiles_x, self.i // fr.tiles_x)
            if t not in self.used and not (low and t[0] >= 64):
                self.used.add(t)
                return t
        raise AssertionError("out of tiles")


def tile_id(fr, t):
    return t[1] * fr.tiles_x + t[0]


def depth_bits(n):
    """the n-th positive fp16 from 1.0 up: ascending n is ascending depth"""
    assert 0 <= n < 0x7BFF - 0x3C00
    return 0x3C00 + n


def colour(rng):
    return tuple(int(v) for v in rng.integers(0, 256, 3))


def flat(fr, t, op, rgb, dep_bits, rect=None, mask=None, conic=TINY):
    r = rect or (t[0], t[0], t[1], t[1])
    mx = (r[0] + r[1] + 1) * R.TILE_W // 2
    my = (r[2] + r[3] + 1) * R.TILE_H // 2
    return fr.add(mx, my, conic, conic, 0.0, op, rgb, rect=r, mask=mask, dep_bits=dep_bits)


def column(fr, t, x, op, rgb, dep_bits):
    return fr.add(t[0] * 32 + x, t[1] * 16 + 8, 64.0, 0.0, 0.0, op, rgb, rect=(t[0], t[0], t[1], t[1]),
                  dep_bits=dep_bits)


def row(fr, t, y, op, rgb, dep_bits):
    return fr.add(t[0] * 32 + 16, t[1] * 16 + y, 0.0, 64.0, 0.0, op, rgb, rect=(t[0], t[0], t[1], t[1]),
                  dep_bits=dep_bits)


def point(fr, t, x, y, op, rgb, dep_bits):
    return fr.add(t[0] * 32 + x, t[1] * 16 + y, 64.0, 64.0, 0.0, op, rgb, rect=(t[0], t[0], t[1], t[1]),
                  dep_bits=dep_bits)


# ---- list lengths ----
def case_lengths(geo):
    fr = new_frame("lengths", geo)
    rng = np.random.default_rng(1)
    T = Tiles(fr)
    fr.notes["length"] = {}
    for n in LENGTHS:
        t = T.take()
        fr.notes["length"][tile_id(fr, t)] = n
        for d in rng.permutation(n):  # record order is not depth order
            flat(fr, t, 1 + int(d) % 3, colour(rng), depth_bits(int(d)))
    return fr


# ---- saturation position ----
def case_saturation(geo):
    fr = new_frame("saturation", geo)
    rng = np.random.default_rng(2)
    T = Tiles(fr)
    n = fr.notes
    n["prefix"], n["staggered"], n["half_dead"] = {}, [], {}  # (and "threshold", below)
    for k in PREFIXES:  # a transparent prefix (alpha 0 and alpha 1/255 in turn), then alpha 0.99: a break at k + 2
        t = T.take()
        n["prefix"][tile_id(fr, t)] = k
        for d in range(k):
            flat(fr, t, d % 2, colour(rng), depth_bits(d))
        for d in range(k, k + 6):
            flat(fr, t, 255, colour(rng), depth_bits(d))
    # groups of one unit break at different entries: the four pixel columns of group column lx twice each, lx by
    # lx from the left, then rows from the top over what is left, then a tail over the whole tile
    t = T.take(low=True)
    n["staggered"].append(tile_id(fr, t))
    d = 0
    for lx in (0, 1, 5):
        for x in range(4 * lx, 4 * lx + 4):
            for _ in range(2):
                column(fr, t, x, 255, colour(rng), depth_bits(d))
                d += 1
    for y in (0, 1, 6, 7):
        for _ in range(2):
            row(fr, t, y, 255, colour(rng), depth_bits(d))
            d += 1
    for _ in range(40):
        flat(fr, t, 2, colour(rng), depth_bits(d))
        d += 1
    # exactly 15, 16 and 17 of the left half's 32 groups dead from entry 64 on (rows kill 4 of its groups with 4
    # records, points one group with 16), alpha-0 entries up to entry 64, then a tail over the whole tile
    for dead in (15, 16, 17):
        t = T.take(low=True)
        n["half_dead"][tile_id(fr, t)] = dead
        d = 0
        rows_ = {15: 3, 16: 4, 17: 4}[dead]
        for ly in range(rows_):
            for y in (2 * ly, 2 * ly + 1):
                for _ in range(2):
                    row(fr, t, y, 255, colour(rng), depth_bits(d))
                    d += 1
        singles = {15: [(0, 5), (2, 6), (3, 7)], 16: [], 17: [(1, 6)]}[dead]  # (lx, ly) killed point by point
        for lx, ly in singles:
            for x in range(4 * lx, 4 * lx + 4):
                for y in (2 * ly, 2 * ly + 1):
                    for _ in range(2):
                        point(fr, t, x, y, 255, colour(rng), depth_bits(d))
                        d += 1
        assert d <= 64
        while d < 64:
            flat(fr, t, 0, colour(rng), depth_bits(d))
            d += 1
        for _ in range(40):
            flat(fr, t, 2, colour(rng), depth_bits(d))
            d += 1
    # T lands on the break threshold exactly: fp16(1 - 191/255) * fp16(1 - 251/255) = fp16(1 / 255), so the walk
    # goes on (the break is T < 1/255), blends one more entry and breaks before the next
    t = T.take()
    n["threshold"] = (tile_id(fr, t), 2)
    for d, op in enumerate((191, 251, 255, 1, 1, 1, 1, 1)):  # (the third one bright: it shows in the pixel)
        flat(fr, t, op, (255, 255, 255) if d == 2 else (10, 20, 30), depth_bits(d))
    return fr


# ---- non-finite and signed depths ----
def case_depths(geo):
    """A depth of +inf or NaN sorts after every finite one (key field bits ^ 0x8000), so what follows it in a
    list is non-finite too: position p of 70 = p finite entries, the record, then NaNs of larger bits.  The
    record is a column in the left half's first group column: nonzero alpha for 8 groups of that half, zero
    for its other 24, zero for the whole right half."""
    fr = new_frame("depths", geo)
    rng = np.random.default_rng(3)
    T = Tiles(fr)
    fr.notes["nonfinite"] = {}
    for bits in (0x7C00, 0x7E00):
        for pos in NONFINITE_POSITIONS:
            t = T.take(low=True)
            fr.notes["nonfinite"][tile_id(fr, t)] = (bits, pos)
            for d in range(pos):
                flat(fr, t, 3, colour(rng), depth_bits(d))
            column(fr, t, 2, 200, colour(rng), bits)
            for j in range(70 - pos - 1):
                b = 0x7E01 + j  # (what follows touches only the left half's first two group columns)
                if j % 2 == 0:
                    column(fr, t, (3 * j) % 8, 60, colour(rng), b)
                else:
                    flat(fr, t, 0, colour(rng), b)
    # the key order of signed depths (the key flips the sign bit and compares bits): -0 first, then the negative
    # ones by ascending magnitude, then +0, the positive subnormals and the positive normals
    t = T.take()
    order = [0x8000, 0x8001, 0x83FF, 0xBC00, 0xFBFF, 0x0000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF]
    fr.notes["signed"] = (tile_id(fr, t), order)
    for i in rng.permutation(len(order)):
        flat(fr, t, 40 + 10 * int(i), colour(rng), order[int(i)])
    return fr


# ---- the half-tile skip band ----
RHOS = ("0", "0.9", "below", "above")


def conic_for(ex, rho, cyy_ratio):
    """fp16 (cxx, cyy, cxy2) whose skip band is about ex pixels wide: ex^2 = L cyy / det"""
    L = R.BLEND_ZERO_P + 1e-3
    if rho in ("below", "above"):  # cxx = cyy = a power of two c: 1.875 c is an fp16, rho = 15/16 exactly there
        c0 = L / (ex * ex * (1.0 - (15.0 / 16.0) ** 2))
        c = 2.0 ** round(np.log2(c0))
        edge = np.float16(1.875 * c)
        assert float(edge) == 1.875 * c
        cxy2 = np.nextafter(edge, np.float16(0 if rho == "below" else np.inf))
        return c, c, float(cxy2)
    r = float(rho)
    cxx = L / (ex * ex * (1.0 - r * r))
    cyy = cxx * cyy_ratio
    return cxx, cyy, -2.0 * r * np.sqrt(float(np.float16(cxx)) * float(np.float16(cyy)))


def case_skip_band(geo):
    fr = new_frame("skip_band", geo)
    bases = [48, 112, 208] + ([2064, 3088, 4016] if fr.max_width > 2048 else [])
    idx = 0
    fr.notes["band"] = []
    for base in bases:
        for ex in (0.7, 3.0, 12.0, 50.0, 150.0, 200.0):
            for rho in RHOS:
                for ratio in (1.0 / 64.0, 64.0):
                    if rho in ("below", "above") and ratio != 64.0:
                        continue
                    for delta in (-1.0, -0.5, 0.0, 0.5, 1.0):
                        for side in (-1, 1):
                            cxx, cyy, cxy2 = conic_for(ex, rho, ratio)
                            ty = idx % fr.tiles_y
                            # the band's edge mx + side * ex lies delta pixels from the half-tile boundary `base`
                            mx = float(np.float16(base + delta - side * ex))
                            if mx < 0 or mx > fr.max_width - 1:
                                continue
                            lo = max(int(np.floor((mx - ex - 8) / 32)), 0)
                            hi = min(int(np.floor((mx + ex + 8) / 32)), fr.tiles_x - 1)
                            hi = min(hi, lo + 31)
                            i = fr.add(mx, ty * 16 + 8, cxx, cyy, cxy2, 255, (255, 255, 255),
                                       rect=(lo, hi, ty, ty), dep_bits=depth_bits(idx % 4000))
                            fr.notes["band"].append(i)
                            idx += 1
    return fr


# ---- scatter and sort ----
def case_scatter(geo):
    fr = new_frame("scatter", geo)
    rng = np.random.default_rng(5)
    n = fr.notes
    big = (1, 8, 2, 5)  # 8 x 4 tiles
    # block 0: 256 full 8 x 4 rects, 8192 slots, depths with ties
    for i in range(256):
        flat(fr, None, 1, colour(rng), depth_bits(int(rng.integers(0, 40))), rect=big)
    n["full_block"] = (0, 256)
    # block 1: 127 full rects (4064 slots), then 1-tile and 32-tile records in turn: slot 4096 falls inside a
    # 32-tile record that follows 1-tile ones
    for i in range(127):
        flat(fr, None, 1, colour(rng), depth_bits(int(rng.integers(0, 40))), rect=big)
    for i in range(129):
        if i % 9 == 8:
            flat(fr, None, 1, colour(rng), depth_bits(int(rng.integers(0, 40))), rect=big)
        else:
            flat(fr, (int(rng.integers(1, 9)), int(rng.integers(2, 6))), 1, colour(rng),
                 depth_bits(int(rng.integers(0, 40))))
    n["mixed_block"] = (256, 512)
    assert fr.count == 512
    # every rect shape w x h of at most 32 tiles that fits the grid, at the grid's far corner (the frame's last
    # column and row), with a full mask, one of alternating bits and a random one; every mask bit gets used
    n["shapes"] = fr.count
    for w in range(1, min(32, fr.tiles_x) + 1):
        for hh in range(1, min(32 // w, fr.tiles_y) + 1):
            rect = (fr.tiles_x - w, fr.tiles_x - 1, fr.tiles_y - hh, fr.tiles_y - 1)
            full = (1 << (w * hh)) - 1
            for m in (full, 0x55555555 & full, int(rng.integers(0, 1 << 32)) & full):
                flat(fr, None, 1, colour(rng), depth_bits(int(rng.integers(0, 40))), rect=rect, mask=m)
    # single-bit masks of an 8 x 4 rect: only bit 0, only bit 31; alternating bits both ways
    for m in (1, 1 << 31, 0x55555555, 0xAAAAAAAA):
        flat(fr, None, 2, colour(rng), depth_bits(50), rect=big, mask=m)
    n["shapes_end"] = fr.count
    # 600 records of equal depth bits in one tile, across the 256-record block edges that follow
    t = (0, 0)
    n["ties"] = (tile_id(fr, t), fr.count, 600)
    for i in range(600):
        flat(fr, t, 1 + i % 2, colour(rng), depth_bits(7))
    # one tile past 2048 entries (the per-tile LDS sort's limit): 2100, every fourth with some alpha
    t = (0, 1)
    n["crowded"] = (tile_id(fr, t), 2100)
    for i in range(2100):
        flat(fr, t, 1 if i % 4 == 0 else 0, colour(rng), depth_bits(int(rng.integers(0, 300))))
    return fr


def case_count(count):
    def make(geo):
        fr = new_frame("count%d" % count, geo)
        rng = np.random.default_rng(count)
        for i in range(count):
            t = (int(rng.integers(0, fr.tiles_x)), int(rng.integers(0, fr.tiles_y)))
            flat(fr, t, 100, colour(rng), depth_bits(int(rng.integers(0, 8))))
        return fr
    return make


def case_sprinkle(geo):
    """a few records in every tile of a small frame: the frame shapes and the stores"""
    fr = new_frame("sprinkle", geo)
    rng = np.random.default_rng(7)
    for ty in range(fr.tiles_y):
        for tx in range(fr.tiles_x):
            for d in range(3):
                fr.add(tx * 32 + int(rng.integers(0, 32)), ty * 16 + int(rng.integers(0, 16)), 0.02, 0.03, 0.01, 180,
                       colour(rng), rect=(tx, tx, ty, ty), dep_bits=depth_bits(d))
    return fr


CASES = {"lengths": case_lengths, "saturation": case_saturation, "depths": case_depths,
         "skip_band": case_skip_band, "scatter": case_scatter, "count1": case_count(1),
         "count255": case_count(255), "count256": case_count(256), "count257": case_count(257),
         "sprinkle": case_sprinkle}
MAX_GAUSSIANS = 16384  # of every renderer of these tests: 65536 assignments

_frames = {}


def frame(name, geo):
    """the case's frame for a geometry (a name of GEOMETRIES or a (w, h, max_w, max_h) tuple), built once"""
    key = (name, geo)
    if key not in _frames:
        _frames[key] = CASES[name](geo)
        assert _frames[key].count <= MAX_GAUSSIANS
    return _frames[key]
