"""The frame sort restated in numpy (integers only): the order, the tile starts and the half-tile lists that
gsm_debug_frame_sort_run (include/gsm_debug.h) must produce, bit for bit.

  order       a stable argsort -- on the whole tile << 16 | depth word with the depth sort, on keys >> shift alone
              without it (the depth field then rides along in input order);
  tile starts tileStart[t] = the number of keys whose tile is below t, for t = 0 .. all_tiles (the lower bound the
              kernel's comment promises for an empty tile as well), so tileStart[all_tiles] = n;
  half lists  per tile, in sorted order, half h keeps the values & GID_MASK whose bit 30 + h is clear, written from the
              tile's start; half_count[h * all_tiles + t] = how many.

`perturb` bends the reference on purpose (tests only: the comparisons must then fail)."""
import numpy as np

HALF_SKIP_SHIFT = 30                     # kHalfSkipShift (gsm_internal.h)
GID_MASK = (1 << HALF_SKIP_SHIFT) - 1    # kGidMask
CHUNK = 4096                             # kRadixChunk: keys per block and round of the narrow passes
WIDE_CHUNK = 4096                        # kWideChunk
SUPER_GROUP = 32                         # kSuperGroup: blocks sharing one scanless row
TILE_SORT_CAP = 2048                     # kTsCap: the longest run k_tile_sort holds in LDS


def bits_for(tiles):
    """radix_sort_tiles' bitsFor: the bits of the largest tile id, at least 1, at most 16"""
    b = 1
    while b < 16 and ((tiles - 1) >> b):
        b += 1
    return b


def narrow_widths(all_tiles):
    """(low, high) digit widths of the two narrow passes (radix_sort_tiles); (bits, 0) for one pass"""
    bits = bits_for(all_tiles)
    if bits <= 8:
        return max(bits, 4), 0
    lo = (bits + 1) // 2
    return lo, max(bits - lo, 4)


def wide_low_bits(all_tiles):
    """the wide first pass of radix_sort_tiles_wide: tile bits (17..19) - 8"""
    b = 17
    while b < 32 and ((all_tiles - 1) >> b):
        b += 1
    return b - 8


def grid_for(capacity):
    return max(1, min(1024, -(-capacity // CHUNK)))


def block_ranges(n, capacity):
    """[begin, end) of every block of a pass over n keys on a grid sized for `capacity` (block_range)"""
    grid = grid_for(capacity)
    per = -(-n // grid)
    per = -(-per // CHUNK) * CHUNK
    b = np.minimum(np.arange(grid, dtype=np.int64) * per, n)
    return b, np.minimum(b + per, n)


def reference(keys, values, shift, all_tiles, depth_sort, perturb=None):
    """-> dict(order, sorted_keys, sorted_values, tile_start[all_tiles + 1], and with depth_sort: half[2] (lists of
    per-tile arrays are flattened: half[h][tile_start[t] : tile_start[t] + half_count[h, t]]), half_count[2, tiles])"""
    keys = np.asarray(keys, np.uint32)
    values = np.asarray(values, np.uint32)
    n = keys.size
    sort_word = keys if depth_sort else keys >> np.uint32(shift)
    order = np.argsort(sort_word, kind="stable")
    if perturb == "ties_reversed":  # equal words in reverse input order
        order = (n - 1 - np.argsort(sort_word[::-1], kind="stable"))
    sk, sv = keys[order], values[order]
    tile = (sk >> np.uint32(shift)).astype(np.int64)
    side = "right" if perturb == "starts_right" else "left"
    tile_start = np.searchsorted(tile, np.arange(all_tiles + 1), side).astype(np.uint32)
    if perturb != "starts_right":
        tile_start[all_tiles] = n
    out = dict(order=order, sorted_keys=sk, sorted_values=sv, tile_start=tile_start)
    if depth_sort:
        ts = np.searchsorted(tile, np.arange(all_tiles + 1), "left")
        half = [np.zeros(n, np.uint32), np.zeros(n, np.uint32)]
        kept = [np.zeros(n, bool), np.zeros(n, bool)]  # which words of half[h] the sort writes
        count = np.zeros((2, all_tiles), np.uint32)
        for h in range(2):
            bit = HALF_SKIP_SHIFT + (h ^ 1 if perturb == "flags_swapped" else h)
            keep = ((sv >> np.uint32(bit)) & 1) == 0
            # rank among the kept entries of the same tile, in sorted order
            c = np.cumsum(keep)
            before_tile = np.concatenate(([0], c))[ts[tile]] if n else np.zeros(0, np.int64)
            rank = c - keep - before_tile
            dst = (ts[tile] + rank)[keep]
            half[h][dst] = sv[keep] & np.uint32(GID_MASK)
            kept[h][dst] = True
            count[h] = np.bincount(tile[keep], minlength=all_tiles)[:all_tiles]
        out.update(half=half, half_written=kept, half_count=count)
    return out
