"""The reference of the crafted-records tests, checked without a device: the oracle's exported
record and blend steps against og_render, the numpy list builder and blend (tests/records_ref.py) against the
oracle, every adversarial property of every crafted case (tests/records_cases.py) asserted on the input from the
reference's alphas and group_iters, and every bent reference told from the true one by the case built for it."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import records_cases as K  # noqa: E402
import records_ref as R  # noqa: E402

GEOS = ("small", "wide")
IMAGE = ("color", "depth", "group_iters")


def first_diff(name, got, want):
    d = np.argwhere(np.asarray(got) != np.asarray(want))
    if not len(d):
        return name + ": equal"
    i = tuple(d[0])
    return "%s: %d differ, first at %s: got %s, want %s" % (name, len(d), i, got[i], want[i])


# ---- the oracle's exports and the list builder on a projected frame ----
@pytest.fixture(scope="module")
def projected(oracle):
    w, h, n = 640, 360, 6000
    world, harm = oracle.gen_visible_gaussians(n, 42)
    r = oracle.render(world, harm, 1, oracle.make_camera(w, h), w, h, max_gaussians=64 * n)
    assert r["overflow"] == 0 and r["total_assignments"] > 20000 and r["visible"] > n // 2
    return r


def test_exports_reproduce_og_render(oracle, projected):
    r = projected
    rec = oracle.blend_records(r["render_data"], r["mask"])
    b = oracle.blend_tiles(rec, r["headers"], r["sorted_values"], r["tiles_x"], r["tiles_y"], 640, 360)
    for k in IMAGE:
        assert np.array_equal(b[k], r[k]), first_diff(k, b[k], r[k])
    assert not rec[r["mask"] == 0].view(np.uint16).any()  # only the masked records are written


def test_list_builder_reproduces_the_frames_lists(projected):
    r = projected
    L = R.sort_lists(r["keys"], r["values"], r["tile_count"])
    for k in ("sorted_keys", "sorted_values", "headers"):
        assert np.array_equal(L[k], r[k]), first_diff(k, L[k], r[k])
    assert (np.diff(r["sorted_keys"].astype(np.int64)) == 0).sum() > 100  # ties: the order is the stable one
    bent = R.sort_lists(r["keys"], r["values"], r["tile_count"], "ties_reversed")
    assert not np.array_equal(bent["sorted_values"], r["sorted_values"])


def test_numpy_blend_equals_og_render_on_a_projected_frame(oracle):
    w, h, n = 320, 180, 2500
    world, harm = oracle.gen_visible_gaussians(n, 7)
    r = oracle.render(world, harm, 1, oracle.make_camera(w, h), w, h, max_gaussians=64 * n)
    assert r["overflow"] == 0
    rec = oracle.blend_records(r["render_data"], r["mask"])
    fr = R.Frame("projected", w, h)
    fr._done = {k: rec[k].copy() for k in R.FIELDS}
    b = R.blend(fr, {"headers": r["headers"], "sorted_values": r["sorted_values"]})
    for k in IMAGE:
        assert np.array_equal(b[k], r[k]), first_diff(k, b[k], r[k])
    assert (r["group_iters"] < r["headers"][:, 1][:, None, None]).any()  # some groups did break early


def test_fma16_is_the_oracles_hfma(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(11)
    a = rng.integers(0, 1 << 16, 60000).astype(np.uint16)
    b = rng.integers(0, 1 << 16, 60000).astype(np.uint16)
    c = rng.integers(0, 1 << 16, 60000).astype(np.uint16)
    # where a double rounding would show: a * b + c on or next to an fp16 midpoint (c = a midpoint's neighbour
    # minus the product), tiny products beside large c, and c of the product's own size with the other sign
    k = 20000
    with np.errstate(all="ignore"):
        prod = R.f(a[:k]).astype(np.float64) * R.f(b[:k]).astype(np.float64)
        target = R.f(c[:k]).astype(np.float64)
        mid = (target + np.nextafter(R.f(c[:k]), np.float16(np.inf)).astype(np.float64)) / 2
        c[:k] = (mid - prod).astype(np.float16).view(np.uint16)
        c[k:2 * k] = (-prod).astype(np.float16).view(np.uint16)
    a[2 * k:2 * k + 2000] &= 0x83FF  # subnormal factors
    got = R.fma16(R.f(a), R.f(b), R.f(c)).view(np.uint16)
    want = np.array([L.og_hfma(int(x), int(y), int(z)) for x, y, z in zip(a, b, c)], np.uint16)
    assert np.array_equal(got, want), first_diff("fma16", got, want)
    assert (np.isnan(R.f(want))).sum() > 100 and np.isinf(R.f(want)).sum() > 100


def test_unorm_and_record_layout():
    """the 256 colour values are the oracle's; SplatRecord is laid out as gsm_internal.h and gsm_types.h say"""
    import oracle as O
    L = O.lib()
    want = [L.og_f2h(L.og_h2f(L.og_f2h(float(k))) / np.float32(255.0)) for k in range(256)]
    assert R.unorm(np.arange(256)).tolist() == want
    src = open(os.path.join(ROOT, "gsm-renderer_amd", "csrc", "gsm_internal.h")).read()
    m = re.search(r"struct SplatRecord \{(.*?)\};", src, re.S)
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", m.group(1), re.M)
    assert fields == [("uint4", "rd"), ("BlendRecordA", "ra"), ("short4", "bounds"), ("uint32_t", "rb"),
                      ("uint32_t", "pad")], fields
    types = open(os.path.join(ROOT, "gsm-renderer_amd", "csrc", "gsm_types.h")).read()
    assert "a.x = meanX | meanY<<16, a.y = cxx | cyy<<16, a.z = cxy2 | opacity<<16" in types
    assert "a.w = colR | colG<<16, b = colB | depth<<16" in types
    assert [R.SPLAT_RECORD.fields[k][1] for k in ("rd", "ra", "bounds", "rb", "pad")] == [0, 16, 32, 40, 44]
    fr = R.Frame("one", 64, 32)
    fr.add(33.5, 7.25, 0.5, 0.25, -0.125, 200, (1, 2, 3), dep_bits=0x4123, rect=(0, 1, 0, 1), mask=0b1010)
    rec = R.pack(fr)[0]
    h = lambda v: int(R.h(v))  # noqa: E731
    u = lambda v: int(R.unorm(v))  # noqa: E731
    assert rec["ra"].tolist() == [h(33.5) | h(7.25) << 16, h(0.5) | h(0.25) << 16, h(-0.125) | u(200) << 16,
                                  u(1) | u(2) << 16]
    assert rec["rb"] == u(3) | 0x4123 << 16 and rec["pad"] == 0b1010 and rec["bounds"].tolist() == [0, 1, 0, 1]
    keys, vals = R.assignments(fr)  # bits 1 and 3 of a 2 x 2 rect: tiles (1, 0) and (1, 1) of a 2-wide grid
    assert (keys >> 16).tolist() == [1, 3] and vals.tolist() == [0, 0]
    assert (keys & 0xFFFF).tolist() == [0x4123 ^ 0x8000] * 2


# ---- every crafted case: the two derivations agree ----
def every_record_is_allowed(fr):
    a = fr.arrays()
    b = a["bounds"].astype(np.int64)
    area = (b[:, 1] - b[:, 0] + 1) * (b[:, 3] - b[:, 2] + 1)
    assert (b[:, 0] >= 0).all() and (b[:, 2] >= 0).all() and (b[:, 0] <= b[:, 1]).all() and (b[:, 2] <= b[:, 3]).all()
    assert (b[:, 1] < fr.tiles_x).all() and (b[:, 3] < fr.tiles_y).all() and (area <= 32).all()
    assert (a["mask"].astype(np.int64) < (1 << area)).all()
    allowed = set(R.unorm(np.arange(256)).tolist())
    for k in ("op", "cr", "cg", "cb"):
        assert set(a[k].tolist()) <= allowed, k
    assert 1 <= fr.count <= 8192 or fr.name.startswith("sprinkle")


@pytest.mark.parametrize("geo", GEOS)
@pytest.mark.parametrize("name", list(K.CASES))
def test_numpy_blend_equals_the_oracle(oracle, name, geo):
    fr = K.frame(name, geo)
    every_record_is_allowed(fr)
    ref = R.reference(fr, oracle)
    b = R.blend(fr, ref)
    for k in IMAGE:
        assert np.array_equal(b[k], ref[k]), first_diff(fr.name + " " + k, b[k], ref[k])


@pytest.mark.parametrize("shape", K.TINY_SHAPES)
def test_numpy_blend_equals_the_oracle_on_small_frames(oracle, shape):
    fr = K.frame("sprinkle", shape + shape)
    ref = R.reference(fr, oracle)
    b = R.blend(fr, ref)
    for k in IMAGE:
        assert np.array_equal(b[k], ref[k]), first_diff(fr.name + " " + k, b[k], ref[k])
    assert ref["color"][..., :3].any()


# ---- the properties each case is there for, from the reference ----
def tile_list(ref, tile):
    s, c = (int(v) for v in ref["headers"][tile])
    return ref["sorted_values"][s:s + c]


@pytest.mark.parametrize("geo", GEOS)
def test_lengths_every_group_walks_its_whole_list(oracle, geo):
    fr = K.frame("lengths", geo)
    ref = R.reference(fr, oracle)
    assert sorted(fr.notes["length"].values()) == sorted(K.LENGTHS)
    for tile, n in fr.notes["length"].items():
        assert ref["headers"][tile, 1] == n
        assert (ref["group_iters"][tile] == n).all(), (tile, n)  # low alpha: no group ever saturates
    assert int((ref["headers"][:, 1] > 0).sum()) == len(K.LENGTHS) - 1
    tiles = np.array(list(fr.notes["length"]))
    assert (tiles % fr.tiles_x == fr.tiles_x - 1).any() and (tiles // fr.tiles_x == fr.tiles_y - 1).any()


@pytest.mark.parametrize("geo", GEOS)
def test_saturation_break_patterns(oracle, geo):
    fr = K.frame("saturation", geo)
    ref = R.reference(fr, oracle)
    it = ref["group_iters"]
    for tile, k in fr.notes["prefix"].items():
        assert ref["headers"][tile, 1] == k + 6 and (it[tile] == k + 2).all(), (tile, k, np.unique(it[tile]))
    for tile in fr.notes["staggered"]:
        count = ref["headers"][tile, 1]
        for unit in (it[tile][:, :4], it[tile][:, 4:], it[tile][:4, :4], it[tile][4:, :4], it[tile][:4, 4:]):
            assert np.unique(unit).size >= 3, np.unique(unit)  # half-tile and quadrant units alike
        assert (it[tile] == count).any() and (it[tile] < 16).any() and ((it[tile] > 16) & (it[tile] < 32)).any()
    for tile, dead in fr.notes["half_dead"].items():
        count = ref["headers"][tile, 1]
        left = it[tile][:, :4]
        assert count == 104 and int((left <= 64).sum()) == dead, (dead, np.unique(left))
        assert (left[left > 64] == count).all()  # the others walk the tail to its end
        for checkpoint in (64, 80, 96):
            assert int((left <= checkpoint).sum()) == dead
    tile, n = fr.notes["threshold"]
    a = np.fmin(R.f(R.unorm(np.array([191, 251]))), np.float16(0.99))
    T = (np.float16(1) - a[0]) * (np.float16(1) - a[1])
    assert T == np.float16(np.float32(1) / np.float32(255))  # exactly the threshold after two entries
    assert (it[tile] == n + 1).all(), np.unique(it[tile])


@pytest.mark.parametrize("geo", GEOS)
def test_depths_positions_and_alphas(oracle, geo):
    fr = K.frame("depths", geo)
    ref = R.reference(fr, oracle)
    dep = fr.arrays()["dep"]
    seen = set()
    for tile, (bits, pos) in fr.notes["nonfinite"].items():
        ids = tile_list(ref, tile)
        d = dep[ids]
        assert ids.size == 70 and d[pos] == bits, (tile, hex(bits), pos)
        nonfinite = (d & 0x7C00) == 0x7C00
        assert not nonfinite[:pos].any() and nonfinite[pos:].all()
        al = R.tile_alphas(fr, tile, ids[pos:pos + 1])[0].reshape(8, 2, 8, 4) != 0
        per_group = al.sum(axis=(1, 3))
        assert (per_group[:, 0] == 2).all()  # the half's first group column: 2 of 8 alphas nonzero
        assert not per_group[:, 1:].any()    # its other 24 groups and the right half: all zero
        assert (ref["group_iters"][tile] == 70).all()  # every group is still walking when it comes
        x0, y0 = (tile % fr.tiles_x) * 32, (tile // fr.tiles_x) * 16
        got = R.f(ref["depth"][y0:y0 + 16, x0:x0 + 32])
        assert not np.isfinite(got[:, 2]).any()       # the record's own column
        assert np.isnan(got[:, 0]).all()              # alpha 0 in a group that blends it: inf * 0
        assert np.isfinite(got[:, 16:]).all()         # the right half skipped it
        if pos:
            assert (got[:, 16:] > 0).all()
        seen.add((bits, pos))
    assert seen == {(b, p) for b in (0x7C00, 0x7E00) for p in K.NONFINITE_POSITIONS}
    tile, order = fr.notes["signed"]
    assert dep[tile_list(ref, tile)].tolist() == order
    assert {0x8000, 0x0000, 0x0001, 0x03FF, 0x8001} <= set(order)


def band_halves(fr, ref):
    """per (band record, tile of its rect, half): all-zero alpha?, only the boundary column nonzero?, flagged by
    the skip-band model?"""
    a = fr.arrays()
    rows = []
    for i in fr.notes["band"]:
        x0, x1, ty, _ = (int(v) for v in a["bounds"][i])
        band = R.skip_band(fr, i)
        for tx in range(x0, x1 + 1):
            al = R.tile_alphas(fr, ty * fr.tiles_x + tx, [i])[0] != 0
            flags = R.half_skip_flags(band, tx)
            for hh in (0, 1):
                cols = al[:, 16 * hh:16 * hh + 16].any(axis=0)
                edge_only = cols.sum() == 1 and (cols[0] or cols[15])
                rows.append((i, tx, hh, not cols.any(), bool(edge_only), flags[hh], band is not None))
    return np.array(rows, np.int64)


@pytest.mark.parametrize("geo", GEOS)
def test_skip_band_halves(oracle, geo, capsys):
    fr = K.frame("skip_band", geo)
    ref = R.reference(fr, oracle)
    t = band_halves(fr, ref)
    zero, edge, flagged, banded = (t[:, k].astype(bool) for k in (3, 4, 5, 6))
    assert zero.sum() > 200 and edge.sum() > 20, (zero.sum(), edge.sum())
    assert (flagged <= zero).all(), t[flagged & ~zero][:5]  # the model never flags a half with a nonzero alpha
    assert flagged.sum() > 100 and (zero & ~flagged & banded).sum() > 0 and (~banded).sum() > 0
    a = fr.arrays()
    mx = R.f(a["mx"][fr.notes["band"]]).astype(np.float32)
    if fr.max_width > 2048:  # fp16 pixel coordinates 2 apart
        assert (mx >= 2048).sum() > 100 and (t[:, 1] >= 64).sum() > 100
        assert (zero & flagged & (t[:, 1] >= 64)).any() and (edge & (t[:, 1] >= 64)).any()
    with capsys.disabled():
        print("\n[skip band, %s] halves %d, all-zero %d, boundary column only %d, flagged by the model %d "
              "(%.1f %% of the all-zero ones), records without a band %d" %
              (geo, len(t), zero.sum(), edge.sum(), flagged.sum(), 100.0 * flagged.sum() / zero.sum(),
               len({int(r[0]) for r in t[~banded]})))
    # the group's walk reaches these entries: unsaturated pixels remain in the tiles' edge columns
    assert (ref["group_iters"][ref["headers"][:, 1] > 0] > 1).any()


@pytest.mark.parametrize("geo", GEOS)
def test_scatter_block_shapes(oracle, geo):
    fr = K.frame("scatter", geo)
    ref = R.reference(fr, oracle)
    a = fr.arrays()
    slots = np.array([bin(int(m)).count("1") for m in a["mask"]])
    b = a["bounds"].astype(np.int64)
    lo, hi = fr.notes["full_block"]
    assert (lo, hi) == (0, 256) and slots[lo:hi].sum() == 8192 and (slots[lo:hi] == 32).all()
    lo, hi = fr.notes["mixed_block"]
    assert lo % 256 == 0 and hi - lo == 256
    cum = np.cumsum(slots[lo:hi])
    at = int(np.searchsorted(cum, 4096, "right"))  # the record that holds the block's slot 4096
    assert slots[lo + at] == 32 and cum[at - 1] < 4096 < cum[at] and (slots[lo + at - 3:lo + at] == 1).all()
    assert cum[-1] > 4096
    s0, s1 = fr.notes["shapes"], fr.notes["shapes_end"]
    rw = (b[s0:s1, 1] - b[s0:s1, 0] + 1)
    wmax = min(32, fr.tiles_x)
    assert set(rw.tolist()) == set(range(1, wmax + 1))
    for w in range(1, wmax + 1):  # every mask bit a rect of this width can have is set in some record
        rows = np.flatnonzero(rw == w) + s0
        area = int(((b[rows, 1] - b[rows, 0] + 1) * (b[rows, 3] - b[rows, 2] + 1)).max())
        used = np.bitwise_or.reduce(a["mask"][rows])
        assert used == (1 << area) - 1, (w, hex(used))
    assert (b[s0:s1, 1] == fr.tiles_x - 1).any() and (b[s0:s1, 3] == fr.tiles_y - 1).any()
    assert {1, 1 << 31, 0x55555555, 0xAAAAAAAA} <= set(a["mask"][s0:s1].tolist())
    tile, first, n = fr.notes["ties"]
    ks = ref["sorted_keys"][ref["headers"][tile, 0]:][:ref["headers"][tile, 1]]
    vals, counts = np.unique(ks, return_counts=True)
    assert counts.max() >= n
    ids = tile_list(ref, tile)[ks == vals[counts.argmax()]]
    assert np.unique(ids // 256).size >= 3 and (np.diff(ids) > 0).all()  # across block edges, in record order
    tile, n = fr.notes["crowded"]
    assert ref["headers"][tile, 1] == n > 2048
    assert ref["keys"].size <= 4 * K.MAX_GAUSSIANS and fr.count <= K.MAX_GAUSSIANS


def test_record_counts():
    for n in (1, 255, 256, 257):
        assert K.frame("count%d" % n, "small").count == n == K.frame("count%d" % n, "wide").count


# ---- bent references: each is told from the true one by the case built for it ----
BENT_CASE = {"ties_reversed": "scatter", "break_le": "saturation", "no_zero_skip": "depths", "unfused": "lengths",
             "key_no_xor": "depths"}


@pytest.mark.parametrize("bend", R.BENDS)
def test_bent_reference_changes_its_case(oracle, bend):
    assert set(BENT_CASE) == set(R.BENDS)
    fr = K.frame(BENT_CASE[bend], "small")
    ref = R.reference(fr, oracle)
    L = R.lists(fr, bend) if bend in ("ties_reversed", "key_no_xor") else ref
    if bend == "ties_reversed":  # only the tile of the equal keys has to be walked again
        tile = fr.notes["ties"][0]
        hdr = np.zeros_like(ref["headers"])
        hdr[tile] = ref["headers"][tile]
        L = dict(L, headers=hdr)
        true = R.blend(fr, dict(ref, headers=hdr))
    else:
        true = ref
    bent = R.blend(fr, L, bend)
    x0, y0 = 0, 0
    differs = {k: not np.array_equal(bent[k], true[k]) for k in IMAGE}
    if bend == "ties_reversed":
        assert not np.array_equal(L["sorted_values"], ref["sorted_values"]) and differs["color"], differs
    elif bend == "break_le":
        tile, n = fr.notes["threshold"]
        assert (bent["group_iters"][tile] == n).all() and differs["color"] and differs["group_iters"], differs
    elif bend == "no_zero_skip":
        tile = next(iter(fr.notes["nonfinite"]))
        x0, y0 = (tile % fr.tiles_x) * 32, (tile // fr.tiles_x) * 16
        assert np.isnan(R.f(bent["depth"][y0:y0 + 16, x0 + 16:x0 + 32])).all() and differs["depth"], differs
        assert not differs["color"] and not differs["group_iters"]  # alpha 0 changes nothing else
    elif bend == "unfused":
        assert differs["color"] and differs["depth"] and not differs["group_iters"], differs
    else:
        assert not np.array_equal(L["sorted_values"], ref["sorted_values"]) and differs["color"], differs


def test_explain_pixel_finds_a_dropped_entry(oracle):
    """the GPU comparison's message: a walk that stopped one entry short is reported at that entry"""
    fr = K.frame("lengths", "small")
    ref = R.reference(fr, oracle)
    tile = next(t for t, n in fr.notes["length"].items() if n == 17)
    hdr = ref["headers"].copy()
    hdr[tile, 1] = 16
    short = R.blend(fr, dict(ref, headers=hdr))
    x, y = (tile % fr.tiles_x) * 32 + 5, (tile // fr.tiles_x) * 16 + 3
    if x >= fr.width or y >= fr.height:
        x, y = (tile % fr.tiles_x) * 32, (tile // fr.tiles_x) * 16
    got = list(short["color"][y, x]) + [short["depth"][y, x]]
    assert got != list(ref["color"][y, x]) + [ref["depth"][y, x]]
    text = R.explain_pixel(fr, ref, y, x, got)
    assert "list 17 entries" in text and "after [16] entries" in text, text
