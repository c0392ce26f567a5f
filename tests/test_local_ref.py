"""LocalRenderer frame, CPU side (include/gsm_local.h).

The restatement of LocalRenderer.render (tests/local/local_ref.c) checked for the properties the
reference's pipeline guarantees, tied to the committed Global oracle where the two projections compute
the same values, the reference's per-tile sort known-answer tests (LocalUnitTests.swift:122-235), the
overflow scene the GPU test relies on, and the ABI surface.  The GPU side is tests/test_local.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import local_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _h(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


@pytest.fixture(scope="module")
def small_frame(oracle):
    import local_ref
    n, w, h = 2000, 100, 70  # 7 x 5 tiles, the right and bottom ones partial
    world, harm = S.scene(n, w, h, 4, 1, 7)
    r = local_ref.render(world, harm, 4, S.cam(w, h), w, h)
    assert r["status"] == 0
    return r, world, harm, w, h


def test_ref_pipeline_invariants(small_frame, oracle):
    r, world, _, w, h = small_frame
    V = r["visible"]
    assert 0 < V <= len(world) and V == int(r["mask"].sum())
    # compaction preserves gaussian order
    np.testing.assert_array_equal(r["source"], np.nonzero(r["mask"])[0])
    P = r["projected"]
    assert np.all(P["maxTile"] > P["minTile"])
    assert np.all(P["maxTile"][:, 0] <= r["tiles_x"]) and np.all(P["maxTile"][:, 1] <= r["tiles_y"])
    depth16 = P["depth"] ^ 0x8000
    counts, lists = r["tile_counts"], r["tile_lists"]
    assert r["overflow"] == 0 and r["max_tile_count"] == counts.max() <= S.MAX_PER_TILE
    assert r["total_entries"] == int(counts.sum()) and r["active_tiles"] == int((counts > 0).sum())
    # every list is strictly ascending in (depth16, compacted index) and holds the tile's gaussians
    rect = np.zeros(r["tile_count"], np.int64)
    for g in range(V):
        for ty in range(P["minTile"][g, 1], P["maxTile"][g, 1]):
            rect[ty * r["tiles_x"] + P["minTile"][g, 0]:ty * r["tiles_x"] + P["maxTile"][g, 0]] += 1
    pruned = 0
    for t in range(r["tile_count"]):
        lst = lists[t, :counts[t]].astype(np.int64)
        key = (depth16[lst].astype(np.int64) << 32) | lst
        assert np.all(np.diff(key) > 0)
        tx, ty = t % r["tiles_x"], t // r["tiles_x"]
        inside = (P["minTile"][lst, 0] <= tx) & (tx < P["maxTile"][lst, 0]) & \
                 (P["minTile"][lst, 1] <= ty) & (ty < P["maxTile"][lst, 1])
        assert inside.all()
        assert counts[t] <= rect[t]  # the entries are the rect's tiles that pass intersectsTile
        pruned += int(rect[t] - counts[t])
        assert r["walked"][t] <= counts[t] and (counts[t] == 0) == (r["walked"][t] == 0)
    assert pruned > 0  # intersectsTile drops some tiles of some rects
    # tiles with count 0 hold the clear value: colour (0, 0, 0, 0), depth 0
    for t in np.nonzero(counts == 0)[0]:
        tx, ty = t % r["tiles_x"], t // r["tiles_x"]
        assert not r["color"][ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].any()
        assert not r["depth"][ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].any()


def test_ref_counts_equal_intersecting_rect_tiles(oracle):
    """The counts from a second, independent walk: per gaussian, the tiles of its rect that pass
    intersectsTile on the widened fp16 record (numpy restatement of GaussianShared.h:595-653 in fp32)."""
    import local_ref
    n, w, h = 300, 100, 70
    world, harm = S.scene(n, w, h, 1, 0, 3, scale_px=3.0)
    r = local_ref.render(world, harm, 1, S.cam(w, h), w, h)
    P = r["projected"]
    f = np.float32
    L = local_ref.lib()

    def seg(a, b, c, d, lo, hi):
        delta = f(f(b * b) - f(f(f(4.0) * a) * c))
        t1 = f(f(f(lo - d) * f(f(2.0) * a)) + b)
        t2 = f(f(f(hi - d) * f(f(2.0) * a)) + b)
        return delta >= 0 and (t1 <= 0 or f(t1 * t1) <= delta) and (t2 >= 0 or f(t2 * t2) <= delta)

    counts = np.zeros(r["tile_count"], np.uint32)
    for g in range(r["visible"]):
        cx, cy = _h(P["posX"][g]), _h(P["posY"][g])
        A, B, Cc = _h(P["conicA"][g]), _h(P["conicB"][g]), _h(P["conicC"][g])
        wv = f(f(2.0) * f(L.lr_compute_power(float(_h(P["opacity"][g])))))
        for ty in range(P["minTile"][g, 1], P["maxTile"][g, 1]):
            for tx in range(P["minTile"][g, 0], P["maxTile"][g, 0]):
                x0, y0, x1, y1 = f(tx * 16), f(ty * 16), f(tx * 16 + 15), f(ty * 16 + 15)
                hit = x0 <= cx <= x1 and y0 <= cy <= y1
                if not hit:
                    dx = f(cx - x0) if f(cx * f(2.0)) < f(x0 + x1) else f(cx - x1)
                    hit = seg(Cc, f(f(f(-2.0) * B) * dx), f(f(f(A * dx) * dx) - wv), cy, y0, y1)
                if not hit:
                    dy = f(cy - y0) if f(cy * f(2.0)) < f(y0 + y1) else f(cy - y1)
                    hit = seg(A, f(f(f(-2.0) * B) * dy), f(f(f(Cc * dy) * dy) - wv), cx, x0, x1)
                counts[ty * r["tiles_x"] + tx] += hit
    np.testing.assert_array_equal(counts, r["tile_counts"])


def test_ref_ties_to_global_oracle(oracle):
    """Well-separated gaussians inside the frustum: the visible set is the Global oracle's, the fp16
    position and depth are its bits (ndcToScreenCentered and clip w are shared), and the fp32 conic
    before packing is the inverse covariance the Global record quantises as (theta, sigma1, sigma2):
    equal up to that packing -- fp16 sigmas (2 * 2^-11 relative on 1 / sigma^2) and a 16-bit angle."""
    import local_ref
    n, w, h = 1500, 200, 150
    world, harm = S.scene(n, w, h, 4, 1, 13, scale_px=2.0, spread=0.4)
    r = local_ref.render(world, harm, 4, S.cam(w, h), w, h)
    g = oracle.render(world, harm, 4, S.cam(w, h), w, h)
    np.testing.assert_array_equal(r["mask"] > 0, g["mask"] > 0)
    vis = r["mask"] > 0
    assert vis.sum() > 1000
    rd = g["render_data"][vis]
    np.testing.assert_array_equal(r["projected"]["posX"], rd["meanX"])
    np.testing.assert_array_equal(r["projected"]["posY"], rd["meanY"])
    np.testing.assert_array_equal(r["projected"]["depth"], rd["depth"])
    # the packed record is the rounding of the fp32 values the checker reports
    pre = r["pre"][vis]
    np.testing.assert_array_equal(pre[:, 0].astype(np.float16).view(np.uint16), r["projected"]["posX"])
    np.testing.assert_array_equal(pre[:, 2].astype(np.float16).view(np.uint16), r["projected"]["conicA"])
    th = rd["theta"].astype(np.float64) * (np.pi / 65535.0)
    i1, i2 = 1.0 / _h(rd["sigma1"]).astype(np.float64) ** 2, 1.0 / _h(rd["sigma2"]).astype(np.float64) ** 2
    c, s = np.cos(th), np.sin(th)
    A, B, C = c * c * i1 + s * s * i2, c * s * (i1 - i2), s * s * i1 + c * c * i2
    tol = 2.5e-3 * np.maximum(i1, i2)
    assert np.all(np.abs(pre[:, 2] - A) <= tol) and np.all(np.abs(pre[:, 3] - B) <= tol)
    assert np.all(np.abs(pre[:, 4] - C) <= tol)


@pytest.mark.parametrize("which", ["full", "variable"])
def test_ref_sort_kats(oracle, which):
    """LocalUnitTests.testPerTileSortCorrectness / testPerTileSortVariableCounts, restated."""
    import local_ref
    keys, idx, counts, mpt = S.kat_inputs(which)
    got = local_ref.sort_tiles(keys, idx, counts, mpt)
    np.testing.assert_array_equal(got, S.kat_expected(keys, counts, mpt))
    for t, c in enumerate(counts.tolist()):  # the reference's own assertion: depths ascending
        d = keys[t * mpt + got[t * mpt:t * mpt + c].astype(np.int64)]
        assert np.all(np.diff(d.astype(np.int64)) >= 0)


def test_ref_overflow_scene(oracle):
    """2 500 identical gaussians in one tile and 300 others elsewhere: overflow is reported, the tile's
    unclamped count is 2 500 and its walk consumes exactly the 2 048 kept entries (the corner pixels
    never saturate), so whichever 2 048 a GPU keeps give these pixels."""
    import local_ref
    w = h = 64
    world, harm = S.stack(2500, w, h, others=300)
    r = local_ref.render(world, harm, 1, S.cam(w, h), w, h)
    assert r["status"] == 0 and r["overflow"] == 1 and r["max_tile_count"] == 2500
    over = np.nonzero(r["tile_counts"] > S.MAX_PER_TILE)[0]
    assert over.tolist() == [1 * r["tiles_x"] + 1]
    assert r["tile_counts"][over[0]] == 2500 and r["walked"][over[0]] == S.MAX_PER_TILE
    assert r["total_entries"] == int(np.minimum(r["tile_counts"], S.MAX_PER_TILE).sum())
    P = r["projected"]
    assert len(np.unique(P[:2500].view(np.uint8).reshape(2500, 32), axis=0)) == 1  # the copies are identical
    assert (r["tile_counts"] > 0).sum() > 4 and r["color"][16:32, 16:32, 3].min() < 0x3C00


def test_ref_stack_edges(oracle):
    """The scenes of the GPU's padding-edge test put exactly k entries into tile (1, 1)."""
    import local_ref
    for k in (1, 2, 2047, 2048):
        world, harm = S.stack(k)
        r = local_ref.render(world, harm, 1, S.cam(64, 64), 64, 64)
        assert r["tile_counts"][5] == k and r["tile_counts"].sum() == k and r["overflow"] == 0


def test_ref_plane_has_long_tie_runs(oracle):
    import local_ref
    w, h = 100, 70
    world, harm = S.plane(3000, w, h, 17)
    r = local_ref.render(world, harm, 1, S.cam(w, h), w, h)
    d16 = r["projected"]["depth"]
    assert len(np.unique(d16)) == 1 and r["tile_counts"].max() > 64 and r["overflow"] == 0


def test_ref_nonfinite_colour_scene(oracle):
    import local_ref
    world, harm = S.nonfinite_colour()
    r = local_ref.render(world, harm, 1, S.cam(64, 64), 64, 64)
    assert (r["projected"]["colorR"] == 0x7C00).sum() == 1  # half(colour) = +inf
    tile = _h(r["color"][16:32, 16:32, :3])
    assert np.isnan(tile).any() and np.isfinite(tile).any()


def test_header_declares_and_library_exports(gsm):
    hdr = open(os.path.join(ROOT, "include", "gsm_local.h")).read()
    names = ["gsm_local_create", "gsm_local_destroy", "gsm_local_render", "gsm_local_debug_counters",
             "gsm_local_debug_copy", "gsm_local_debug_sort_tiles", "gsm_local_set_profiling",
             "gsm_local_stage_times", "gsm_local_last_gpu_time"]
    declared = set(re.findall(r"\b(gsm_local_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(names) == set(gsm._LOCAL_SIGNATURES)
    lib = ctypes.CDLL(gsm.library_path())
    for n in names:
        assert hasattr(lib, n), n
    for f in ("gaussian_count", "visible", "tiles_x", "tiles_y", "tile_count", "active_tiles", "total_entries",
              "max_tile_count", "max_per_tile", "overflow"):
        assert re.search(r"uint32_t\s+[a-z_, ]*\b%s\b" % f, hdr), f
    assert all(hasattr(gsm.LocalRenderer, m) for m in ("render", "counters", "copy_buffer", "sort_tiles", "close"))
    assert [b.name for b in gsm.LocalBuffer] == ["PROJECTED", "TILE_COUNTS", "TILE_LISTS"]
    assert gsm.PROJECTED.itemsize == 32
    assert gsm.abi_version() == 1
