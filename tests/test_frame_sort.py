"""The production frame sort on crafted key distributions (gsm_debug_frame_sort, include/gsm_debug.h)
against its restatement in numpy (tests/frame_sort_ref.py): a stable argsort, searchsorted tile starts and the
half-tile lists.  Every comparison is exact.  Every adversarial property of an input is asserted on the input, in
numpy, before the GPU is consulted, and every case asserts the plan (the passes) it means to hit."""
import os
import re
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import frame_sort_ref as R  # noqa: E402

CSRC = os.path.join(ROOT, "gsm-renderer_amd", "csrc")
CHECK_SRC = os.path.join(HERE, "host", "frame_sort_check_test.cpp")
ERR_TILES, ERR_CAPACITY, ERR_RENDER, ERR_MISSING, ERR_ARG = 9, 10, 11, 13, 14
ONE_NARROW, TWO_NARROW, ONE_WIDE, WIDE_THEN_NARROW = 1, 2, 3, 4
SORT_ENV = ("GSM_SORT_RANK", "GSM_SORT_WIDE", "GSM_SORT_SCAN")
CHUNK = R.CHUNK

# ---- the plans: (id, all_tiles, num_tiles, shift, environment at create, the plan the run must report) ----
Plan = namedtuple("Plan", "name all_tiles num_tiles shift env plan")


def _plan(all_tiles, plan, num_tiles=None, shift=16, env=None, tag=""):
    num_tiles = all_tiles if num_tiles is None else num_tiles
    name = "%s-%d%s-s%d%s" % ({1: "narrow", 2: "narrow2", 3: "wide", 4: "wide+8"}[plan], all_tiles,
                              "" if num_tiles == all_tiles else "of%d" % num_tiles, shift, tag)
    return Plan(name, all_tiles, num_tiles, shift, env or {}, plan)


NO_WIDE = {"GSM_SORT_WIDE": "0"}
PLANS = (
    # one narrow pass: digits of 4 (1, 2, 16 tiles), 5, 6, 7 and 8 bits
    [_plan(t, ONE_NARROW) for t in (1, 2, 16, 17, 33, 65, 129, 256)] + [_plan(129, ONE_NARROW, shift=0)] +
    # two narrow passes: more than 2048 tiles in the frame, or wide digits off
    [_plan(t, TWO_NARROW) for t in (2049, 4080, 16200, 65536)] + [_plan(4080, TWO_NARROW, shift=0)] +
    [_plan(t, TWO_NARROW, env=NO_WIDE, tag="-nowide") for t in (257, 300, 1800)] +
    # one wide pass: 9, 10 and 11 bits; a frame smaller than its configuration
    [_plan(t, ONE_WIDE) for t in (257, 1000, 2048)] + [_plan(16200, ONE_WIDE, num_tiles=1800)] +
    [_plan(1000, ONE_WIDE, shift=0)] +
    # one wide pass, then 8 bits over up to 2048 buckets (BIGL): 17, 18 and 19 bit tile fields
    [_plan(t, WIDE_THEN_NARROW, shift=0) for t in (65537, 65792, 131072, 262144, 524288)])
PLAN_BY_NAME = {p.name: p for p in PLANS}
REPRESENTATIVES = ["narrow-129-s16", "narrow2-4080-s16", "wide-1000-s16", "wide+8-65792-s0"]


def low_bits(p):
    """bits of the first of two passes: its digits are the buckets the last pass derives the tile starts from"""
    if p.plan == TWO_NARROW:
        return R.narrow_widths(p.all_tiles)[0]
    if p.plan == WIDE_THEN_NARROW:
        return R.wide_low_bits(p.all_tiles)
    return 0


def test_plan_table_covers_every_digit_width():
    one = sorted({R.narrow_widths(p.all_tiles)[0] for p in PLANS if p.plan == ONE_NARROW})
    assert one == [4, 5, 6, 7, 8]
    two = {R.narrow_widths(p.all_tiles) for p in PLANS if p.plan == TWO_NARROW}
    assert {(5, 4), (6, 5), (7, 7), (8, 8)} <= two, two
    assert sorted({max(9, R.bits_for(p.num_tiles)) for p in PLANS if p.plan == ONE_WIDE}) == [9, 10, 11]
    assert sorted({R.wide_low_bits(p.all_tiles) for p in PLANS if p.plan == WIDE_THEN_NARROW}) == [9, 10, 11]
    assert any(p.all_tiles & (p.all_tiles - 1) for p in PLANS if p.plan == TWO_NARROW)  # the tt <= numTiles guard
    assert set(REPRESENTATIVES) <= set(PLAN_BY_NAME)


# ---- the distributions: f(rng, plan) -> (tile ids int64, capacity); each asserts what it is there for ----
def bucket_starts(tiles, lo):
    """where the first pass leaves the low-digit buckets (their starts, per digit)"""
    return np.searchsorted(np.sort(tiles & ((1 << lo) - 1)), np.arange(1 << lo), "left")


def starts_per_chunk(tiles, lo):
    """how many distinct bucket starts fall into each 4096-key chunk (starts at n belong to no chunk)"""
    s = np.unique(bucket_starts(tiles, lo))
    s = s[s < tiles.size]
    return np.bincount(s // CHUNK, minlength=-(-tiles.size // CHUNK))


def mixed(rng, T, n):
    """half of the keys anywhere, half in a few tiles (heavy duplicates: stability shows)"""
    hot = rng.integers(0, T, 8)
    t = np.where(rng.random(n) < 0.5, rng.integers(0, T, n), hot[rng.integers(0, 8, n)])
    return t.astype(np.int64)


def with_low_digits(rng, p, allowed, n):
    """n tiles below num_tiles whose low digit is one of `allowed` (each at least once), the high digit anywhere"""
    lo = low_bits(p)
    allowed = np.asarray(allowed, np.int64)
    highs = -(-p.num_tiles // (1 << lo))
    t = (rng.integers(0, highs, 4 * n + 64) << lo) | allowed[rng.integers(0, allowed.size, 4 * n + 64)]
    t = np.concatenate([allowed, t[t < p.num_tiles]])[:n]  # (high digit 0: the low digit is the tile)
    assert t.size == n and allowed.size <= n and allowed.max() < p.num_tiles
    return rng.permutation(t).astype(np.int64)


def d_count(n):
    def f(rng, p):
        cap = 3 * CHUNK
        assert n <= cap
        return mixed(rng, p.num_tiles, n), cap
    return f


def d_mostly_idle(rng, p):
    cap, n = 64 * CHUNK, 5000
    b, e = R.block_ranges(n, cap)
    assert b.size == 64 and int((b < e).sum()) == 2  # two blocks hold keys, 62 do not
    return mixed(rng, p.num_tiles, n), cap


def d_two_rows(rng, p):
    cap = 40 * CHUNK
    assert R.grid_for(cap) == 40 > R.SUPER_GROUP  # two super-group rows
    return mixed(rng, p.num_tiles, cap), cap


def d_all_in(which):
    def f(rng, p):
        t = {"first": 0, "last": p.num_tiles - 1, "middle": p.num_tiles // 2}[which]
        return np.full(9000, t, np.int64), 3 * CHUNK
    return f


def d_low_digit_only(rng, p):
    lo = low_bits(p)
    t = with_low_digits(rng, p, [5], 9000)
    s = bucket_starts(t, lo)
    assert (s[:6] == 0).all() and (s[6:] == t.size).all()  # every other bucket is empty and shares a start
    assert np.unique(t >> lo).size > 1
    return t, 3 * CHUNK


def d_high_digit_only(rng, p):
    lo = low_bits(p)
    h = (p.num_tiles >> lo) // 2
    t = ((h << lo) | rng.integers(0, 1 << lo, 9000)).astype(np.int64)
    assert (t < p.num_tiles).all() and np.unique(t >> lo).size == 1 and np.unique(t).size > 8
    return t, 3 * CHUNK


def d_one_per_tile(rng, p):
    T = p.num_tiles
    t = np.arange(T, dtype=np.int64) if T <= 300_000 else np.arange(0, T, 2, dtype=np.int64)
    t = rng.permutation(t)
    assert t.size <= 300_000 and np.bincount(t).max() == 1
    lo = low_bits(p)
    if lo:  # several bucket starts in one chunk: the recount loop
        per = starts_per_chunk(t, lo)
        assert per.max() >= 2, per
        if p.all_tiles == 65536:
            assert (per == 16).all()
    return t, max(t.size, 1)


def d_chunk_edges(rng, p):
    """bucket 1 starts on a multiple of 4096 (a block's and a chunk's first key), bucket 2 on a chunk's last key"""
    lo = low_bits(p)
    t = np.concatenate([with_low_digits(rng, p, [0], CHUNK), with_low_digits(rng, p, [1], CHUNK - 1),
                        with_low_digits(rng, p, [2], 1500)])
    t = rng.permutation(t)
    s = bucket_starts(t, lo)
    assert s[1] == CHUNK and s[2] == 2 * CHUNK - 1 and (s[3:] == t.size).all()
    b, _ = R.block_ranges(t.size, 3 * CHUNK)
    assert CHUNK in b  # the start is also a block's first key
    return t, 3 * CHUNK


def d_empty_buckets(which):
    def f(rng, p):
        lo = low_bits(p)
        L = 1 << lo
        allowed = {"leading": np.arange(L // 2, L), "trailing": np.arange(0, L // 4 + 1),
                   "alternating": np.arange(1, L, 2)}[which]
        t = with_low_digits(rng, p, allowed, 9000)
        cnt = np.bincount(t & (L - 1), minlength=L)
        s = bucket_starts(t, lo)
        if which == "leading":
            assert (cnt[:L // 2] == 0).all() and (s[:L // 2 + 1] == 0).all() and cnt[L // 2] > 0
        elif which == "trailing":  # the last block writes these
            assert (cnt[L // 4 + 1:] == 0).all() and (s[L // 4 + 1:] == t.size).all() and cnt[L // 4] > 0
        else:
            assert (cnt[0::2] == 0).all() and (cnt[1::2] > 0).all() and (s[0::2] == s[1::2]).all()
        return t, 3 * CHUNK
    return f


def d_order(which):
    def f(rng, p):
        few = np.unique(np.concatenate([rng.integers(0, p.num_tiles, 38), [0, p.num_tiles - 1]]))
        t = few[rng.integers(0, few.size, 9000)].astype(np.int64)
        t = {"sorted": np.sort(t), "reversed": np.sort(t)[::-1].copy(), "random": t}[which]
        assert np.bincount(t).max() >= 9000 // 40  # heavy duplicates
        return t, 3 * CHUNK
    return f


EVERY_PLAN = {"n0": d_count(0), "n1": d_count(1), "n4095": d_count(4095), "n4096": d_count(4096),
              "n4097": d_count(4097), "n8192": d_count(8192), "n_capacity": d_count(3 * CHUNK),
              "mostly_idle": d_mostly_idle, "all_first": d_all_in("first"), "all_last": d_all_in("last"),
              "all_middle": d_all_in("middle"), "one_per_tile": d_one_per_tile, "sorted": d_order("sorted"),
              "reversed": d_order("reversed"), "random": d_order("random")}
TWO_PASS_ONLY = {"low_digit_only": d_low_digit_only, "high_digit_only": d_high_digit_only,
                 "chunk_edges": d_chunk_edges, "leading_empty": d_empty_buckets("leading"),
                 "trailing_empty": d_empty_buckets("trailing"), "alternating_empty": d_empty_buckets("alternating")}
DISTRIBUTIONS = dict(EVERY_PLAN, **TWO_PASS_ONLY, two_rows=d_two_rows)
CASES = [(p.name, d) for p in PLANS for d in list(EVERY_PLAN) + (list(TWO_PASS_ONLY) if low_bits(p) else [])]


def make_case(plan_name, dist):
    """(plan, keys, values, capacity): the same bits every time (the seed is the case's name)"""
    p = PLAN_BY_NAME[plan_name]
    rng = np.random.default_rng(list((plan_name + "/" + dist).encode()))
    tiles, cap = DISTRIBUTIONS[dist](rng, p)
    n = tiles.size
    assert n <= cap and n <= 300_000 and (n == 0 or (tiles.min() >= 0 and tiles.max() < p.num_tiles))
    keys = tiles.astype(np.uint32)
    if p.shift == 16:  # a depth field that must ride along in input order
        keys = (keys << np.uint32(16)) | rng.integers(0, 1 << 16, n).astype(np.uint32)
    return p, keys, np.arange(n, dtype=np.uint32), cap


def test_every_case_precondition_holds_on_the_cpu():
    """every generator's own assertions (the adversarial property each case is there for), without a device"""
    for name, dist in CASES:
        make_case(name, dist)
    for name in REPRESENTATIVES:
        make_case(name, "two_rows")


# ---- comparison ----
def first_diff(a, b):
    i = np.flatnonzero(a != b)
    return "%d differ, first at %d: got %s, want %s" % (i.size, i[0], a[i[0]], b[i[0]]) if i.size else "equal"


FakeResult = namedtuple("FakeResult", "sorted_keys sorted_values tile_start half0 half1 half_count")


def assert_matches(res, ref, p, depth_sort=False, full=True):
    ts = ref["tile_start"]
    assert res.tile_start.shape == ts.shape
    assert np.array_equal(res.tile_start, ts), "tile starts: " + first_diff(res.tile_start, ts)
    if not depth_sort or full:
        assert np.array_equal(res.sorted_keys, ref["sorted_keys"]), \
            "sorted keys: " + first_diff(res.sorted_keys, ref["sorted_keys"])
        assert np.array_equal(res.sorted_values, ref["sorted_values"]), \
            "sorted values: " + first_diff(res.sorted_values, ref["sorted_values"])
    if depth_sort:
        got = res.half_count.reshape(2, p.all_tiles)[:, :p.num_tiles]
        want = ref["half_count"][:, :p.num_tiles]
        assert np.array_equal(got, want), "half counts: " + first_diff(got.ravel(), want.ravel())
        for h, lst in enumerate((res.half0, res.half1)):
            w = ref["half_written"][h]
            assert np.array_equal(lst[w], ref["half"][h][w]), "half %d: %s" % (h, first_diff(lst[w], ref["half"][h][w]))


def as_result(ref, p):
    """a reference dressed as a run's result (CPU: the comparisons against a bent reference)"""
    hc = None
    if "half_count" in ref:
        hc = ref["half_count"].reshape(-1).copy()
    return FakeResult(ref["sorted_keys"], ref["sorted_values"], ref["tile_start"],
                      ref.get("half", [None, None])[0], ref.get("half", [None, None])[1], hc)


def test_bent_references_fail_the_comparisons():
    """ties reversed, searchsorted(..., "right") and a swapped flag bit on the reference side alone: the
    comparisons of the tile-pass cases and of the depth-sort cases tell each from the true one"""
    p, keys, values, _ = make_case("narrow2-4080-s16", "random")
    true = R.reference(keys, values, p.shift, p.all_tiles, False)
    assert_matches(as_result(true, p), true, p)
    for bend in ("ties_reversed", "starts_right"):
        with pytest.raises(AssertionError):
            assert_matches(as_result(true, p), R.reference(keys, values, p.shift, p.all_tiles, False, bend), p)
    p, keys, values = depth_case(300, "equal", "random")
    true = R.reference(keys, values, 16, p.all_tiles, True)
    assert_matches(as_result(true, p), true, p, True, True)
    for bend, full in (("ties_reversed", True), ("ties_reversed", False), ("starts_right", False),
                       ("flags_swapped", False)):
        with pytest.raises(AssertionError):
            assert_matches(as_result(true, p), R.reference(keys, values, 16, p.all_tiles, True, bend), p, True, full)


# ---- CPU: declaration, binding, the host checks ----
def test_entries_are_declared_exported_and_bound(gsm):
    src = open(os.path.join(ROOT, "include", "gsm_debug.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    for name in ("gsm_debug_frame_sort_create", "gsm_debug_frame_sort_destroy", "gsm_debug_frame_sort_run"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert f" T {name}\n" in out, name
        assert name in gsm._SIGNATURES, name
    assert callable(gsm.FrameSort.run) and callable(gsm.FrameSort.close)
    assert [int(x) for x in gsm.FrameSortPlan] == [ONE_NARROW, TWO_NARROW, ONE_WIDE, WIDE_THEN_NARROW]
    assert (R.HALF_SKIP_SHIFT, R.CHUNK, R.SUPER_GROUP, R.TILE_SORT_CAP) == (30, 4096, 32, 2048)
    internal = "".join(open(os.path.join(CSRC, f)).read() for f in ("gsm_internal.h", "gsm_sort.hip", "gsm_sort_plan.h"))
    assert re.search(r"kHalfSkipShift = 30;", internal) and re.search(r"kSuperGroup = 32;", internal)


def test_struct_layouts_match_the_header(gsm, tmp_path):
    import ctypes as C
    prog = tmp_path / "fs.c"
    prog.write_text('#include "gsm_debug.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(gsm_debug_frame_sort_desc),'
                    ' sizeof(gsm_debug_frame_sort_out), offsetof(gsm_debug_frame_sort_desc, full),'
                    ' offsetof(gsm_debug_frame_sort_out, half_count), offsetof(gsm_debug_frame_sort_out, plan));'
                    'return 0;}\n')
    exe = tmp_path / "fs"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, O = gsm._FrameSortDesc, gsm._FrameSortOut
    assert got == [C.sizeof(D), C.sizeof(O), D.full.offset, O.half_count.offset, O.plan.offset]


def test_create_and_null_handle_refusals_need_no_device(gsm):
    import ctypes as C
    L = gsm._lib()
    h = C.c_void_p()
    assert L.gsm_debug_frame_sort_create(0, 16, 0, C.byref(h)) == ERR_CAPACITY
    assert L.gsm_debug_frame_sort_create(16, 0, 0, C.byref(h)) == ERR_TILES
    assert L.gsm_debug_frame_sort_create(16, (1 << 19) + 1, 0, C.byref(h)) == ERR_TILES
    assert L.gsm_debug_frame_sort_create(16, 16, 0, None) == ERR_ARG
    assert not h.value
    desc, out = gsm._FrameSortDesc(16, 1, 1, 0, 0, 0), gsm._FrameSortOut()
    assert L.gsm_debug_frame_sort_run(None, None, C.byref(desc), None, None, 0, C.byref(out)) == ERR_ARG
    L.gsm_debug_frame_sort_destroy(None)


def test_every_check_row_on_the_cpu(tmp_path):
    """tests/host/frame_sort_check_test.cpp: the checks' header alone -- every refusal row and their order, the
    reported plan, the guard on the tile starts -- a stand-alone program built with the address and
    undefined-behaviour sanitizers and run here, with no device and no Python in its process."""
    exe = tmp_path / "frame_sort_check_test"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", "-I" + CSRC, "-o", str(exe), CHECK_SRC], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout


# ---- GPU ----
def open_sorter(gsm, monkeypatch, env, capacity, max_tiles):
    for k in SORT_ENV:  # read at create
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return gsm.FrameSort(capacity, max_tiles)


def on_device(torch, a):
    return torch.from_numpy(a.view(np.int32).copy()).cuda()


def run_tile_pass(gsm, torch, sorter, p, keys, values):
    res = sorter.run(on_device(torch, keys), on_device(torch, values), shift=p.shift, num_tiles=p.num_tiles,
                     all_tiles=p.all_tiles)
    assert res.plan == p.plan, "the case was meant for another plan"
    assert_matches(res, R.reference(keys, values, p.shift, p.all_tiles, False), p)


@pytest.mark.gpu
@pytest.mark.parametrize("plan_name,dist", CASES)
def test_tile_passes(gsm, cuda, monkeypatch, plan_name, dist):
    p, keys, values, cap = make_case(plan_name, dist)
    with open_sorter(gsm, monkeypatch, p.env, cap, p.all_tiles) as s:
        run_tile_pass(gsm, cuda, s, p, keys, values)


@pytest.mark.gpu
@pytest.mark.parametrize("scan", ["none", "kernel"])
@pytest.mark.parametrize("plan_name", REPRESENTATIVES)
def test_two_super_group_rows(gsm, cuda, monkeypatch, plan_name, scan):
    """40 blocks: the scanless passes read two rows (and GSM_SORT_SCAN=kernel none); twice on one handle"""
    p, keys, values, cap = make_case(plan_name, "two_rows")
    with open_sorter(gsm, monkeypatch, dict(p.env, GSM_SORT_SCAN=scan), cap, p.all_tiles) as s:
        run_tile_pass(gsm, cuda, s, p, keys, values)
        run_tile_pass(gsm, cuda, s, p, keys, values)


@pytest.mark.gpu
@pytest.mark.parametrize("rank", ["atomic", "ballot"])
@pytest.mark.parametrize("plan_name", REPRESENTATIVES)
def test_rank_variants(gsm, cuda, monkeypatch, plan_name, rank):
    p = PLAN_BY_NAME[plan_name]
    for dist in ["random", "one_per_tile"] + (["chunk_edges"] if low_bits(p) else []):
        _, keys, values, cap = make_case(plan_name, dist)
        with open_sorter(gsm, monkeypatch, dict(p.env, GSM_SORT_RANK=rank), cap, p.all_tiles) as s:
            run_tile_pass(gsm, cuda, s, p, keys, values)


@pytest.mark.gpu
@pytest.mark.parametrize("scan", ["none", "kernel"])
def test_one_handle_several_sorts(gsm, cuda, monkeypatch, scan):
    """Nothing of one sort is left for the next -- row sets, totals, buckets, tile starts: a full-capacity
    two-pass sort, 10 keys, no keys, the first again; then one-pass, wide, two-pass and wide + 8-bit plans in turn
    on the same handle."""
    cap = 40 * CHUNK
    with open_sorter(gsm, monkeypatch, {"GSM_SORT_SCAN": scan}, cap, 65792) as s:
        rng = np.random.default_rng(77)

        def sort(p, n):
            keys = mixed(rng, p.num_tiles, n).astype(np.uint32)
            run_tile_pass(gsm, cuda, s, p, keys, np.arange(n, dtype=np.uint32))

        two, one, wide, big = (_plan(4080, TWO_NARROW, shift=0), _plan(200, ONE_NARROW, shift=0),
                               _plan(1000, ONE_WIDE, shift=0), _plan(65792, WIDE_THEN_NARROW, shift=0))
        for n in (cap, 10, 0, cap):
            sort(two, n)
        for p, n in ((one, cap), (wide, 5000), (two, 9000), (big, cap), (one, 10), (big, 0), (wide, cap), (two, cap),
                     (big, 3000), (one, 0), (two, 10)):
            sort(p, n)


@pytest.mark.gpu
def test_run_refusals(gsm, cuda, monkeypatch):
    import ctypes as C
    L = gsm._lib()
    k = on_device(cuda, np.zeros(64, np.uint32))
    with open_sorter(gsm, monkeypatch, {}, 32, 100) as s:
        def status(n=16, shift=16, num=50, all_=100, depth=0, full=0, keys=k, values=k):
            desc, out = gsm._FrameSortDesc(shift, num, all_, depth, full, 0), gsm._FrameSortOut()
            return L.gsm_debug_frame_sort_run(s._h, None, C.byref(desc), gsm._ptr(keys), gsm._ptr(values), n,
                                              C.byref(out))
        assert status() == 0
        assert status(n=33) == ERR_ARG
        assert status(num=101) == ERR_ARG and status(all_=101, num=101) == ERR_ARG and status(num=0) == ERR_ARG
        assert status(shift=8) == ERR_ARG and status(shift=0, depth=1) == ERR_ARG
        assert status(keys=None) == ERR_MISSING
        assert status(n=0, keys=None, values=None) == 0


# ---- the depth sort ----
RUNS = [1, 2, 255, 256, 257, 512, 513, 1024, 1025, 2047, 2048, 2049, 5000]
DEPTHS = ["equal", "low_byte", "high_byte", "descending", "extremes"]
FLAGS = ["random", "half0_all", "none"]


def depth_case(num_tiles, depths, flags, all_tiles=None):
    """(plan, keys, values): every run length of RUNS in a tile of its own among small and empty tiles, in random
    input order; depth fields and skip flags as named"""
    rng = np.random.default_rng([num_tiles, DEPTHS.index(depths), FLAGS.index(flags)])
    counts = rng.integers(0, 6, num_tiles)
    crowded = 10 + 3 * np.arange(len(RUNS))
    counts[crowded] = RUNS
    counts[crowded + 1] = 0  # empty tiles between crowded ones
    counts[crowded[-1] + 2] = 0
    counts[num_tiles - 1] = max(counts[num_tiles - 1], 3)
    tiles = rng.permutation(np.repeat(np.arange(num_tiles, dtype=np.int64), counts))
    n = tiles.size
    assert n <= 300_000 and crowded[-1] + 2 < num_tiles - 1
    # the E = 2 / 4 / 8 load variants, the LDS limit and the long-run path
    assert {-(-c // 256) for c in RUNS if c <= R.TILE_SORT_CAP} >= {1, 2, 3, 4, 5, 8}
    assert R.TILE_SORT_CAP in RUNS and R.TILE_SORT_CAP + 1 in RUNS and max(RUNS) > 2 * R.TILE_SORT_CAP
    per_tile = np.bincount(tiles, minlength=num_tiles)
    assert (per_tile[crowded] == RUNS).all() and (per_tile[crowded + 1] == 0).all() and per_tile[num_tiles - 1] > 0
    by_tile = np.argsort(tiles, kind="stable")
    rank = np.empty(n, np.int64)  # position among the keys of the same tile, in input order
    rank[by_tile] = np.arange(n) - np.searchsorted(tiles[by_tile], tiles[by_tile], "left")
    if depths == "equal":
        depth = np.full(n, 0x1234, np.int64)
    elif depths == "low_byte":
        depth = 0x4200 | rng.integers(0, 256, n)
    elif depths == "high_byte":
        depth = (rng.integers(0, 256, n) << 8) | 0x37
    elif depths == "descending":
        depth = 0xFFFF - rank
        assert depth.min() >= 0 and (np.diff(depth[by_tile])[np.diff(tiles[by_tile]) == 0] == -1).all()
    else:
        depth = rng.integers(0, 1 << 16, n)
        for t in (crowded[-1], crowded[RUNS.index(2048)], crowded[RUNS.index(2)]):
            mine = np.flatnonzero(tiles == t)
            depth[mine[0]], depth[mine[-1]] = 0xFFFF, 0x0000
        assert (depth == 0).any() and (depth == 0xFFFF).any()
    if depths in ("equal", "low_byte", "high_byte"):  # ties inside every crowded tile
        assert all(np.unique(depth[tiles == t]).size < c for t, c in zip(crowded[2:], RUNS[2:]))
    ids = rng.permutation(n).astype(np.uint32)
    ids[np.flatnonzero(tiles == crowded[-1])[7]] = R.GID_MASK  # the largest id
    if flags == "random":
        fl = rng.integers(0, 4, n).astype(np.uint32)
    elif flags == "half0_all":
        fl = np.full(n, 1, np.uint32)
    else:
        fl = np.zeros(n, np.uint32)
    values = ids | (fl << np.uint32(R.HALF_SKIP_SHIFT))
    assert (values & R.GID_MASK).max() == R.GID_MASK
    keys = ((tiles << 16) | depth).astype(np.uint32)
    all_tiles = num_tiles if all_tiles is None else all_tiles
    plan = ONE_NARROW if all_tiles <= 256 else (ONE_WIDE if num_tiles <= 2048 else TWO_NARROW)
    return _plan(all_tiles, plan, num_tiles=num_tiles), keys, values


def run_depth_sort(gsm, torch, sorter, p, keys, values, full):
    res = sorter.run(on_device(torch, keys), on_device(torch, values), shift=16, num_tiles=p.num_tiles,
                     all_tiles=p.all_tiles, depth_sort=True, full=full)
    assert res.plan == p.plan
    ref = R.reference(keys, values, 16, p.all_tiles, True)
    if (values >> 30 & 1).all():
        assert not ref["half_count"][0].any() and ref["half_count"][1].sum() == keys.size
    assert_matches(res, ref, p, True, full)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("depths", DEPTHS)
def test_depth_sort(gsm, cuda, monkeypatch, depths, flags, full):
    p, keys, values = depth_case(300, depths, flags)
    with open_sorter(gsm, monkeypatch, {}, keys.size, p.all_tiles) as s:
        run_depth_sort(gsm, cuda, s, p, keys, values, bool(full))


@pytest.mark.gpu
@pytest.mark.parametrize("num_tiles,all_tiles,env", [(200, 200, {}), (2100, 2100, {}), (1800, 16200, {}),
                                                     (300, 300, {"GSM_SORT_RANK": "ballot"}),
                                                     (300, 300, {"GSM_SORT_WIDE": "0"})])
def test_depth_sort_after_every_plan(gsm, cuda, monkeypatch, num_tiles, all_tiles, env):
    """after one narrow pass, two narrow passes, a frame smaller than its configuration (the half counts' stride
    is the configuration's tile count), with ballot ranks and with wide digits off; both on one handle, the
    full sort last (a stale sorted run of the first would show)"""
    p, keys, values = depth_case(num_tiles, "extremes", "random", all_tiles)
    if env.get("GSM_SORT_WIDE") == "0":
        p = p._replace(plan=TWO_NARROW)
    with open_sorter(gsm, monkeypatch, env, keys.size + 100, p.all_tiles) as s:
        run_depth_sort(gsm, cuda, s, p, keys, values, False)
        run_depth_sort(gsm, cuda, s, p, keys[::-1].copy(), values[::-1].copy(), True)


@pytest.mark.gpu
def test_bent_references_fail_against_the_gpu(gsm, cuda, monkeypatch):
    """the three bends of test_bent_references_fail_the_comparisons, against what the GPU wrote"""
    p, keys, values = depth_case(300, "equal", "random")
    with open_sorter(gsm, monkeypatch, {}, keys.size, p.all_tiles) as s:
        res = run_depth_sort(gsm, cuda, s, p, keys, values, True)
    for bend, full in (("ties_reversed", True), ("ties_reversed", False), ("starts_right", False),
                       ("flags_swapped", False)):
        with pytest.raises(AssertionError):
            assert_matches(res, R.reference(keys, values, 16, p.all_tiles, True, bend), p, True, full)
