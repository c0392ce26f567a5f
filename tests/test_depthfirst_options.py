"""DepthFirst create options: 16-bit depth keys and 32-bit tile ids (gsm_depthfirst_create_with_options,
include/gsm_depthfirst.h; DESIGN.md "DepthFirst create options").

CPU (`-m "not gpu"`): the restatement with the two parameters (tests/df_options/df_options_ref.c) tied to the
two existing checkers at the defaults, its 16-bit key derived independently in numpy, the scenes that make
each option observable, and the ABI surface.
GPU (`-m gpu`): the HIP path through the C ABI against that restatement, bit for bit, on every debug buffer
(the sorted depth keys included), the counters, the colour and, for mono frames, the depth.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import df_options_scenes as S
from test_depthfirst import DF_CASES, _cams, _scene, assert_df_equal, gpu_df
from test_depthfirst_mono import _cam, assert_mono_equal, gpu_mono

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = "sh0_f32_ragged"  # the smallest DF_CASES scene
MODES = [(16, 16), (16, 32), (32, 32)]


# ---------------------------------------------------------------------------
# shared references: computed once, never modified
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_scene(name):
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    return _scene(n, w, h, sh, prec, seed, **kw)


@functools.lru_cache(maxsize=None)
def _ref(kind, name, bits):
    """The restatement's frame of a DF_CASES shape in mode `bits` = (depth_key_bits, tile_id_bits)."""
    import df_options_ref
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    world, harm = _case_scene(name)
    if kind == "mono":
        r = df_options_ref.render_mono(world, harm, sh, _cam(w, h), w, h, bits[0], bits[1], color_space=cs)
    else:
        L, R = _cams(w, h)
        r = df_options_ref.render_stereo(world, harm, sh, L, R, w, h, bits[0], bits[1], color_space=cs)
    assert r["status"] == 0
    return r


@functools.lru_cache(maxsize=None)
def _ties_ref(kind, bits, max_gaussians=None):
    import df_options_ref
    world, harm = S.depth_ties()
    w, h = 160, 128
    mg = max_gaussians or 8 * len(world)
    if kind == "mono":
        r = df_options_ref.render_mono(world, harm, 1, S.cam(w, h), w, h, bits[0], bits[1], max_gaussians=mg)
    else:
        L, R = S.cams(w, h)
        r = df_options_ref.render_stereo(world, harm, 1, L, R, w, h, bits[0], bits[1], max_gaussians=mg)
    assert r["status"] == 0
    return r


@functools.lru_cache(maxsize=None)
def _big_ref(kind):
    import df_options_ref
    world, harm = S.big_grid()
    w, h = S.BIG_W, S.BIG_H
    mg = 8 * len(world)
    if kind == "mono":
        r = df_options_ref.render_mono(world, harm, 1, S.cam(w, h), w, h, 32, 32, max_gaussians=mg)
    else:
        L, R = S.cams(w, h)
        r = df_options_ref.render_stereo(world, harm, 1, L, R, w, h, 32, 32, max_gaussians=mg, eye_color=False)
    assert r["status"] == 0 and r["overflow"] == 0
    return r


@functools.lru_cache(maxsize=None)
def _dense_ref(kind):
    import df_options_ref
    n = S.DENSE_N[kind]
    world, harm = S.big_grid_dense(n)
    w, h = S.BIG_W, S.BIG_H
    if kind == "mono":
        r = df_options_ref.render_mono(world, harm, 1, S.cam(w, h), w, h, 32, 32, max_gaussians=8 * n)
    else:
        L, R = S.cams(w, h)
        r = df_options_ref.render_stereo(world, harm, 1, L, R, w, h, 32, 32, max_gaussians=8 * n, eye_color=False)
    assert r["status"] == 0 and r["overflow"] == 0
    return r


def _key16(pre_keys):
    """The 16-bit key from the 32-bit sortable key, in numpy: undo the sortable mapping, round the fp32
    depth to fp16 (nearest even, overflow to inf), flip the sign bit."""
    k = np.asarray(pre_keys, np.uint32)
    bits = np.where(k & 0x80000000, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    with np.errstate(over="ignore"):
        half = bits.view(np.float32).astype(np.float16)
    return (half.view(np.uint16) ^ np.uint16(0x8000)).astype(np.uint32)


# ---------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------
def test_ref_defaults_equal_existing_checkers(oracle):
    """1. (32, 16) is og_df_render_stereo and dfm_render byte for byte: every intermediate, colour, depth."""
    import df_mono_ref
    name = SMALL
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    world, harm = _case_scene(name)
    L, R = _cams(w, h)
    a = oracle.df_render_stereo(world, harm, sh, L, R, w, h, color_space=cs)
    b = _ref("stereo", name, (32, 16))
    for k in ("visible", "total_instances", "overflow", "tiles_x", "tiles_y", "tile_count", "active_tiles",
              "max_instances"):
        assert a[k] == b[k], k
    for k in ("render_data", "bounds", "touched", "depth_keys", "depth_order", "inst_tiles", "inst_gids", "headers",
              "eye_color", "color"):
        assert a[k].tobytes() == b[k].tobytes(), k
    am = df_mono_ref.render(world, harm, sh, _cam(w, h), w, h, color_space=cs)
    bm = _ref("mono", name, (32, 16))
    for k in ("visible", "total_instances", "overflow", "tiles_x", "tiles_y", "tile_count", "active_tiles",
              "max_instances"):
        assert am[k] == bm[k], k
    for k in ("render_data", "bounds", "touched", "depth_keys", "depth_order", "inst_tiles", "inst_gids", "headers",
              "color", "depth"):
        assert am[k].tobytes() == bm[k].tobytes(), k
    # the sorted keys of the 32-bit mode are the 32-bit keys in depth order
    np.testing.assert_array_equal(b["sorted_keys"], b["depth_keys"][b["depth_order"]])
    np.testing.assert_array_equal(bm["sorted_keys"], bm["depth_keys"][bm["depth_order"]])


@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_ref_key16_independent_derivation(oracle, kind):
    """2. The sorted 16-bit keys and the depth order from numpy alone."""
    r = _ref(kind, SMALL, (16, 16))
    vis = np.nonzero(r["touched"] > 0)[0]
    assert len(vis) == r["visible"] > 1000
    k16 = _key16(r["depth_keys"][vis])
    order = np.argsort(k16, kind="stable")
    np.testing.assert_array_equal(r["sorted_keys"], k16[order])
    np.testing.assert_array_equal(r["depth_order"], vis[order])
    assert np.all(r["sorted_keys"] < 65536)
    # a depth above 65504 becomes +inf: bits 0x7C00 ^ 0x8000
    big = np.array([0x80000000 | np.float32(70000.0).view(np.uint32)], np.uint32)
    assert _key16(big)[0] == 0xFC00


def test_ref_depth_tie_scene(oracle):
    """3. The depth-tie scene makes the 16-bit order observable."""
    a, b = _ties_ref("mono", (16, 16)), _ties_ref("mono", (32, 16))
    np.testing.assert_array_equal(a["depth_keys"], b["depth_keys"])
    vis = np.nonzero(a["touched"] > 0)[0]
    pre = a["depth_keys"][vis]
    k16 = _key16(pre)
    o = np.argsort(k16, kind="stable")
    same16 = k16[o][1:] == k16[o][:-1]
    diff32 = pre[o][1:] != pre[o][:-1]
    assert int((same16 & diff32).sum()) >= 100
    assert not np.array_equal(a["depth_order"], b["depth_order"])
    assert sorted(a["depth_order"].tolist()) == sorted(b["depth_order"].tolist())
    assert not np.array_equal(a["color"], b["color"])
    s16, s32 = _ties_ref("stereo", (16, 16)), _ties_ref("stereo", (32, 16))
    assert not np.array_equal(s16["depth_order"], s32["depth_order"])
    assert not np.array_equal(s16["color"], s32["color"])


@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_ref_grid_above_65535_tiles(oracle, kind):
    """4. 65,792 tiles: instances in tile ids >= 65,536 and in the ids they would alias to."""
    r = _big_ref(kind)
    assert (r["tiles_x"], r["tiles_y"], r["tile_count"]) == (257, 256, 65792)
    t = r["inst_tiles"]
    high = np.unique(t[t >= 65536])
    assert len(high) >= 100 and int(t.max()) < 65792
    aliased = np.intersect1d(high - 65536, t)
    assert len(aliased) >= 50
    assert np.all(np.diff(t.astype(np.int64)) >= 0)
    hi_hdr = r["headers"][65536:]
    assert int(hi_hdr[:, 1].sum()) == int((t >= 65536).sum())
    # the pixels of those tiles were blended: the bottom tile row is not all clear
    if kind == "mono":
        assert np.any(r["color"][S.BIG_H - 16:, :, :3] != 0)
    else:  # (the copy pass flips rows: the bottom tile row lands in the first target rows)
        assert np.any(r["color"][:16, :, :3] != 0)


@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_ref_dense_grid_spans_blocks(oracle, kind):
    """4b. The dense 65,792-tile scene gives the two-pass tile sort several workgroups of work in both passes
    (4096 instances a block): more than 8192 instances, hundreds of them in tile ids >= 65,536, and among the
    512 low-digit buckets of its 17-bit tile field (9 + 8 bits) non-empty ones that start inside a block, and
    one that starts exactly on a block boundary.  (The sort's grid is ceil(max_instances / 4096) <= 1024
    workgroups and a workgroup's share is rounded up to whole 4096-key chunks: here one chunk each.)"""
    r = _dense_ref(kind)
    t = r["inst_tiles"]
    tot = r["total_instances"]
    assert r["tile_count"] == 65792 and tot > 8192 and tot <= r["max_instances"] < 1024 * 4096
    assert int((t >= 65536).sum()) > 1000 and len(np.intersect1d(t[t >= 65536] - 65536, t)) >= 50
    cnt = np.bincount(t & 511, minlength=512)
    start = np.cumsum(cnt) - cnt
    live = cnt > 0
    assert int(live.sum()) > 400
    on = live & (start % 4096 == 0) & (start > 0)
    assert on.any()
    blocks = np.unique(start[live & ~on] // 4096)
    assert len(blocks) == -(-tot // 4096)  # every block of the last pass holds bucket starts


def test_options_abi_surface(gsm):
    """5. Header, exports, struct size, defaults, Python surface."""
    hdr = open(os.path.join(ROOT, "include", "gsm_depthfirst.h")).read()
    assert re.search(r"void\s+gsm_depthfirst_default_options\s*\(\s*gsm_depthfirst_options\s*\*", hdr)
    assert re.search(r"gsm_status\s+gsm_depthfirst_create_with_options\s*\(", hdr)
    assert re.search(r"gsm_status\s+gsm_depthfirst_get_options\s*\(\s*gsm_depthfirst\s*\*", hdr)
    assert re.search(r"GSM_DF_BUF_SORTED_DEPTH_KEYS\s*=\s*9\b", hdr)
    assert re.search(r"#define\s+GSM_DF_MAX_TILES_32\s+(\d+)u", hdr)
    assert int(re.search(r"#define\s+GSM_DF_MAX_TILES_32\s+(\d+)u", hdr).group(1)) >= 262144
    lib = ctypes.CDLL(gsm.library_path())
    for fn in ("gsm_depthfirst_default_options", "gsm_depthfirst_create_with_options", "gsm_depthfirst_get_options"):
        assert hasattr(lib, fn), fn
    assert ctypes.sizeof(gsm._DfOptions) == 16

    class Opt(ctypes.Structure):
        _fields_ = [(f, ctypes.c_uint32) for f in ("struct_bytes", "depth_key_bits", "tile_id_bits", "reserved")]
    o = Opt(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    lib.gsm_depthfirst_default_options.restype = None
    lib.gsm_depthfirst_default_options(ctypes.byref(o))
    assert (o.struct_bytes, o.depth_key_bits, o.tile_id_bits, o.reserved) == (16, 32, 16, 0)
    assert isinstance(gsm.DepthFirstRenderer.options, property)
    assert int(gsm.DepthFirstBuffer.SORTED_DEPTH_KEYS) == 9


# ---------------------------------------------------------------------------
# GPU: HIP path through the C ABI, bit-exact against the restatement
# ---------------------------------------------------------------------------
def _renderer(gsm, world, w, h, bits, max_gaussians=None, color_space=0):
    prec = 1 if world.dtype.itemsize == 32 else 0
    cfg = gsm.RendererConfig(max_gaussians=max_gaussians or max(len(world), 1), max_width=w, max_height=h,
                             precision=prec, gaussian_color_space=color_space)
    return gsm.DepthFirstRenderer(config=cfg, depth_key_bits=bits[0], tile_id_bits=bits[1])


def _gpu(gsm, torch, kind, rend, world, harm, sh, w, h, color_space=0, cams=None):
    if kind == "mono":
        g = gpu_mono(gsm, torch, world, harm, sh, cams or _cam(w, h), w, h, color_space=color_space, renderer=rend)
    else:
        L, R = cams or _cams(w, h)
        g = gpu_df(gsm, torch, world, harm, sh, L, R, w, h, color_space=color_space, renderer=rend)
    g["sorted_keys"] = rend.copy_buffer(gsm.DepthFirstBuffer.SORTED_DEPTH_KEYS)
    return g


def _assert_equal(kind, g, r):
    (assert_mono_equal if kind == "mono" else assert_df_equal)(g, r)
    assert g["sorted_keys"].dtype == np.uint32
    np.testing.assert_array_equal(g["sorted_keys"], r["sorted_keys"])
    assert g["counters"]["tile_count"] == r["tile_count"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mono", "stereo"])
@pytest.mark.parametrize("bits", MODES)
def test_mode_grid_bit_exact(gsm, cuda, oracle, bits, kind):
    """6. Every mode on the smallest DF_CASES scene."""
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[SMALL]
    world, harm = _case_scene(SMALL)
    rend = _renderer(gsm, world, w, h, bits, color_space=cs)
    g = _gpu(gsm, cuda, kind, rend, world, harm, sh, w, h, color_space=cs)
    _assert_equal(kind, g, _ref(kind, SMALL, bits))
    assert rend.options == {"depth_key_bits": bits[0], "tile_id_bits": bits[1]}
    rend.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_depth_tie_scene_gpu(gsm, cuda, oracle, kind):
    """7. (16, 16) on the depth-tie scene equals the restatement and differs from (32, 16)."""
    world, harm = S.depth_ties()
    w, h = 160, 128
    cams = S.cam(w, h) if kind == "mono" else S.cams(w, h)
    out = {}
    for bits in ((16, 16), (32, 16)):
        rend = _renderer(gsm, world, w, h, bits, max_gaussians=8 * len(world))
        g = _gpu(gsm, cuda, kind, rend, world, harm, 1, w, h, cams=cams)
        _assert_equal(kind, g, _ties_ref(kind, bits))
        out[bits] = g
        rend.close()
    assert not np.array_equal(out[(16, 16)]["depth_order"], out[(32, 16)]["depth_order"])
    assert not np.array_equal(out[(16, 16)]["color"], out[(32, 16)]["color"])
    assert not np.array_equal(out[(16, 16)]["sorted_keys"], out[(32, 16)]["sorted_keys"])


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"GSM_SORT_WIDE": "0"}, {"GSM_SORT_RANK": "ballot"}])
def test_key16_sort_switches(gsm, cuda, oracle, monkeypatch, env):
    """8. The create-time sort switches leave the 16-bit frame unchanged."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[SMALL]
    world, harm = _case_scene(SMALL)
    for kind in ("mono", "stereo"):
        rend = _renderer(gsm, world, w, h, (16, 16), color_space=cs)
        g = _gpu(gsm, cuda, kind, rend, world, harm, sh, w, h, color_space=cs)
        _assert_equal(kind, g, _ref(kind, SMALL, (16, 16)))
        rend.close()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 257])
def test_key16_edge_counts(gsm, cuda, oracle, count):
    """9. One gaussian, and one past a 256 block, in 16-bit mode (mono and stereo)."""
    import df_options_ref
    world, harm = S.depth_ties()
    world, harm = world[:count].copy(), harm.reshape(-1, 3)[:count].reshape(-1).copy()
    w, h = 160, 128
    for kind in ("mono", "stereo"):
        rend = _renderer(gsm, world, w, h, (16, 16), max_gaussians=64 * count)
        if kind == "mono":
            cams = S.cam(w, h)
            r = df_options_ref.render_mono(world, harm, 1, cams, w, h, 16, 16, max_gaussians=64 * count)
        else:
            cams = S.cams(w, h)
            r = df_options_ref.render_stereo(world, harm, 1, cams[0], cams[1], w, h, 16, 16, max_gaussians=64 * count)
        assert r["status"] == 0 and r["visible"] == count
        g = _gpu(gsm, cuda, kind, rend, world, harm, 1, w, h, cams=cams)
        _assert_equal(kind, g, r)
        rend.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_key16_nothing_visible(gsm, cuda, oracle, kind):
    """9. A scene behind the camera: visible count 0, the frame comes out cleared, no error."""
    import df_options_ref
    world, harm = S.depth_ties()
    world, harm = world[:257].copy(), harm.reshape(-1, 3)[:257].reshape(-1).copy()
    world["pz"] = -world["pz"]
    w, h = 160, 128
    rend = _renderer(gsm, world, w, h, (16, 16))
    if kind == "mono":
        cams = S.cam(w, h)
        r = df_options_ref.render_mono(world, harm, 1, cams, w, h, 16, 16)
    else:
        cams = S.cams(w, h)
        r = df_options_ref.render_stereo(world, harm, 1, cams[0], cams[1], w, h, 16, 16)
    assert r["status"] == 0 and r["visible"] == 0 and r["total_instances"] == 0
    g = _gpu(gsm, cuda, kind, rend, world, harm, 1, w, h, cams=cams)
    _assert_equal(kind, g, r)
    assert len(g["sorted_keys"]) == 0
    assert np.all(g["color"][..., :3] == 0) and np.all(g["color"][..., 3] == 0x3C00)
    if kind == "mono":
        assert not g["depth"].any()
    rend.close()


@pytest.mark.gpu
def test_key16_capacity_clamp(gsm, cuda, oracle):
    """10. More passing tiles than 4 * max_gaussians in 16-bit mode: overflow is set and the dropped
    instances are the tail of the 16-bit depth order (the shape of test_mono_capacity_clamp)."""
    import df_options_ref
    n, w, h = 3000, 160, 128
    world, harm = _scene(n, w, h, 1, 1, 9, scale_px=3.0)
    full = df_options_ref.render_mono(world, harm, 1, _cam(w, h), w, h, 16, 16, max_gaussians=4 * n)
    r = df_options_ref.render_mono(world, harm, 1, _cam(w, h), w, h, 16, 16, max_gaussians=n)
    assert full["overflow"] == 0 and full["total_instances"] > 4 * n
    assert r["overflow"] == 1 and r["total_instances"] == 4 * n
    r32 = df_options_ref.render_mono(world, harm, 1, _cam(w, h), w, h, 32, 16, max_gaussians=n)
    assert not np.array_equal(r["depth_order"], r32["depth_order"])
    rend = _renderer(gsm, world, w, h, (16, 16), max_gaussians=n)
    g = _gpu(gsm, cuda, "mono", rend, world, harm, 1, w, h)
    _assert_equal("mono", g, r)
    assert g["counters"]["overflow"] == 1
    # the kept instances are the first 4 n of the full frame's expansion in the 16-bit depth order
    per = {}
    for t, gid in zip(full["inst_tiles"].tolist(), full["inst_gids"].tolist()):
        per.setdefault(gid, []).append(t)
    exp = [(gid, t) for gid in full["depth_order"].tolist() for t in per[gid]][:4 * n]
    assert sorted(zip(g["inst_gids"].tolist(), g["inst_tiles"].tolist())) == sorted(exp)
    rend.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_above_65535_tiles_gpu(gsm, cuda, oracle, kind):
    """11. 65,792 tiles per eye in (32, 32): instances, headers and every pixel of the 4112 x 4096 mono
    and the 8224 x 4096 stereo target."""
    world, harm = S.big_grid()
    w, h = S.BIG_W, S.BIG_H
    r = _big_ref(kind)
    rend = _renderer(gsm, world, w, h, (32, 32), max_gaussians=8 * len(world))
    cams = S.cam(w, h) if kind == "mono" else S.cams(w, h)
    g = _gpu(gsm, cuda, kind, rend, world, harm, 1, w, h, cams=cams)
    assert int(g["inst_tiles"].max()) >= 65536
    _assert_equal(kind, g, r)
    assert g["color"].shape == ((h, w, 4) if kind == "mono" else (h, 2 * w, 4))
    rend.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"GSM_SORT_RANK": "ballot"}])
@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_above_65535_tiles_many_blocks_gpu(gsm, cuda, oracle, monkeypatch, kind, env):
    """11b. The dense scene on the 65,792-tile grid in (32, 32): tens of thousands of instances, so both passes
    of the wide tile sort run in several workgroups, with bucket starts inside blocks and on a block boundary
    (test_ref_dense_grid_spans_blocks); once with lane-ordered ranks and once with ballot ranks."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = S.DENSE_N[kind]
    world, harm = S.big_grid_dense(n)
    w, h = S.BIG_W, S.BIG_H
    r = _dense_ref(kind)
    rend = _renderer(gsm, world, w, h, (32, 32), max_gaussians=8 * n)
    cams = S.cam(w, h) if kind == "mono" else S.cams(w, h)
    g = _gpu(gsm, cuda, kind, rend, world, harm, 1, w, h, cams=cams)
    print(f"{kind} {env} stage_ms {g['stage_ms']} instances {g['counters']['total_instances']}")
    _assert_equal(kind, g, r)
    rend.close()


@pytest.mark.gpu
def test_options_errors(gsm, cuda):
    """12. Create-time errors of the options."""
    L = gsm._lib()
    St = gsm.Status

    def create(w, h, opt, out=True):
        cfg = gsm._Config(64, w, h, 0, 0, 0, 0)
        hnd = ctypes.c_void_p()
        st = L.gsm_depthfirst_create_with_options(ctypes.byref(cfg), -1, ctypes.byref(opt) if opt is not None else None,
                                                  ctypes.byref(hnd) if out else None)
        if st == 0:
            L.gsm_depthfirst_destroy(hnd)
        return st

    O = gsm._DfOptions
    assert create(64, 64, None) == St.OK
    assert create(64, 64, O(16, 16, 32, 0)) == St.OK
    for bits in ((16, 16), (32, 16)):
        assert create(S.BIG_W, S.BIG_H, O(16, bits[0], bits[1], 0)) == St.INVALID_TILE_COUNT
    assert create(S.BIG_W, S.BIG_H, None) == St.INVALID_TILE_COUNT
    assert create(64, 64, O(16, 8, 16, 0)) == St.INVALID_ARGUMENT
    assert create(64, 64, O(16, 32, 8, 0)) == St.INVALID_ARGUMENT
    assert create(64, 64, O(12, 32, 16, 0)) == St.INVALID_ARGUMENT
    assert create(64, 64, O(20, 32, 16, 0)) == St.INVALID_ARGUMENT
    assert create(64, 64, O(16, 32, 16, 1)) == St.INVALID_ARGUMENT
    assert create(64, 64, O(16, 16, 32, 0), out=False) == St.INVALID_ARGUMENT
    hdr = open(os.path.join(ROOT, "include", "gsm_depthfirst.h")).read()
    limit = int(re.search(r"#define\s+GSM_DF_MAX_TILES_32\s+(\d+)u", hdr).group(1))
    tx = 1024
    ty = limit // tx + 1
    assert create(16 * tx, 16 * ty, O(16, 32, 32, 0)) == St.INVALID_TILE_COUNT
    # more than GSM_DF_MAX_TILES_AXIS tiles along one axis (tile rects are 16-bit signed), inside the limit
    axis = int(re.search(r"#define\s+GSM_DF_MAX_TILES_AXIS\s+(\d+)u", hdr).group(1))
    assert axis == 32767 and (axis + 1) * 8 <= limit
    assert create(16 * (axis + 1), 16 * 8, O(16, 32, 32, 0)) == St.INVALID_TILE_COUNT
    assert create(16 * 8, 16 * (axis + 1), O(16, 32, 32, 0)) == St.INVALID_TILE_COUNT
    with pytest.raises(gsm.RendererError) as e:
        gsm.DepthFirstRenderer(config=gsm.RendererConfig(max_gaussians=16, max_width=64, max_height=64),
                               depth_key_bits=24)
    assert e.value.status == St.INVALID_ARGUMENT
    o = O()
    assert L.gsm_depthfirst_get_options(None, ctypes.byref(o)) == St.INVALID_ARGUMENT


@pytest.mark.gpu
def test_mixed_frames_on_one_handle(gsm, cuda, oracle):
    """13. Mono, stereo, mono on one (16, 32) handle, each frame exact."""
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[SMALL]
    world, harm = _case_scene(SMALL)
    rend = _renderer(gsm, world, w, h, (16, 32), color_space=cs)
    for kind in ("mono", "stereo", "mono"):
        g = _gpu(gsm, cuda, kind, rend, world, harm, sh, w, h, color_space=cs)
        _assert_equal(kind, g, _ref(kind, SMALL, (16, 32)))
        assert rend.options == {"depth_key_bits": 16, "tile_id_bits": 32}
    rend.close()
