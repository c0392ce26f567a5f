"""DepthFirst mono frame (gsm_depthfirst_render, include/gsm_depthfirst.h; DESIGN.md "DepthFirst mono").

CPU (`-m "not gpu"`): the restatement of DepthFirstRenderer.render (tests/df_mono/df_mono_ref.c)
checked for the properties the reference's pipeline guarantees, tied to the committed Global oracle
where the two projection kernels compute the same fields, and the ABI surface.
GPU (`-m gpu`): the HIP path through the C ABI against the restatement, bit for bit, on every
intermediate buffer, the colour and the depth.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from test_depthfirst import DF_CASES, _cams, _scene, assert_df_equal, gpu_df
from test_gpu_parity import first_diff, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cam(w, h):
    from gsm_amd import scenes
    return scenes.make_camera(w, h, 0.0)


@functools.lru_cache(maxsize=None)
def _case_ref(name):
    """(world, harm, reference frame) of one DF_CASES shape: computed once, shared, never modified."""
    import df_mono_ref
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    world, harm = _scene(n, w, h, sh, prec, seed, **kw)
    r = df_mono_ref.render(world, harm, sh, _cam(w, h), w, h, color_space=cs)
    assert r["status"] == 0
    return world, harm, r


# ---------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_frame(oracle):
    import df_mono_ref
    n, w, h = 6000, 200, 150
    world, harm = _scene(n, w, h, 9, 1, 7)
    r = df_mono_ref.render(world, harm, 9, _cam(w, h), w, h)
    assert r["status"] == 0
    return r, world, harm


def _passing_tiles_in_depth_order(r):
    """Instances as "expansion in depth order" from the frame's own sorted instances: per gaussian the
    tiles it holds, ascending (ty-major, tx-minor)."""
    per = {}
    for t, g in zip(r["inst_tiles"].tolist(), r["inst_gids"].tolist()):
        per.setdefault(g, []).append(t)
    return per


def test_ref_pipeline_invariants(small_frame):
    r, world, _ = small_frame
    n = len(world)
    touched, keys, order, b = r["touched"], r["depth_keys"], r["depth_order"], r["bounds"]
    vis = np.nonzero(touched > 0)[0]
    assert r["visible"] == len(vis) and 0 < len(vis) <= n
    # stable 32-bit depth order of the visible ids (ascending id among equal keys)
    np.testing.assert_array_equal(order, vis[np.argsort(keys[vis], kind="stable")])
    assert np.all(keys[touched == 0] == 0xFFFFFFFF)
    assert r["overflow"] == 0 and r["total_instances"] == int(touched.sum())
    # touched[g] == number of instances of g
    np.testing.assert_array_equal(np.bincount(r["inst_gids"], minlength=n), touched)
    # every instance tile lies inside bounds[g]
    tiles_x = r["tiles_x"]
    tx, ty = r["inst_tiles"] % tiles_x, r["inst_tiles"] // tiles_x
    bg = b[r["inst_gids"]]
    assert np.all((tx >= bg[:, 0]) & (tx <= bg[:, 1]) & (ty >= bg[:, 2]) & (ty <= bg[:, 3]))
    # instances == expansion in depth order (each gaussian's tiles ascending), then a stable tile sort
    per = _passing_tiles_in_depth_order(r)
    exp_t, exp_g = [], []
    for g in order.tolist():
        ts = per[g]
        assert ts == sorted(ts) and len(set(ts)) == len(ts)
        exp_t += ts
        exp_g += [g] * len(ts)
    exp_t, exp_g = np.array(exp_t), np.array(exp_g)
    srt = np.argsort(exp_t, kind="stable")
    np.testing.assert_array_equal(r["inst_tiles"], exp_t[srt])
    np.testing.assert_array_equal(r["inst_gids"], exp_g[srt])
    # headers: lower bound and count per tile
    t = np.arange(r["tile_count"])
    lo = np.searchsorted(r["inst_tiles"], t, side="left")
    hi = np.searchsorted(r["inst_tiles"], t, side="right")
    np.testing.assert_array_equal(r["headers"][:, 0], lo)
    np.testing.assert_array_equal(r["headers"][:, 1], hi - lo)


def test_ref_prunes_tiles(small_frame):
    """The per-tile test drops tiles of the rect: some visible gaussian has touched < rect area."""
    r, _, _ = small_frame
    b = r["bounds"]
    area = np.maximum(b[:, 1] - b[:, 0] + 1, 0) * np.maximum(b[:, 3] - b[:, 2] + 1, 0)
    vis = r["touched"] > 0
    assert np.all(r["touched"][vis] <= area[vis])
    assert int((r["touched"][vis] < area[vis]).sum()) > 100


def test_ref_ties_to_global_oracle(small_frame, oracle):
    """Bytes 4-15 of the record (theta, sigma1, sigma2, depth, colour, opacity) equal the Global
    oracle's for gaussians visible in both: the two projection kernels compute them identically; the
    fp16 means differ by the half-pixel shift."""
    r, world, harm = small_frame
    w, h = 200, 150
    g = oracle.render(world, harm, 9, _cam(w, h), w, h)
    both = (r["touched"] > 0) & (g["mask"] > 0)
    assert both.sum() > 1000
    a = r["render_data"].view(np.uint8).reshape(-1, 16)[both]
    c = g["render_data"].view(np.uint8).reshape(-1, 16)[both]
    np.testing.assert_array_equal(a[:, 4:], c[:, 4:])
    assert not np.array_equal(a[:, :4], c[:, :4])


def test_ref_d2_cutoff_negative_branch(oracle):
    """Opacities in [0.005, 2/255) pass the opacity cull, quantise to the byte 1 (1/255 < tau) and
    end with touched == 0 (computeD2Cutoff < 0); at the byte 2 the same gaussians are visible."""
    import df_mono_ref
    n, w, h = 3000, 160, 128
    world, harm = _scene(n, w, h, 1, 1, 9, scale_px=3.0)
    lo, hi = world.copy(), world.copy()
    lo["opacity"] = np.float16(0.0078).view(np.uint16)
    hi["opacity"] = np.float16(0.0079).view(np.uint16)
    assert 0.005 <= float(np.float16(0.0078)) < 2 / 255 <= float(np.float16(0.0079))
    a = df_mono_ref.render(lo, harm, 1, _cam(w, h), w, h, max_gaussians=4 * n)
    b = df_mono_ref.render(hi, harm, 1, _cam(w, h), w, h, max_gaussians=4 * n)
    assert b["visible"] > 100 and np.all(b["render_data"]["opacity"][b["touched"] > 0] == 2)
    assert a["visible"] == 0 and a["total_instances"] == 0 and not a["touched"].any()
    assert np.all(a["color"][..., 3] == 0x3C00) and not a["depth"].any()


def test_ref_capacity_clamp(oracle):
    import df_mono_ref
    n, w, h = 3000, 160, 128
    world, harm = _scene(n, w, h, 1, 1, 9, scale_px=3.0)
    full = df_mono_ref.render(world, harm, 1, _cam(w, h), w, h, max_gaussians=4 * n)
    clamped = df_mono_ref.render(world, harm, 1, _cam(w, h), w, h, max_gaussians=n)
    assert full["overflow"] == 0 and full["total_instances"] > 4 * n
    assert clamped["overflow"] == 1 and clamped["total_instances"] == 4 * n
    # the dropped instances are the tail of the depth order: the kept ones are a prefix of the full
    # frame's expansion in depth order
    tiles_x = full["tiles_x"]
    assert tiles_x == clamped["tiles_x"]
    np.testing.assert_array_equal(full["depth_order"], clamped["depth_order"])
    per = _passing_tiles_in_depth_order(full)
    exp = [(g, t) for g in full["depth_order"].tolist() for t in per[g]][:4 * n]
    got = sorted(zip(clamped["inst_gids"].tolist(), clamped["inst_tiles"].tolist()))
    assert got == sorted(exp)


def test_header_declares_and_library_exports_render(gsm):
    hdr = open(os.path.join(ROOT, "include", "gsm_depthfirst.h")).read()
    assert re.search(r"gsm_status\s+gsm_depthfirst_render\s*\(\s*gsm_depthfirst\s*\*", hdr)
    lib = ctypes.CDLL(gsm.library_path())
    assert hasattr(lib, "gsm_depthfirst_render")
    assert hasattr(gsm.DepthFirstRenderer, "render")


# ---------------------------------------------------------------------------
# GPU: HIP path through the C ABI, bit-exact against the restatement
# ---------------------------------------------------------------------------
def gpu_mono(gsm, torch, world, harm, sh, cam, w, h, max_gaussians=None, max_width=None, max_height=None,
             color_space=0, color_format=0, renderer=None, with_depth=True, pad=0):
    """One mono frame; `pad` extra columns in both targets (row pitch wider than the frame)."""
    prec = 1 if world.dtype.itemsize == 32 else 0
    n = len(world)
    if renderer is None:
        cfg = gsm.RendererConfig(max_gaussians=max_gaussians or max(n, 1), max_width=max_width or w,
                                 max_height=max_height or h, precision=prec, gaussian_color_space=color_space,
                                 color_format=color_format)
        renderer = gsm.DepthFirstRenderer(config=cfg)
    renderer.set_profiling(True)
    fmt = gsm.ColorFormat(color_format)
    dt = torch.float16 if fmt == gsm.ColorFormat.RGBA16F else (torch.float32 if fmt == gsm.ColorFormat.RGBA32F
                                                                else torch.uint8)
    color = torch.full((h, w + pad, 4), 7, dtype=dt, device="cuda")
    if dt == torch.float16:
        color.fill_(float("nan"))
    depth = torch.full((h, w + pad), float("nan"), dtype=torch.float16, device="cuda")
    inp = gsm.GaussianInput(to_dev(torch, world), to_dev(torch, harm), n, sh)
    renderer.render(color, depth if with_depth else None, inp, gsm.CameraParams.from_dict(cam), w, h,
                    color_pitch=(w + pad) * fmt.bytes_per_pixel, depth_pitch=(w + pad) * 2)
    torch.cuda.synchronize()
    B = gsm.DepthFirstBuffer
    out = {"counters": renderer.counters(), "stage_ms": renderer.stage_times_ms(), "renderer": renderer}
    c = color.cpu().numpy()
    out["color_full"] = c.view(np.uint16) if dt == torch.float16 else c
    out["depth_full"] = depth.cpu().numpy().view(np.uint16)
    out["color"] = out["color_full"][:, :w]
    out["depth"] = out["depth_full"][:, :w]
    for name, which in (("render_data", B.RENDER_DATA), ("bounds", B.BOUNDS), ("touched", B.TOUCHED),
                        ("depth_keys", B.DEPTH_KEYS), ("depth_order", B.DEPTH_ORDER),
                        ("inst_tiles", B.INSTANCE_TILES), ("inst_gids", B.INSTANCE_GAUSSIANS),
                        ("headers", B.HEADERS)):
        out[name] = renderer.copy_buffer(which)
    return out


def assert_mono_equal(g, r, color=True, depth=True):
    c = g["counters"]
    assert (c["visible"], c["total_instances"], c["overflow"]) == \
        (r["visible"], r["total_instances"], r["overflow"])
    assert (c["tiles_x"], c["tiles_y"]) == (r["tiles_x"], r["tiles_y"])
    np.testing.assert_array_equal(g["touched"], r["touched"], err_msg=first_diff(g["touched"], r["touched"]))
    np.testing.assert_array_equal(g["bounds"], r["bounds"])
    np.testing.assert_array_equal(g["depth_keys"], r["depth_keys"])
    assert g["render_data"].dtype.itemsize == 16
    vis = r["touched"] > 0
    grd = g["render_data"].view(np.uint8).reshape(-1, 16)[vis]
    ord_ = r["render_data"].view(np.uint8).reshape(-1, 16)[vis]
    if not np.array_equal(grd, ord_):
        bad = np.nonzero((grd != ord_).any(1))[0][:3]
        raise AssertionError(f"render_data differs at visible rows {bad}: {grd[bad]} vs {ord_[bad]}")
    np.testing.assert_array_equal(g["depth_order"], r["depth_order"])
    np.testing.assert_array_equal(g["inst_tiles"], r["inst_tiles"])
    np.testing.assert_array_equal(g["inst_gids"], r["inst_gids"])
    np.testing.assert_array_equal(g["headers"], r["headers"])
    if color:
        assert np.array_equal(g["color"], r["color"]), first_diff(g["color"], r["color"])
    if depth:
        assert np.array_equal(g["depth"], r["depth"]), first_diff(g["depth"], r["depth"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DF_CASES))
def test_mono_bit_exact(gsm, cuda, oracle, name):
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    world, harm, r = _case_ref(name)
    g = gpu_mono(gsm, cuda, world, harm, sh, _cam(w, h), w, h, color_space=cs)
    assert_mono_equal(g, r)
    g["renderer"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"GSM_SORT_WIDE": "0"}, {"GSM_SORT_RANK": "ballot"}])
def test_mono_sort_switches(gsm, cuda, oracle, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name = "sh2_f16_config5_shape"
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    world, harm, r = _case_ref(name)
    g = gpu_mono(gsm, cuda, world, harm, sh, _cam(w, h), w, h, color_space=cs)
    assert_mono_equal(g, r)
    g["renderer"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,w,h,sh,seed", [("f16", 30_000, 360, 400, 9, 21), ("f32", 20_000, 250, 170, 1, 22)])
def test_mono_adversarial_scenes_bit_exact(gsm, cuda, oracle, kind, n, w, h, sh, seed):
    """tests/adversarial.py scenes (zero / extreme / inf / NaN scales, positions and quaternions,
    opacities around the cull, huge / NaN SH; rects of thousands of tiles) through the mono frame."""
    import adversarial
    import df_mono_ref
    case = adversarial.scene(kind, n, w, h, sh, seed)
    mg = 4 * n
    r = df_mono_ref.render(case["world"], case["harm"], sh, _cam(w, h), w, h, max_gaussians=mg)
    assert r["status"] == 0 and r["overflow"] == 0
    g = gpu_mono(gsm, cuda, case["world"], case["harm"], sh, _cam(w, h), w, h, max_gaussians=mg)
    assert_mono_equal(g, r)
    g["renderer"].close()


@pytest.mark.gpu
def test_mono_capacity_clamp(gsm, cuda, oracle):
    """More passing tiles than 4 * max_gaussians: the dropped tail of the depth order matches."""
    import df_mono_ref
    n, w, h = 3000, 160, 128
    world, harm = _scene(n, w, h, 1, 1, 9, scale_px=3.0)
    r = df_mono_ref.render(world, harm, 1, _cam(w, h), w, h, max_gaussians=n)
    assert r["overflow"] == 1 and r["total_instances"] == 4 * n
    g = gpu_mono(gsm, cuda, world, harm, 1, _cam(w, h), w, h, max_gaussians=n)
    assert_mono_equal(g, r)
    g["renderer"].close()


@pytest.mark.gpu
def test_mono_null_depth_target(gsm, cuda, oracle):
    name = "sh0_f32_ragged"
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    world, harm, r = _case_ref(name)
    g = gpu_mono(gsm, cuda, world, harm, sh, _cam(w, h), w, h, color_space=cs, with_depth=False)
    assert_mono_equal(g, r, depth=False)
    assert np.all(g["depth_full"] == 0x7E00)  # the NaN fill, untouched
    g["renderer"].close()


@pytest.mark.gpu
def test_mono_inside_larger_configuration_with_wide_pitch(gsm, cuda, oracle):
    """250x170 inside a 512x512 configuration, rows 37 pixels wider than the frame: bytes outside the
    frame stay untouched."""
    name = "sh0_f32_ragged"
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    world, harm, r = _case_ref(name)
    g = gpu_mono(gsm, cuda, world, harm, sh, _cam(w, h), w, h, color_space=cs, max_width=512, max_height=512,
                 pad=37)
    assert_mono_equal(g, r)
    assert np.all(g["color_full"][:, w:] == 0x7E00) and np.all(g["depth_full"][:, w:] == 0x7E00)
    g["renderer"].close()


@pytest.mark.gpu
def test_mono_color_format_bgra8_srgb(gsm, cuda, oracle):
    name = "sh0_f32_ragged"
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    world, harm, r = _case_ref(name)
    fmt = int(gsm.ColorFormat.BGRA8_UNORM_SRGB)
    g = gpu_mono(gsm, cuda, world, harm, sh, _cam(w, h), w, h, color_space=cs, color_format=fmt)
    assert_mono_equal(g, r, color=False)
    np.testing.assert_array_equal(g["color"], oracle.convert_color(r["color"], fmt))
    g["renderer"].close()


@pytest.mark.gpu
def test_mono_stereo_mono_on_one_handle(gsm, cuda, oracle):
    """A mono frame, a stereo frame, then a mono frame on one handle, each bit-exact: the shared
    arena carries nothing over, and the debug buffers describe the last frame, whichever kind."""
    name = "sh0_f32_ragged"
    n, w, h, sh, prec, cs, seed, kw = DF_CASES[name]
    world, harm, r = _case_ref(name)
    L, R = _cams(w, h)
    rs = oracle.df_render_stereo(world, harm, sh, L, R, w, h, color_space=cs)
    g1 = gpu_mono(gsm, cuda, world, harm, sh, _cam(w, h), w, h, color_space=cs)
    assert_mono_equal(g1, r)
    rend = g1["renderer"]
    gs = gpu_df(gsm, cuda, world, harm, sh, L, R, w, h, color_space=cs, renderer=rend)
    assert gs["render_data"].dtype.itemsize == 32
    assert_df_equal(gs, rs)
    g2 = gpu_mono(gsm, cuda, world, harm, sh, _cam(w, h), w, h, color_space=cs, renderer=rend)
    assert_mono_equal(g2, r)
    assert rend.last_gpu_time is not None and set(g2["stage_ms"]) == set(gsm.DF_STAGES)
    rend.close()


@pytest.mark.gpu
def test_mono_errors(gsm, cuda):
    w, h = 64, 48
    rend = gsm.DepthFirstRenderer(config=gsm.RendererConfig(max_gaussians=16, max_width=w, max_height=h))
    x = cuda.zeros(w * h * 8, dtype=cuda.uint8, device="cuda")
    cam = gsm.CameraParams.from_dict(_cam(w, h))
    for count, ww, col, status in ((0, w, x, gsm.Status.INVALID_GAUSSIAN_COUNT),
                                   (17, w, x, gsm.Status.INVALID_GAUSSIAN_COUNT),
                                   (1, w + 1, x, gsm.Status.INVALID_DIMENSIONS),
                                   (1, 0, x, gsm.Status.INVALID_DIMENSIONS),
                                   (1, w, None, gsm.Status.MISSING_REQUIRED_BUFFER)):
        with pytest.raises(gsm.RendererError) as e:
            rend.render(col, None, gsm.GaussianInput(x, x, count, 1), cam, ww, h)
        assert e.value.status == status
    rend.close()
