"""LocalRenderer frame, GPU side (gsm_local_render, include/gsm_local.h).

The HIP path through the C ABI against the restatement (tests/local/local_ref.c), bit for bit: the
colour target, the depth target, the counters, PROJECTED, TILE_COUNTS and TILE_LISTS up to each tile's
clamped count.  The CPU side is tests/test_local_ref.py.
"""
import functools

import numpy as np
import pytest

import local_scenes as S
from test_gpu_parity import first_diff, to_dev

# name: (gaussians, width, height, SH components, precision (1 = f16), colour space, seed, gen_scene kw)
CASES = {
    "sh0_f32_64x48": (1000, 64, 48, 1, 0, 0, 31, {}),
    "sh1_f16_100x70": (2000, 100, 70, 4, 1, 0, 32, {}),
    "sh2_f32_100x70_srgb": (5000, 100, 70, 9, 0, 1, 33, {"scale_px": 2.0}),
    "sh3_f16_320x180": (20000, 320, 180, 16, 1, 0, 34, {}),
    "sh0_f16_320x180_large_splats": (3000, 320, 180, 1, 1, 0, 35, {"scale_px": 6.0}),
}


@functools.lru_cache(maxsize=None)
def _case_ref(name):
    """(world, harm, reference frame) of one CASES shape: computed once, shared, never modified."""
    import local_ref
    n, w, h, sh, prec, cs, seed, kw = CASES[name]
    world, harm = S.scene(n, w, h, sh, prec, seed, **kw)
    r = local_ref.render(world, harm, sh, S.cam(w, h), w, h, color_space=cs)
    assert r["status"] == 0 and r["overflow"] == 0
    return world, harm, r


def gpu_local(gsm, torch, world, harm, sh, cam, w, h, max_gaussians=None, max_width=None, max_height=None,
              color_space=0, color_format=0, renderer=None, with_depth=True, pad=0):
    """One frame; `pad` extra columns in both targets (row pitch wider than the frame)."""
    prec = 1 if world.dtype.itemsize == 32 else 0
    n = len(world)
    if renderer is None:
        cfg = gsm.RendererConfig(max_gaussians=max_gaussians or max(n, 1), max_width=max_width or w,
                                 max_height=max_height or h, precision=prec, gaussian_color_space=color_space,
                                 color_format=color_format)
        renderer = gsm.LocalRenderer(config=cfg)
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
    B = gsm.LocalBuffer
    out = {"counters": renderer.counters(), "stage_ms": renderer.stage_times_ms(), "renderer": renderer}
    c = color.cpu().numpy()
    out["color_full"] = c.view(np.uint16) if dt == torch.float16 else c
    out["depth_full"] = depth.cpu().numpy().view(np.uint16)
    out["color"] = out["color_full"][:, :w]
    out["depth"] = out["depth_full"][:, :w]
    out["projected"] = renderer.copy_buffer(B.PROJECTED)
    out["tile_counts"] = renderer.copy_buffer(B.TILE_COUNTS)
    out["tile_lists"] = renderer.copy_buffer(B.TILE_LISTS)
    return out


def assert_local_equal(g, r, color=True, depth=True, lists=True):
    """lists=False for an overflowing frame: which 2048 entries such a tile keeps is unspecified."""
    c = g["counters"]
    for k in ("visible", "tiles_x", "tiles_y", "tile_count", "active_tiles", "total_entries", "max_tile_count",
              "max_per_tile", "overflow"):
        assert c[k] == r[k], (k, c[k], r[k])
    assert c["gaussian_count"] == r["count"]
    gp = g["projected"].view(np.uint8).reshape(-1, 32)
    rp = r["projected"].view(np.uint8).reshape(-1, 32)
    assert gp.shape == rp.shape
    if not np.array_equal(gp, rp):
        bad = np.nonzero((gp != rp).any(1))[0][:3]
        raise AssertionError(f"PROJECTED differs at rows {bad}: {g['projected'][bad]} vs {r['projected'][bad]}")
    np.testing.assert_array_equal(g["tile_counts"], r["tile_counts"])
    assert g["tile_lists"].shape == r["tile_lists"].shape
    for t, cnt in enumerate(np.minimum(r["tile_counts"], S.MAX_PER_TILE).tolist()):
        if lists or r["tile_counts"][t] <= S.MAX_PER_TILE:
            np.testing.assert_array_equal(g["tile_lists"][t, :cnt], r["tile_lists"][t, :cnt], err_msg=f"tile {t}")
    if color:
        assert np.array_equal(g["color"], r["color"]), first_diff(g["color"], r["color"])
    if depth:
        assert np.array_equal(g["depth"], r["depth"]), first_diff(g["depth"], r["depth"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_local_bit_exact(gsm, cuda, oracle, name):
    n, w, h, sh, prec, cs, seed, kw = CASES[name]
    world, harm, r = _case_ref(name)
    g = gpu_local(gsm, cuda, world, harm, sh, S.cam(w, h), w, h, color_space=cs)
    assert_local_equal(g, r)
    assert set(g["stage_ms"]) == set(gsm.LOCAL_STAGES) and g["renderer"].last_gpu_time is not None
    g["renderer"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,w,h,sh,seed", [("f16", 2500, 100, 70, 9, 21), ("f32", 2500, 64, 48, 1, 22)])
def test_local_adversarial_scenes_bit_exact(gsm, cuda, oracle, kind, n, w, h, sh, seed):
    """tests/adversarial.py scenes (zero / extreme / inf / NaN scales, positions and quaternions,
    opacities around the cull, huge / NaN SH) through the Local frame."""
    import adversarial
    import local_ref
    case = adversarial.scene(kind, n, w, h, sh, seed)
    r = local_ref.render(case["world"], case["harm"], sh, S.cam(w, h), w, h)
    assert r["status"] == 0 and r["overflow"] == 0 and r["visible"] > 500
    g = gpu_local(gsm, cuda, case["world"], case["harm"], sh, S.cam(w, h), w, h)
    assert_local_equal(g, r)
    g["renderer"].close()


@pytest.mark.gpu
def test_local_depth_ties(gsm, cuda, oracle):
    """A plane of gaussians at one view depth: every list is one tie run, ordered by the compacted index
    whatever slots the atomics handed out."""
    import local_ref
    w, h = 100, 70
    world, harm = S.plane(3000, w, h, 17)
    r = local_ref.render(world, harm, 1, S.cam(w, h), w, h)
    assert len(np.unique(r["projected"]["depth"])) == 1 and r["tile_counts"].max() > 64 and r["overflow"] == 0
    g = gpu_local(gsm, cuda, world, harm, 1, S.cam(w, h), w, h)
    assert_local_equal(g, r)
    g["renderer"].close()


@pytest.mark.gpu
def test_local_overflow(gsm, cuda, oracle):
    """2 500 identical gaussians in one tile: overflow = 1, the count 2 500, and -- any kept subset of
    identical copies giving the same pixels -- the frame bit for bit."""
    import local_ref
    w = h = 64
    world, harm = S.stack(2500, w, h, others=300)
    r = local_ref.render(world, harm, 1, S.cam(w, h), w, h)
    assert r["overflow"] == 1 and r["max_tile_count"] == 2500 and r["walked"][5] == S.MAX_PER_TILE
    g = gpu_local(gsm, cuda, world, harm, 1, S.cam(w, h), w, h)
    assert_local_equal(g, r, lists=False)
    kept = g["tile_lists"][5]  # some 2048 distinct copies, ascending (equal depth16: index order)
    assert np.all(np.diff(kept.astype(np.int64)) > 0) and kept.max() < 2500
    g["renderer"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 2047, 2048])
def test_local_sort_padding_edges(gsm, cuda, oracle, k):
    import local_ref
    w = h = 64
    world, harm = S.stack(k, w, h)
    r = local_ref.render(world, harm, 1, S.cam(w, h), w, h)
    assert r["tile_counts"][5] == k and r["overflow"] == 0
    g = gpu_local(gsm, cuda, world, harm, 1, S.cam(w, h), w, h)
    assert_local_equal(g, r)
    g["renderer"].close()


@pytest.mark.gpu
def test_local_nonfinite_colour(gsm, cuda, oracle):
    """half(colour) = inf on a gaussian that partly covers a tile: the 4x2 groups with eight zero alphas
    skip it and stay finite, the others turn NaN (inf * 0), exactly as the reference's grouping does."""
    import local_ref
    w = h = 64
    world, harm = S.nonfinite_colour(w, h)
    r = local_ref.render(world, harm, 1, S.cam(w, h), w, h)
    tile = r["color"][16:32, 16:32, :3].view(np.float16)
    assert np.isnan(tile).any() and np.isfinite(tile).any()
    g = gpu_local(gsm, cuda, world, harm, 1, S.cam(w, h), w, h)
    assert_local_equal(g, r)
    g["renderer"].close()


@pytest.mark.gpu
def test_local_null_depth_target(gsm, cuda, oracle):
    name = "sh1_f16_100x70"
    n, w, h, sh, prec, cs, seed, kw = CASES[name]
    world, harm, r = _case_ref(name)
    g = gpu_local(gsm, cuda, world, harm, sh, S.cam(w, h), w, h, color_space=cs, with_depth=False)
    assert_local_equal(g, r, depth=False)
    assert np.all(g["depth_full"] == 0x7E00)  # the NaN fill, untouched
    g["renderer"].close()


@pytest.mark.gpu
def test_local_inside_larger_configuration_with_wide_pitch(gsm, cuda, oracle):
    """100x70 inside a 512x256 configuration, rows 37 pixels wider than the frame: bytes outside the
    frame stay untouched."""
    name = "sh1_f16_100x70"
    n, w, h, sh, prec, cs, seed, kw = CASES[name]
    world, harm, r = _case_ref(name)
    g = gpu_local(gsm, cuda, world, harm, sh, S.cam(w, h), w, h, color_space=cs, max_gaussians=3 * n, max_width=512,
                  max_height=256, pad=37)
    assert_local_equal(g, r)
    assert np.all(g["color_full"][:, w:] == 0x7E00) and np.all(g["depth_full"][:, w:] == 0x7E00)
    g["renderer"].close()


@pytest.mark.gpu
def test_local_color_format_bgra8_srgb(gsm, cuda, oracle):
    name = "sh0_f32_64x48"
    n, w, h, sh, prec, cs, seed, kw = CASES[name]
    world, harm, r = _case_ref(name)
    fmt = int(gsm.ColorFormat.BGRA8_UNORM_SRGB)
    g = gpu_local(gsm, cuda, world, harm, sh, S.cam(w, h), w, h, color_space=cs, color_format=fmt)
    assert_local_equal(g, r, color=False)
    np.testing.assert_array_equal(g["color"], oracle.convert_color(r["color"], fmt))
    g["renderer"].close()


@pytest.mark.gpu
def test_local_two_frames_on_one_handle(gsm, cuda, oracle):
    """A frame, then a smaller one with fewer gaussians on the same handle: no counts or lists are left
    over from the first."""
    import local_ref
    name = "sh0_f16_320x180_large_splats"
    n, w, h, sh, prec, cs, seed, kw = CASES[name]
    world, harm, r = _case_ref(name)
    g1 = gpu_local(gsm, cuda, world, harm, sh, S.cam(w, h), w, h)
    assert_local_equal(g1, r)
    rend = g1["renderer"]
    n2, w2, h2 = 700, 100, 70
    world2, harm2 = S.scene(n2, w2, h2, sh, prec, 77)
    r2 = local_ref.render(world2, harm2, sh, S.cam(w2, h2), w2, h2)
    g2 = gpu_local(gsm, cuda, world2, harm2, sh, S.cam(w2, h2), w2, h2, renderer=rend)
    assert_local_equal(g2, r2)
    rend.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["full", "variable"])
def test_local_sort_tiles_kats(gsm, cuda, oracle, which):
    """gsm_local_debug_sort_tiles on the inputs of LocalUnitTests.swift:122-235."""
    keys, idx, counts, mpt = S.kat_inputs(which)
    dk = cuda.from_numpy(keys.view(np.int16).copy()).cuda()
    di = cuda.from_numpy(idx.view(np.int32).copy()).cuda()
    dc = cuda.from_numpy(counts.view(np.int32).copy()).cuda()
    out = cuda.zeros(len(keys), dtype=cuda.int16, device="cuda")
    gsm.LocalRenderer.sort_tiles(dk, di, dc, mpt, out)
    cuda.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint16), S.kat_expected(keys, counts, mpt))
    with pytest.raises(gsm.RendererError) as e:
        gsm.LocalRenderer.sort_tiles(dk, di, dc, 4096, out)
    assert e.value.status == gsm.Status.INVALID_ARGUMENT


@pytest.mark.gpu
def test_local_errors(gsm, cuda):
    w, h = 64, 48
    rend = gsm.LocalRenderer(config=gsm.RendererConfig(max_gaussians=16, max_width=w, max_height=h))
    x = cuda.zeros(w * h * 8, dtype=cuda.uint8, device="cuda")
    cam = gsm.CameraParams.from_dict(S.cam(w, h))
    for count, ww, col, pitch, status in ((0, w, x, None, gsm.Status.INVALID_GAUSSIAN_COUNT),
                                          (17, w, x, None, gsm.Status.INVALID_GAUSSIAN_COUNT),
                                          (1, w + 1, x, None, gsm.Status.INVALID_DIMENSIONS),
                                          (1, 0, x, None, gsm.Status.INVALID_DIMENSIONS),
                                          (1, w, None, None, gsm.Status.MISSING_REQUIRED_BUFFER),
                                          (1, w, x, w * 8 - 4, gsm.Status.INVALID_BUFFER_SIZE),
                                          (1, w, x, w * 8 + 2, gsm.Status.INVALID_BUFFER_SIZE)):
        with pytest.raises(gsm.RendererError) as e:
            rend.render(col, None, gsm.GaussianInput(x, x, count, 1), cam, ww, h, color_pitch=pitch)
        assert e.value.status == status
    with pytest.raises(gsm.RendererError) as e:
        rend.render(x, None, gsm.GaussianInput(None, x, 1, 1), cam, w, h)
    assert e.value.status == gsm.Status.MISSING_REQUIRED_BUFFER
    rend.close()
    for cfg, status in ((gsm.RendererConfig(max_gaussians=30_000_001, max_width=w, max_height=h),
                         gsm.Status.INVALID_GAUSSIAN_COUNT),
                        (gsm.RendererConfig(max_gaussians=16, max_width=16 * 300, max_height=16 * 300),
                         gsm.Status.INVALID_TILE_COUNT)):
        with pytest.raises(gsm.RendererError) as e:
            gsm.LocalRenderer(config=cfg)
        assert e.value.status == status
