"""gsm_global_render_views: several views of one scene in one Global frame.  The contract
is that every view's bytes -- colour and depth -- equal those of gsm_global_render for its camera; the
yardsticks are `render` on a second handle and the oracle for the same camera.  Shapes are the smallest
that reach each code path (the rules that pick kernels take the batch's tile count)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

ERR_COUNT, ERR_DIMS, ERR_SIZE, ERR_TILES, ERR_MISSING, ERR_UNSUPPORTED = 6, 7, 8, 9, 13, 15
BPP = {0: 8, 1: 16, 2: 4, 3: 4, 4: 4, 5: 4}


# ---- 1. declaration and export (no GPU) ----
def test_views_entry_is_declared_exported_and_bound(gsm):
    src = open(os.path.join(ROOT, "include", "gsm_renderer.h")).read()
    assert re.search(r"gsm_status\s+gsm_global_render_views\s*\(", src)
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    assert " T gsm_global_render_views" in out
    assert "gsm_global_render_views" in gsm._SIGNATURES
    assert callable(getattr(gsm.GlobalRenderer, "render_views", None))


# ---- helpers ----
def to_dev(torch, arr):
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def away_camera(scenes, w, h):
    """make_camera turned half a turn about the y axis: every gaussian of the scenes is behind it."""
    cam = scenes.make_camera(w, h)
    V = np.eye(4, dtype=np.float32)
    V[0, 0] = V[2, 2] = -1.0
    cam["view"] = V.T.reshape(-1).astype(np.float32)
    return cam


def orbit(scenes, w, h, angles):
    return [scenes.orbit_camera(w, h, a) for a in angles]


def pad16(h):
    return (h + 15) // 16 * 16


def roundup256(n):
    return (n + 255) // 256 * 256


class Scene:
    def __init__(self, torch, world, harm, sh, n=None):
        self.world_np, self.harm_np, self.sh = world, harm, sh
        self.n = len(world) if n is None else n
        self.prec = 1 if world.dtype.itemsize == 32 else 0
        self.world, self.harm = to_dev(torch, world), to_dev(torch, harm)

    def input(self, gsm):
        return gsm.GaussianInput(self.world, self.harm, self.n, self.sh)


def batch_handle(gsm, sc, k, w, h, fmt=0, max_gaussians=None, color_space=0):
    """A handle whose tile space holds exactly k frames of w x h and whose item space holds k views."""
    mg = max(k * roundup256(sc.n), 1) if max_gaussians is None else max_gaussians
    return gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=mg, max_width=w, max_height=k * pad16(h),
                                                        precision=sc.prec, color_format=fmt,
                                                        gaussian_color_space=color_space))


def single_handle(gsm, sc, w, h, fmt=0, max_gaussians=None, color_space=0):
    mg = max(sc.n, 1) if max_gaussians is None else max_gaussians
    return gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=mg, max_width=w, max_height=h,
                                                        precision=sc.prec, color_format=fmt,
                                                        gaussian_color_space=color_space))


def targets(torch, k, w, h, bpp=8, extra_rows=0, fill=0xA5):
    """k colour and depth targets, each followed by extra_rows sentinel rows, filled with `fill` bytes."""
    color = torch.full((k, h + extra_rows, w * bpp), fill, dtype=torch.uint8, device="cuda")
    depth = torch.full((k, h + extra_rows, w * 2), fill, dtype=torch.uint8, device="cuda")
    return color, depth


def render_batch(gsm, torch, r, sc, cams, w, h, bpp=8, extra_rows=0, depth=True):
    k = len(cams)
    color, dep = targets(torch, k, w, h, bpp, extra_rows)
    r.render_views(color, dep if depth else None, sc.input(gsm), [gsm.CameraParams.from_dict(c) for c in cams], w, h,
                   color_view_stride=(h + extra_rows) * w * bpp, depth_view_stride=(h + extra_rows) * w * 2)
    torch.cuda.synchronize()
    return color.cpu().numpy(), dep.cpu().numpy()


def render_single(gsm, torch, r, sc, cam, w, h, bpp=8):
    color, dep = targets(torch, 1, w, h, bpp)
    r.render(color, dep, sc.input(gsm), gsm.CameraParams.from_dict(cam), w, h)
    torch.cuda.synchronize()
    return color.cpu().numpy()[0], dep.cpu().numpy()[0], r.debug_read_total_assignments()


def diff(a, b):
    idx = np.nonzero(np.asarray(a).reshape(-1) != np.asarray(b).reshape(-1))[0]
    return f"{idx.size} bytes differ, first at {idx[:4].tolist()}"


def check_batch(gsm, torch, oracle, sc, cams, w, h, batch=None, single=None, oracle_views=None, max_gaussians=None,
                color_space=0):
    """Render the batch and every view alone; each view must equal its own frame (and the oracle's, for
    oracle_views -- all by default).  Returns (batch handle's total, sum of the single totals)."""
    k = len(cams)
    rb = batch or batch_handle(gsm, sc, k, w, h, max_gaussians=None if max_gaussians is None else k * max_gaussians,
                               color_space=color_space)
    rs = single or single_handle(gsm, sc, w, h, max_gaussians=max_gaussians, color_space=color_space)
    bc, bd = render_batch(gsm, torch, rb, sc, cams, w, h)
    total = rb.debug_read_total_assignments()
    assert rb.counters()["overflow"] == 0
    singles = 0
    for v, cam in enumerate(cams):
        c, d, t = render_single(gsm, torch, rs, sc, cam, w, h)
        singles += t
        assert rs.counters()["overflow"] == 0, "the yardstick frame overflowed: no parity to check"
        assert np.array_equal(bc[v], c), f"view {v} colour vs render: " + diff(bc[v], c)
        assert np.array_equal(bd[v], d), f"view {v} depth vs render: " + diff(bd[v], d)
        if oracle_views is None or v in oracle_views:
            ref = oracle.render(sc.world_np, sc.harm_np, sc.sh, cam, w, h,
                                max_gaussians=max_gaussians or max(sc.n, 1), color_space=color_space, count=sc.n)
            oc, od = ref["color"].view(np.uint8).reshape(h, -1), ref["depth"].view(np.uint8).reshape(h, -1)
            assert np.array_equal(bc[v], oc), f"view {v} colour vs oracle: " + diff(bc[v], oc)
            assert np.array_equal(bd[v], od), f"view {v} depth vs oracle: " + diff(bd[v], od)
            assert t == ref["total_assignments"]
    if batch is None:
        rb.close()
    if single is None:
        rs.close()
    return total, singles


def clear_bytes(h, w):
    """the clear value: colour (0, 0, 0, 1) in fp16, depth 0"""
    c = np.zeros((h, w, 4), np.uint16)
    c[..., 3] = 0x3C00
    return c.view(np.uint8).reshape(h, -1), np.zeros((h, w * 2), np.uint8)


# ---- 2. ragged frame ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_ragged_frame_three_views(gsm, cuda, oracle, prec):
    """2 000 gaussians (not a multiple of 256: a view's items are padded to whole blocks), SH degree 1,
    97 x 45; the batch's assignment total is the sum of the three frames'."""
    from gsm_amd import scenes
    w, h = 97, 45
    world, harm, _ = scenes.gen_scene(2000, w, h, 4, prec, seed=5)
    sc = Scene(cuda, world, harm, 4)
    total, singles = check_batch(gsm, cuda, oracle, sc, orbit(scenes, w, h, (0.0, 9.0, -14.0)), w, h)
    assert total == singles and total > 0


# ---- 3. one view, and sentinels between views ----
@pytest.mark.gpu
def test_one_view_equals_render_and_strides_leave_gaps_untouched(gsm, cuda, oracle):
    from gsm_amd import scenes
    w, h = 97, 45
    world, harm, cam = scenes.gen_scene(2000, w, h, 1, 0, seed=6)
    sc = Scene(cuda, world, harm, 1)
    check_batch(gsm, cuda, oracle, sc, [cam], w, h)
    cams = orbit(scenes, w, h, (0.0, 6.0))
    rb, rs = batch_handle(gsm, sc, 2, w, h), single_handle(gsm, sc, w, h)
    for k_cams in ([cam], cams):  # view strides larger than the image: 3 sentinel rows after every view
        bc, bd = render_batch(gsm, cuda, rb, sc, k_cams, w, h, extra_rows=3)
        for v, c in enumerate(k_cams):
            sc_c, sc_d, _ = render_single(gsm, cuda, rs, sc, c, w, h)
            assert np.array_equal(bc[v, :h], sc_c) and np.array_equal(bd[v, :h], sc_d)
            assert (bc[v, h:] == 0xA5).all() and (bd[v, h:] == 0xA5).all(), "sentinel rows were written"
    rb.close()
    rs.close()


# ---- 4. views with no work ----
@pytest.mark.gpu
def test_views_without_work_hold_the_clear_value(gsm, cuda, oracle):
    from gsm_amd import scenes
    w, h = 97, 45
    world, harm, cam = scenes.gen_scene(2000, w, h, 1, 0, seed=7)
    sc = Scene(cuda, world, harm, 1)
    away = away_camera(scenes, w, h)
    assert oracle.render(world, harm, 1, away, w, h, max_gaussians=2000)["total_assignments"] == 0
    cams = [cam, scenes.orbit_camera(w, h, 8.0), away, scenes.orbit_camera(w, h, -5.0)]
    rb = batch_handle(gsm, sc, 4, w, h)
    check_batch(gsm, cuda, oracle, sc, cams, w, h, batch=rb)
    bc, bd = render_batch(gsm, cuda, rb, sc, cams, w, h)
    cc, cd = clear_bytes(h, w)
    assert np.array_equal(bc[2], cc) and np.array_equal(bd[2], cd)
    bc, bd = render_batch(gsm, cuda, rb, sc, [away] * 4, w, h)  # every view empty
    assert rb.debug_read_total_assignments() == 0
    for v in range(4):
        assert np.array_equal(bc[v], cc) and np.array_equal(bd[v], cd)
    rb.close()


# ---- 5. both sides of the rules that pick kernels ----
@pytest.mark.gpu
def test_small_batch_one_pass_sort_and_quadrant_units(gsm, cuda, oracle):
    """2 x 12 tiles: a tile field of <= 8 bits (one narrow pass) and quadrant units."""
    from gsm_amd import scenes
    w, h = 97, 45
    world, harm, _ = scenes.gen_scene(3000, w, h, 1, 0, seed=8)
    sc = Scene(cuda, world, harm, 1)
    rb = batch_handle(gsm, sc, 2, w, h)
    check_batch(gsm, cuda, oracle, sc, orbit(scenes, w, h, (0.0, 12.0)), w, h, batch=rb)
    assert rb.blend_kernel_kind() == 1
    rb.close()


@pytest.mark.gpu
def test_batch_crossing_into_two_passes_and_half_tile_units(gsm, cuda, oracle):
    """5 x 460 = 2300 tiles: past the one wide pass (2048 tiles) and past the quadrant units (8 tiles per CU)."""
    from gsm_amd import scenes
    w, h = 640, 360
    world, harm, _ = scenes.gen_scene(20_000, w, h, 1, 0, seed=9)
    sc = Scene(cuda, world, harm, 1)
    rb = batch_handle(gsm, sc, 5, w, h)
    check_batch(gsm, cuda, oracle, sc, orbit(scenes, w, h, (0.0, 5.0, 10.0, -5.0, -10.0)), w, h, batch=rb,
                oracle_views=(0, 4))
    assert rb.blend_kernel_kind() == 2
    rb.close()


@pytest.mark.gpu
def test_batch_reaching_the_pair_walk(gsm, cuda, oracle):
    """27 x 460 = 12 420 tiles, 24 840 half-tile units >= 6 per wave slot of 256 CUs: 16 waves per workgroup
    and the pair walk (k_blend_pw_views).  Every view against `render`, the first and the last against the
    oracle."""
    from gsm_amd import scenes
    w, h, k = 640, 360, 27
    world, harm, _ = scenes.gen_scene(20_000, w, h, 1, 0, seed=10)
    sc = Scene(cuda, world, harm, 1)
    rb = batch_handle(gsm, sc, k, w, h)
    check_batch(gsm, cuda, oracle, sc, orbit(scenes, w, h, [2.0 * (i - 13) for i in range(k)]), w, h, batch=rb,
                oracle_views=(0, k - 1))
    assert rb.blend_kernel_kind() == 3, "the batch did not reach the pair walk"
    rb.close()


# ---- 6. exact re-walk ----
def far_scene():
    """test_far_gaussian_fp16_depth_overflow's scene (tests/test_gpu_parity.py): gaussian 1 has fp16 depth inf."""
    from gsm_amd.types import WORLD32
    w = np.zeros(3, WORLD32)
    w["rot"][:, 3] = 1.0
    w[0]["px"], w[0]["py"], w[0]["pz"], w[0]["opacity"] = 0.1, 0.05, 3.0, 0.6
    w[0]["sx"], w[0]["sy"], w[0]["sz"] = 0.05, 0.04, 0.05
    w[1]["px"], w[1]["py"], w[1]["pz"], w[1]["opacity"] = 0.0, 0.0, 80000.0, 0.9
    w[1]["sx"], w[1]["sy"], w[1]["sz"] = 3000.0, 2500.0, 3000.0
    w[2]["px"], w[2]["py"], w[2]["pz"], w[2]["opacity"] = -0.2, 0.1, 4.0, 0.3
    w[2]["sx"], w[2]["sy"], w[2]["sz"] = 0.5, 0.3, 0.2
    return w, np.tile(np.array([0.3, -0.2, 0.8], np.float32), 3)


@pytest.mark.gpu
def test_far_gaussian_visible_in_one_view_only(gsm, cuda, oracle):
    from gsm_amd import scenes
    w, h = 640, 360
    world, harm = far_scene()
    cams = [scenes.orbit_camera(w, h, 60.0), scenes.make_camera(w, h), scenes.orbit_camera(w, h, -60.0)]
    vis = [int(oracle.render(world, harm, 1, c, w, h, max_gaussians=3)["mask"][1]) for c in cams]
    assert vis == [0, 1, 0], "the far gaussian must be visible in view 1 only"
    # (room for every assignment: the far gaussian covers all 460 tiles, and a frame over its capacity has no parity)
    check_batch(gsm, cuda, oracle, Scene(cuda, world, harm, 1), cams, w, h, max_gaussians=1024)


# ---- 7. adversarial inputs ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_adversarial_inputs_three_views(gsm, cuda, oracle, kind):
    import adversarial
    from gsm_amd import scenes
    w, h = 160, 90
    case = adversarial.scene(kind, 4000, w, h, 4, seed=21)
    sc = Scene(cuda, case["world"], case["harm"], 4)
    total, singles = check_batch(gsm, cuda, oracle, sc, orbit(scenes, w, h, (0.0, 10.0, -10.0)), w, h,
                                 max_gaussians=case["max_gaussians"])
    assert total == singles


# ---- 8. create-time switches ----
@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"GSM_SORT_RANK": "ballot"}, {"GSM_SORT_WIDE": "0"}, {"GSM_BLEND_SCHED": "0"}])
def test_create_time_switches_same_bytes(gsm, cuda, oracle, monkeypatch, env):
    """3 x 120 tiles (a 9-bit tile field: GSM_SORT_WIDE picks one wide or two narrow passes)."""
    from gsm_amd import scenes
    w, h = 320, 180
    world, harm, _ = scenes.gen_scene(6000, w, h, 1, 0, seed=11)
    sc = Scene(cuda, world, harm, 1)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rb = batch_handle(gsm, sc, 3, w, h)
    for k in env:
        monkeypatch.delenv(k)
    check_batch(gsm, cuda, oracle, sc, orbit(scenes, w, h, (0.0, 7.0, -7.0)), w, h, batch=rb)
    check_batch(gsm, cuda, oracle, sc, orbit(scenes, w, h, (1.0, 8.0, -6.0)), w, h, batch=rb, oracle_views=())
    rb.close()


# ---- 9. handle reuse ----
@pytest.mark.gpu
def test_handle_reuse_between_frames_and_batches(gsm, cuda, oracle):
    """render, render_views, render of another size, render_views with another K on one handle."""
    from gsm_amd import scenes
    world, harm, _ = scenes.gen_scene(5000, 320, 180, 1, 0, seed=12)
    sc = Scene(cuda, world, harm, 1)
    r = gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=4 * roundup256(sc.n), max_width=320,
                                                     max_height=4 * 192, precision=0, gaussian_color_space=0))
    a = render_single(gsm, cuda, r, sc, scenes.make_camera(320, 180), 320, 180)
    check_batch(gsm, cuda, oracle, sc, orbit(scenes, 320, 180, (0.0, 7.0, -7.0)), 320, 180, batch=r, oracle_views=(1,))
    b = render_single(gsm, cuda, r, sc, scenes.make_camera(200, 100), 200, 100)
    check_batch(gsm, cuda, oracle, sc, orbit(scenes, 200, 100, (3.0, -3.0, 6.0, -6.0)), 200, 100, batch=r,
                oracle_views=(2,))
    check_batch(gsm, cuda, oracle, sc, orbit(scenes, 320, 180, (4.0, -4.0)), 320, 180, batch=r, oracle_views=())
    r.close()
    for got, (w, h) in ((a, (320, 180)), (b, (200, 100))):
        fresh = gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=4 * roundup256(sc.n), max_width=320,
                                                             max_height=4 * 192, precision=0,
                                                             gaussian_color_space=0))
        want = render_single(gsm, cuda, fresh, sc, scenes.make_camera(w, h), w, h)
        fresh.close()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


# ---- 10. errors ----
@pytest.mark.gpu
def test_errors_before_enqueue_in_precedence(gsm, cuda):
    from gsm_amd import scenes
    torch = cuda
    w, h, n = 96, 48, 1000  # 3 x 3 = 9 tiles; 1024 items per view
    world, harm, cam = scenes.gen_scene(n, w, h, 1, 0, seed=13)
    sc = Scene(torch, world, harm, 1)
    cp = gsm.CameraParams.from_dict(cam)
    r = gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=3 * 1024, max_width=w, max_height=3 * h,
                                                     precision=0))  # 27 tiles, 3 views of 1024 items
    color, depth = targets(torch, 4, w, h)

    def status(cams, width=w, height=h, color=color, depth=depth, count=n, **kw):
        inp = gsm.GaussianInput(sc.world, sc.harm, count, 1)
        try:
            r.render_views(color, depth, inp, cams, width, height, **kw)
        except gsm.RendererError as e:
            return e.status
        return 0

    before = color.clone()
    assert status([cp] * 3) == 0                       # every bound at its limit
    torch.cuda.synchronize()
    color.copy_(before)
    assert status([cp] * 4) == ERR_COUNT               # one view past the item space (and the tile space)
    assert status([cp] * 3, count=1025) == ERR_COUNT   # 3 x 1280 items > 3072
    assert status([]) == ERR_COUNT                     # K = 0
    assert status([cp], width=w + 1) == ERR_DIMS
    assert status([cp], height=3 * h + 1) == ERR_DIMS
    assert status([cp] * 4, width=w + 1) == ERR_COUNT  # count before dimensions
    assert status([cp] * 2, height=2 * h) == ERR_TILES           # 2 x 18 tiles > 27 (items fit: 2048)
    assert status([cp] * 3, width=w + 1, height=2 * h) == ERR_DIMS  # dimensions before tiles
    assert status([cp], height=3 * h) == 0                       # 27 tiles: at the limit
    torch.cuda.synchronize()
    color.copy_(before)
    assert status(None) == ERR_MISSING                           # NULL cameras
    assert status([cp] * 2, color=None) == ERR_MISSING
    assert status([cp] * 2, height=2 * h, color=None) == ERR_TILES  # tiles before a missing buffer
    assert status([cp] * 2, color=None, color_pitch=4) == ERR_MISSING  # a missing buffer before sizes
    assert status([cp] * 2, color_pitch=w * 8 - 4) == ERR_SIZE
    assert status([cp] * 2, color_view_stride=h * w * 8 - 8) == ERR_SIZE  # a stride shorter than a view's rows
    assert status([cp] * 2, depth_view_stride=h * w * 2 - 2) == ERR_SIZE
    assert status([cp] * 2, color_view_stride=h * w * 8) == 0
    torch.cuda.synchronize()
    color.copy_(before)
    r.set_tile_rows(0, 2)
    assert status([cp] * 2) == ERR_UNSUPPORTED
    r.set_tile_rows(0, 0)
    assert status([cp] * 2) == 0
    torch.cuda.synchronize()
    color.copy_(before)
    for bad in ([cp] * 4, []):  # a refused call enqueues nothing: the targets keep their bytes
        status(bad)
    torch.cuda.synchronize()
    assert torch.equal(color, before)
    r.close()
    # the 65535-tile bound: a handle of 65536 tiles (the largest gsm_global_create allows)
    big = gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=256, max_width=32 * 256, max_height=16 * 256,
                                                       precision=0))
    inp = gsm.GaussianInput(sc.world, sc.harm, 0, 1)
    with pytest.raises(gsm.RendererError) as e:
        big.render_views(color, None, inp, [cp], 32 * 256, 16 * 256)  # 65536 tiles
    assert e.value.status == ERR_TILES
    big.close()


# ---- 11. colour formats ----
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 4, 5])
def test_colour_formats_two_views(gsm, cuda, fmt):
    from gsm_amd import scenes
    w, h = 97, 45
    world, harm, _ = scenes.gen_scene(2000, w, h, 1, 1, seed=14)
    sc = Scene(cuda, world, harm, 1)
    cams = orbit(scenes, w, h, (0.0, 9.0))
    rb, rs = batch_handle(gsm, sc, 2, w, h, fmt=fmt), single_handle(gsm, sc, w, h, fmt=fmt)
    bc, bd = render_batch(gsm, cuda, rb, sc, cams, w, h, bpp=BPP[fmt])
    for v, cam in enumerate(cams):
        c, d, _ = render_single(gsm, cuda, rs, sc, cam, w, h, bpp=BPP[fmt])
        assert np.array_equal(bc[v], c), f"view {v} colour: " + diff(bc[v], c)
        assert np.array_equal(bd[v], d), f"view {v} depth: " + diff(bd[v], d)
    rb.close()
    rs.close()


# ---- 12. the entry beside the batch ----
FW, FH, FN = 96, 48, 1000  # 3 x 3 = 9 tiles, 1024 items per view


def front_scene(cuda):
    from gsm_amd import scenes
    world, harm, _ = scenes.gen_scene(FN, FW, FH, 1, 0, seed=15)
    return Scene(cuda, world, harm, 1)


def strided_targets(torch, k, cs, ds):
    return (torch.full((k * cs,), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((k * ds,), 0xA5, dtype=torch.uint8, device="cuda"))


def view_bytes(buf, v, stride, rows, pitch):
    return buf[v * stride: v * stride + rows * pitch].reshape(rows, pitch)


def check_strided(buf, stride, pitch, want, what):
    """Every view's rows equal its single frame; every byte between and after the views is still 0xA5."""
    buf = buf.cpu().numpy()
    for v, w in enumerate(want):
        got = view_bytes(buf, v, stride, FH, pitch)
        assert np.array_equal(got, w), f"view {v} {what}: " + diff(got, w)
        assert (buf[v * stride + FH * pitch: (v + 1) * stride] == 0xA5).all(), f"{what} gap after view {v} written"


@pytest.mark.gpu
@pytest.mark.parametrize("with_depth", [True, False])
def test_view_strides_that_misalign_later_views(gsm, cuda, with_depth):
    """Three views whose strides leave view 1's colour target 8 bytes off a 16-byte boundary and views 1 and 2's
    depth targets 2 and 4 bytes off an 8-byte one: the wide stores must not be taken where a view's target is
    not aligned for them, and the bytes are the single frame's whichever stores are taken."""
    from gsm_amd import scenes
    torch = cuda
    sc = front_scene(torch)
    cams = orbit(scenes, FW, FH, (0.0, 8.0, -8.0))
    cp, dp = FW * 8, FW * 2
    cs, ds = FH * cp + 8, FH * dp + 2
    rb, rs = batch_handle(gsm, sc, 3, FW, FH), single_handle(gsm, sc, FW, FH)
    color, depth = strided_targets(torch, 3, cs, ds)
    rb.render_views(color, depth if with_depth else None, sc.input(gsm), [gsm.CameraParams.from_dict(c) for c in cams],
                    FW, FH, color_view_stride=cs, depth_view_stride=ds)
    torch.cuda.synchronize()
    singles = [render_single(gsm, torch, rs, sc, c, FW, FH) for c in cams]
    check_strided(color, cs, cp, [s[0] for s in singles], "colour")
    if with_depth:
        check_strided(depth, ds, dp, [s[1] for s in singles], "depth")
    else:
        assert (depth == 0xA5).all(), "a batch without a depth target wrote depth"
    rb.close()
    rs.close()


@pytest.mark.gpu
def test_views_and_batch_share_a_schedule_harmlessly(gsm, cuda):
    """render_views, render_batch of the same three views, render_views with other cameras, then one single
    frame, all on one handle: whatever walk costs a frame finds, the order never changes an image."""
    from gsm_amd import scenes
    torch = cuda
    sc = front_scene(torch)
    cams_a = orbit(scenes, FW, FH, (0.0, 8.0, -8.0))
    cams_b = orbit(scenes, FW, FH, (3.0, -11.0, 5.0))
    cp, dp = FW * 8, FW * 2
    cs, ds = FH * cp + 16, FH * dp + 8
    r, rs = batch_handle(gsm, sc, 3, FW, FH), single_handle(gsm, sc, FW, FH)
    want = {id(c): render_single(gsm, torch, rs, sc, c, FW, FH) for c in cams_a + cams_b}

    def check(color, depth, cams):
        check_strided(color, cs, cp, [want[id(c)][0] for c in cams], "colour")
        check_strided(depth, ds, dp, [want[id(c)][1] for c in cams], "depth")

    c1, d1 = strided_targets(torch, 3, cs, ds)
    r.render_views(c1, d1, sc.input(gsm), [gsm.CameraParams.from_dict(c) for c in cams_a], FW, FH,
                   color_view_stride=cs, depth_view_stride=ds)
    c2, d2 = strided_targets(torch, 3, cs, ds)
    r.render_batch([gsm.BatchView(sc.input(gsm), gsm.CameraParams.from_dict(c), FW, FH, c2[v * cs:], d2[v * ds:])
                    for v, c in enumerate(cams_a)])
    c3, d3 = strided_targets(torch, 3, cs, ds)
    r.render_views(c3, d3, sc.input(gsm), [gsm.CameraParams.from_dict(c) for c in cams_b], FW, FH,
                   color_view_stride=cs, depth_view_stride=ds)
    c4, d4, _ = render_single(gsm, torch, r, sc, cams_b[1], FW, FH)
    torch.cuda.synchronize()
    check(c1, d1, cams_a)
    check(c2, d2, cams_a)
    check(c3, d3, cams_b)
    assert torch.equal(c1, c2) and torch.equal(d1, d2), "render_views and render_batch of the same views differ"
    assert np.array_equal(c4, want[id(cams_b[1])][0]) and np.array_equal(d4, want[id(cams_b[1])][1])
    r.close()
    rs.close()


@pytest.mark.gpu
def test_counters_after_views_keep_their_meaning(gsm, cuda):
    from gsm_amd import scenes
    torch = cuda
    sc = front_scene(torch)
    cams = orbit(scenes, FW, FH, (0.0, 8.0, -8.0))
    rb, rs = batch_handle(gsm, sc, 3, FW, FH), single_handle(gsm, sc, FW, FH)
    render_batch(gsm, torch, rb, sc, cams, FW, FH)
    c = rb.counters()
    assert c["gaussian_count"] == FN, "the scene's count, not the batch's items"
    assert c["overflow"] == 0
    assert c["total_assignments"] == sum(render_single(gsm, torch, rs, sc, cam, FW, FH)[2] for cam in cams) > 0
    rb.close()
    rs.close()


@pytest.mark.gpu
def test_captured_views_frame_replays_its_own_cameras(gsm, cuda):
    """The per-view entries travel as kernel arguments: a frame captured into a graph replays the cameras it was
    captured with, whatever became of the caller's list and whatever the handle rendered since."""
    from gsm_amd import scenes
    torch = cuda
    sc = front_scene(torch)
    cams = orbit(scenes, FW, FH, (0.0, 8.0))
    other = orbit(scenes, FW, FH, (-20.0, 25.0))
    rb, rs = batch_handle(gsm, sc, 2, FW, FH), single_handle(gsm, sc, FW, FH)
    want = [render_single(gsm, torch, rs, sc, c, FW, FH) for c in cams]
    color, depth = targets(torch, 2, FW, FH)
    scratch_c, scratch_d = targets(torch, 2, FW, FH)
    cps = [gsm.CameraParams.from_dict(c) for c in cams]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # (the handle's first batch allocates: not under capture)
        rb.render_views(scratch_c, scratch_d, sc.input(gsm), cps, FW, FH, stream=s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rb.render_views(color, depth, sc.input(gsm), cps, FW, FH, stream=s)
    torch.cuda.synchronize()
    cps[:] = [gsm.CameraParams.from_dict(c) for c in other]
    rb.render_views(scratch_c, scratch_d, sc.input(gsm), cps, FW, FH)
    torch.cuda.synchronize()
    color.fill_(0xA5)
    depth.fill_(0xA5)
    g.replay()
    torch.cuda.synchronize()
    bc, bd = color.cpu().numpy(), depth.cpu().numpy()
    for v in range(2):
        assert np.array_equal(bc[v], want[v][0]), f"view {v} colour: " + diff(bc[v], want[v][0])
        assert np.array_equal(bd[v], want[v][1]), f"view {v} depth: " + diff(bd[v], want[v][1])
    del g
    rb.close()
    rs.close()
