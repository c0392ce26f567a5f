"""gsm_global_render_batch: views of different scenes and sizes in one Global frame.  The
contract is that every view's bytes -- colour and depth -- equal those of gsm_global_render for that view
alone; the yardsticks are `render` on a second handle sized for that view alone and the oracle's frame for
the same scene, camera and size, never the batch itself.  Every target is pre-filled with a sentinel byte
and followed by sentinel rows that must keep it.  Shapes are the smallest that reach each code path (the
rules that pick kernels take the batch's tile count)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

ERR_COUNT, ERR_DIMS, ERR_SIZE, ERR_TILES, ERR_MISSING, ERR_ARG, ERR_UNSUPPORTED = 6, 7, 8, 9, 13, 14, 15
BPP = {0: 8, 1: 16, 2: 4, 3: 4, 4: 4, 5: 4}
FILL, GAP = 0xA5, 3  # the sentinel byte, and the sentinel rows after every target


# ---- 1. declaration, export, binding and layout (no GPU) ----
def test_batch_entry_is_declared_exported_bound_and_laid_out(gsm):
    src = open(os.path.join(ROOT, "include", "gsm_renderer.h")).read()
    assert re.search(r"gsm_status\s+gsm_global_render_batch\s*\(", src)
    assert re.search(r"\}\s*gsm_global_view\s*;", src)
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    assert " T gsm_global_render_batch" in out
    assert "gsm_global_render_batch" in gsm._SIGNATURES
    assert callable(getattr(gsm.GlobalRenderer, "render_batch", None))
    assert {"input", "camera", "width", "height", "color", "depth"} <= set(gsm.BatchView.__dataclass_fields__)
    m = re.search(r"static_assert\s*\(\s*sizeof\s*\(\s*gsm_global_view\s*\)\s*==\s*(\d+)", src)
    assert m, "the header pins sizeof(gsm_global_view)"
    assert C.sizeof(gsm._GlobalView) == int(m.group(1))


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


def roundup256(n):
    return (n + 255) // 256 * 256


def tiles(w, h):
    return ((w + 31) // 32) * ((h + 15) // 16)


def diff(a, b):
    idx = np.nonzero(np.asarray(a).reshape(-1) != np.asarray(b).reshape(-1))[0]
    return f"{idx.size} bytes differ, first at {idx[:4].tolist()}"


class Scene:
    """A scene on the device; max_gaussians: the single frame's handle size (its assignment capacity is 4x)."""

    def __init__(self, torch, world, harm, sh, max_gaussians=None):
        self.world_np, self.harm_np, self.sh = world, harm, sh
        self.n = len(world)
        self.prec = 1 if world.dtype.itemsize == 32 else 0
        self.world, self.harm = to_dev(torch, world), to_dev(torch, harm)
        self.max_gaussians = max(self.n, 1) if max_gaussians is None else max_gaussians

    def input(self, gsm, count=None):
        return gsm.GaussianInput(self.world, self.harm, self.n if count is None else count, self.sh)


class Spec:
    """One view: a scene, a camera and a frame size."""

    def __init__(self, scene, cam, w, h):
        self.sc, self.cam, self.w, self.h = scene, cam, w, h


def batch_handle(gsm, specs, fmt=0, color_space=0, slack=1):
    """A handle whose tile space and item space hold exactly the batch (times `slack`)."""
    mw = max(s.w for s in specs)
    tx = (mw + 31) // 32
    need = slack * sum(tiles(s.w, s.h) for s in specs)
    mh = max(max(s.h for s in specs), 16 * ((need + tx - 1) // tx))
    mg = slack * sum(roundup256(max(s.sc.max_gaussians, s.sc.n)) for s in specs)
    return gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=max(mg, 1), max_width=mw, max_height=mh,
                                                        precision=specs[0].sc.prec, color_format=fmt,
                                                        gaussian_color_space=color_space))


def single_handle(gsm, s, fmt=0, color_space=0):
    return gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=s.sc.max_gaussians, max_width=s.w, max_height=s.h,
                                                        precision=s.sc.prec, color_format=fmt,
                                                        gaussian_color_space=color_space))


def target(torch, w, h, bpp=8):
    color = torch.full((h + GAP, w * bpp), FILL, dtype=torch.uint8, device="cuda")
    depth = torch.full((h + GAP, w * 2), FILL, dtype=torch.uint8, device="cuda")
    return color, depth


def render_batch(gsm, torch, r, specs, bpp=8, no_depth=()):
    """One render_batch call into fresh sentinel targets; returns [(colour rows, depth rows)] per view, with the
    sentinel rows after each checked.  no_depth: views that pass depth = NULL (their would-be target is
    returned as it was left)."""
    tg = [target(torch, s.w, s.h, bpp) for s in specs]
    views = [gsm.BatchView(s.sc.input(gsm), gsm.CameraParams.from_dict(s.cam), s.w, s.h, c,
                           None if v in no_depth else d) for v, (s, (c, d)) in enumerate(zip(specs, tg))]
    r.render_batch(views)
    torch.cuda.synchronize()
    out = []
    for v, (s, (c, d)) in enumerate(zip(specs, tg)):
        c, d = c.cpu().numpy(), d.cpu().numpy()
        assert (c[s.h:] == FILL).all() and (d[s.h:] == FILL).all(), f"view {v}: sentinel rows were written"
        out.append((c[:s.h], d[:s.h]))
    return out


def render_single(gsm, torch, r, s, bpp=8):
    color, depth = target(torch, s.w, s.h, bpp)
    r.render(color, depth, s.sc.input(gsm), gsm.CameraParams.from_dict(s.cam), s.w, s.h)
    torch.cuda.synchronize()
    return color.cpu().numpy()[:s.h], depth.cpu().numpy()[:s.h], r.debug_read_total_assignments()


def oracle_frame(oracle, s, color_space=0):
    ref = oracle.render(s.sc.world_np, s.sc.harm_np, s.sc.sh, s.cam, s.w, s.h, max_gaussians=s.sc.max_gaussians,
                        color_space=color_space, count=s.sc.n)
    return (ref["color"].view(np.uint8).reshape(s.h, -1), ref["depth"].view(np.uint8).reshape(s.h, -1),
            ref["total_assignments"])


def check_batch(gsm, torch, oracle, specs, batch=None, which=None, oracle_views=None, no_depth=()):
    """Render the batch; every view of `which` (all by default) must equal its own frame on a handle sized for
    it alone, and the oracle's frame for oracle_views (all of `which` by default).  Returns (the batch's
    assignment total, the sum of the single frames' when every view was checked, the batch's outputs)."""
    rb = batch or batch_handle(gsm, specs)
    got = render_batch(gsm, torch, rb, specs, no_depth=no_depth)
    total = rb.debug_read_total_assignments()
    assert rb.counters()["overflow"] == 0
    singles = 0
    for v in (range(len(specs)) if which is None else which):
        s = specs[v]
        rs = single_handle(gsm, s)
        c, d, t = render_single(gsm, torch, rs, s)
        assert rs.counters()["overflow"] == 0, "the yardstick frame overflowed: no parity to check"
        rs.close()
        singles += t
        assert np.array_equal(got[v][0], c), f"view {v} colour vs render: " + diff(got[v][0], c)
        if v not in no_depth:
            assert np.array_equal(got[v][1], d), f"view {v} depth vs render: " + diff(got[v][1], d)
        if oracle_views is None or v in oracle_views:
            oc, od, ot = oracle_frame(oracle, s)
            assert np.array_equal(got[v][0], oc), f"view {v} colour vs oracle: " + diff(got[v][0], oc)
            if v not in no_depth:
                assert np.array_equal(got[v][1], od), f"view {v} depth vs oracle: " + diff(got[v][1], od)
            assert t == ot
    if batch is None:
        rb.close()
    return total, singles, got


def gen(torch, scenes, n, w, h, sh, prec, seed, max_gaussians=None):
    world, harm, cam = scenes.gen_scene(n, w, h, sh, prec, seed=seed)
    return Scene(torch, world, harm, sh, max_gaussians), cam


def clear_bytes(h, w):
    """the clear value: colour (0, 0, 0, 1) in fp16, depth 0"""
    c = np.zeros((h, w, 4), np.uint16)
    c[..., 3] = 0x3C00
    return c.view(np.uint8).reshape(h, -1), np.zeros((h, w * 2), np.uint8)


# ---- 2. three scenes, three sizes ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_three_scenes_three_sizes(gsm, cuda, oracle, prec):
    """Counts 1, 257 and 5000 (item bases 0, 256, 768); 33 x 17 (4 tiles, ragged in both axes), 97 x 45 (12
    tiles) and 640 x 360.  The batch's assignment total is the sum of the frames'; the reverse order gives the
    same bytes per view."""
    from gsm_amd import scenes
    specs = []
    for n, (w, h), seed in ((1, (33, 17), 31), (257, (97, 45), 32), (5000, (640, 360), 33)):
        sc, cam = gen(cuda, scenes, n, w, h, 4, prec, seed)
        specs.append(Spec(sc, cam, w, h))
    total, singles, got = check_batch(gsm, cuda, oracle, specs)
    assert total == singles and total > 0
    rb = batch_handle(gsm, specs)
    rev = render_batch(gsm, cuda, rb, specs[::-1])[::-1]
    assert rb.debug_read_total_assignments() == total
    rb.close()
    for v in range(3):
        assert np.array_equal(rev[v][0], got[v][0]) and np.array_equal(rev[v][1], got[v][1]), f"view {v} reversed"


# ---- 3. block boundaries ----
@pytest.mark.gpu
def test_counts_at_the_block_boundary(gsm, cuda, oracle):
    """255, 256 and 257 gaussians of one generator at 64 x 32: a view ending one short of, on, and one past a
    256-item block."""
    from gsm_amd import scenes
    w, h = 64, 32
    world, harm, cam = scenes.gen_scene(257, w, h, 1, 0, seed=34)
    specs = [Spec(Scene(cuda, world[:n].copy(), harm.reshape(257, -1)[:n].reshape(-1).copy(), 1), cam, w, h)
             for n in (255, 256, 257)]
    total, singles, _ = check_batch(gsm, cuda, oracle, specs)
    assert total == singles and total > 0


# ---- 4. same scene and size: render_views ----
@pytest.mark.gpu
def test_same_scene_and_size_matches_render_views(gsm, cuda):
    from gsm_amd import scenes
    w, h, k = 97, 45, 3
    sc, _ = gen(cuda, scenes, 2000, w, h, 1, 0, 35)
    cams = [scenes.orbit_camera(w, h, a) for a in (0.0, 9.0, -14.0)]
    specs = [Spec(sc, c, w, h) for c in cams]
    rb = batch_handle(gsm, specs)
    got = render_batch(gsm, cuda, rb, specs)
    total = rb.debug_read_total_assignments()
    rb.close()
    rv = batch_handle(gsm, specs)
    color = cuda.full((k, h, w * 8), FILL, dtype=cuda.uint8, device="cuda")
    depth = cuda.full((k, h, w * 2), FILL, dtype=cuda.uint8, device="cuda")
    rv.render_views(color, depth, sc.input(gsm), [gsm.CameraParams.from_dict(c) for c in cams], w, h)
    cuda.cuda.synchronize()
    assert rv.debug_read_total_assignments() == total
    rv.close()
    vc, vd = color.cpu().numpy(), depth.cpu().numpy()
    for v in range(k):
        assert np.array_equal(got[v][0], vc[v]), f"view {v} colour: " + diff(got[v][0], vc[v])
        assert np.array_equal(got[v][1], vd[v]), f"view {v} depth: " + diff(got[v][1], vd[v])


# ---- 5. side by side ----
@pytest.mark.gpu
def test_two_views_side_by_side_match_render_stereo_sbs(gsm, cuda):
    """Two views of one scene in one target: view v starts v * width pixels into the rows, both with the shared
    pitch (the second view's targets are 8- and 2-byte aligned only: no wide stores)."""
    from gsm_amd import scenes
    w, h = 97, 45
    sc, _ = gen(cuda, scenes, 3000, w, h, 1, 0, 36)
    left, right = scenes.make_camera(w, h, -0.03), scenes.make_camera(w, h, 0.03)
    inp = sc.input(gsm)

    def pair():
        return (cuda.full((h + GAP, 2 * w * 8), FILL, dtype=cuda.uint8, device="cuda"),
                cuda.full((h + GAP, 2 * w * 2), FILL, dtype=cuda.uint8, device="cuda"))

    rs = single_handle(gsm, Spec(sc, left, w, h))
    sc_c, sc_d = pair()
    rs.render_stereo_sbs(sc_c, sc_d, inp, gsm.CameraParams.from_dict(left), gsm.CameraParams.from_dict(right), w, h)
    cuda.cuda.synchronize()
    rs.close()
    specs = [Spec(sc, left, w, h), Spec(sc, right, w, h)]
    rb = batch_handle(gsm, specs)
    bc, bd = pair()
    views = [gsm.BatchView(inp, gsm.CameraParams.from_dict(s.cam), w, h, bc.data_ptr() + v * w * 8,
                           bd.data_ptr() + v * w * 2, color_pitch=2 * w * 8, depth_pitch=2 * w * 2)
             for v, s in enumerate(specs)]
    rb.render_batch(views)
    cuda.cuda.synchronize()
    rb.close()
    assert cuda.equal(bc, sc_c), "colour: " + diff(bc.cpu().numpy(), sc_c.cpu().numpy())
    assert cuda.equal(bd, sc_d), "depth: " + diff(bd.cpu().numpy(), sc_d.cpu().numpy())
    assert (bc[h:] == FILL).all() and (bd[h:] == FILL).all()


# ---- 6. a view without work ----
@pytest.mark.gpu
def test_view_without_work_between_two_with_work(gsm, cuda, oracle):
    from gsm_amd import scenes
    sa, ca = gen(cuda, scenes, 2000, 97, 45, 1, 0, 37)
    sb, cb = gen(cuda, scenes, 1500, 160, 90, 1, 0, 38)
    away = away_camera(scenes, 64, 40)
    assert oracle.render(sa.world_np, sa.harm_np, 1, away, 64, 40, max_gaussians=sa.n)["total_assignments"] == 0
    specs = [Spec(sa, ca, 97, 45), Spec(sa, away, 64, 40), Spec(sb, cb, 160, 90)]
    total, singles, got = check_batch(gsm, cuda, oracle, specs)
    assert total == singles and total > 0
    cc, cd = clear_bytes(40, 64)
    assert np.array_equal(got[1][0], cc) and np.array_equal(got[1][1], cd)


# ---- 7. per-view NULL depth ----
@pytest.mark.gpu
def test_null_depth_for_one_view_only(gsm, cuda, oracle):
    from gsm_amd import scenes
    sa, ca = gen(cuda, scenes, 2000, 97, 45, 1, 0, 39)
    sb, cb = gen(cuda, scenes, 1500, 160, 90, 1, 0, 40)
    specs = [Spec(sa, ca, 97, 45), Spec(sb, cb, 160, 90), Spec(sa, scenes.orbit_camera(97, 45, 8.0), 97, 45)]
    _, _, got = check_batch(gsm, cuda, oracle, specs, no_depth=(1,))
    assert (got[1][1] == FILL).all(), "view 1 passed depth = NULL: its would-be target was written"


# ---- 8. kernel-selection rules ----
@pytest.mark.gpu
def test_small_batch_one_pass_sort_and_quadrant_units(gsm, cuda, oracle):
    """4 + 12 + 9 tiles: a tile field of <= 8 bits (one pass) and quadrant units."""
    from gsm_amd import scenes
    specs = []
    for n, (w, h), seed in ((600, (33, 17), 41), (3000, (97, 45), 42), (1000, (96, 48), 43)):
        sc, cam = gen(cuda, scenes, n, w, h, 1, 0, seed)
        specs.append(Spec(sc, cam, w, h))
    rb = batch_handle(gsm, specs)
    check_batch(gsm, cuda, oracle, specs, batch=rb)
    assert rb.blend_kernel_kind() == 1
    rb.close()


@pytest.mark.gpu
def test_mixed_batch_two_passes_and_half_tile_units(gsm, cuda, oracle):
    """4 x 460 + 3 x 120 = 2200 tiles: past the one wide pass (2048 tiles) and the quadrant units (8 tiles per CU)."""
    from gsm_amd import scenes
    big, _ = gen(cuda, scenes, 20_000, 640, 360, 1, 0, 44)
    small, _ = gen(cuda, scenes, 5_000, 320, 180, 1, 0, 45)
    specs = [Spec(big, scenes.orbit_camera(640, 360, 5.0 * i), 640, 360) for i in range(4)]
    specs += [Spec(small, scenes.orbit_camera(320, 180, -4.0 * i), 320, 180) for i in range(3)]
    specs = specs[:2] + specs[4:] + specs[2:4]  # sizes interleaved
    rb = batch_handle(gsm, specs)
    check_batch(gsm, cuda, oracle, specs, batch=rb, oracle_views=(0, 2, 6))
    assert rb.blend_kernel_kind() == 2
    rb.close()


@pytest.mark.gpu
def test_mixed_batch_reaching_the_pair_walk(gsm, cuda, oracle):
    """20 x 460 + 27 x 120 = 12 440 tiles, 24 880 half-tile units >= 6 per wave slot of 256 CUs: 16 waves per
    workgroup and the pair walk (k_blend_pw_batch), whose pairs meet units of both sizes.  The first, the last
    and one more view of each size against `render` and the oracle."""
    from gsm_amd import scenes
    big, _ = gen(cuda, scenes, 20_000, 640, 360, 1, 0, 46)
    small, _ = gen(cuda, scenes, 5_000, 320, 180, 1, 0, 47)
    specs = []
    for i in range(27):  # big and small alternate, the last seven are small
        if i < 20:
            specs.append(Spec(big, scenes.orbit_camera(640, 360, 2.0 * (i - 10)), 640, 360))
        specs.append(Spec(small, scenes.orbit_camera(320, 180, 1.5 * (i - 13)), 320, 180))
    assert sum(tiles(s.w, s.h) for s in specs) == 12_440
    rb = batch_handle(gsm, specs)
    check_batch(gsm, cuda, oracle, specs, batch=rb, which=(0, 1, 20, 21, len(specs) - 1))
    assert rb.blend_kernel_kind() == 3, "the batch did not reach the pair walk"
    rb.close()


# ---- 9. exact re-walk ----
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
    """The exact re-walk with per-view stores: the far gaussian covers every tile of the 640 x 360 view and is
    outside the two other views, which have other sizes."""
    from gsm_amd import scenes
    world, harm = far_scene()
    # (room for every assignment: the far gaussian covers all 460 tiles, and a frame over its capacity has no parity)
    sc = Scene(cuda, world, harm, 1, max_gaussians=1024)
    specs = [Spec(sc, scenes.orbit_camera(320, 180, 60.0), 320, 180), Spec(sc, scenes.make_camera(640, 360), 640, 360),
             Spec(sc, scenes.orbit_camera(97, 45, -60.0), 97, 45)]
    vis = [int(oracle.render(world, harm, 1, s.cam, s.w, s.h, max_gaussians=3)["mask"][1]) for s in specs]
    assert vis == [0, 1, 0], "the far gaussian must be visible in view 1 only"
    check_batch(gsm, cuda, oracle, specs)


# ---- 10. adversarial inputs ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_adversarial_inputs_three_views_two_scenes(gsm, cuda, oracle, kind):
    import adversarial
    from gsm_amd import scenes
    a = adversarial.scene(kind, 4000, 160, 90, 4, seed=51)
    b = adversarial.scene(kind, 3000, 97, 45, 4, seed=52)
    sa = Scene(cuda, a["world"], a["harm"], 4, max_gaussians=a["max_gaussians"])
    sb = Scene(cuda, b["world"], b["harm"], 4, max_gaussians=b["max_gaussians"])
    specs = [Spec(sa, a["cam"], 160, 90), Spec(sb, b["cam"], 97, 45), Spec(sa, scenes.orbit_camera(160, 90, 10.0), 160, 90)]
    total, singles, _ = check_batch(gsm, cuda, oracle, specs)
    assert total == singles


# ---- 11. create-time switches ----
@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"GSM_SORT_RANK": "ballot"}, {"GSM_SORT_WIDE": "0"}, {"GSM_BLEND_SCHED": "0"}])
def test_create_time_switches_same_bytes(gsm, cuda, oracle, monkeypatch, env):
    """120 + 49 + 120 tiles (a 9-bit tile field: GSM_SORT_WIDE picks one wide or two narrow passes); two frames,
    so that the second one's blend follows the first one's schedule."""
    from gsm_amd import scenes
    sa, _ = gen(cuda, scenes, 6000, 320, 180, 1, 0, 53)
    sb, cb = gen(cuda, scenes, 2000, 200, 100, 1, 0, 54)
    specs = [Spec(sa, scenes.orbit_camera(320, 180, 0.0), 320, 180), Spec(sb, cb, 200, 100),
             Spec(sa, scenes.orbit_camera(320, 180, 7.0), 320, 180)]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rb = batch_handle(gsm, specs)
    for k in env:
        monkeypatch.delenv(k)
    check_batch(gsm, cuda, oracle, specs, batch=rb)
    check_batch(gsm, cuda, oracle, specs, batch=rb, oracle_views=())
    rb.close()


# ---- 12. handle reuse ----
@pytest.mark.gpu
def test_handle_reuse_render_batch_views_batch_render(gsm, cuda, oracle):
    """render, batch A, render_views, a batch B of another shape, render -- on one handle; every output equals
    its yardstick."""
    from gsm_amd import scenes
    sa, ca = gen(cuda, scenes, 5000, 320, 180, 1, 0, 55)
    sb, cb = gen(cuda, scenes, 2000, 200, 100, 1, 0, 56)
    A = [Spec(sa, ca, 320, 180), Spec(sb, cb, 200, 100), Spec(sa, scenes.orbit_camera(320, 180, 7.0), 320, 180)]
    B = [Spec(sb, scenes.orbit_camera(97, 45, 3.0), 97, 45), Spec(sa, scenes.orbit_camera(200, 100, -3.0), 200, 100)]
    r = batch_handle(gsm, A, slack=2)

    def single_on_r(s):
        got = render_single(gsm, cuda, r, s)
        fresh = single_handle(gsm, s)
        want = render_single(gsm, cuda, fresh, s)
        fresh.close()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]

    single_on_r(A[0])
    check_batch(gsm, cuda, oracle, A, batch=r, oracle_views=(1,))
    # render_views on the same handle: against render on a second handle
    w, h = 320, 180
    cams = [scenes.orbit_camera(w, h, a) for a in (2.0, -2.0)]
    color = cuda.full((2, h, w * 8), FILL, dtype=cuda.uint8, device="cuda")
    depth = cuda.full((2, h, w * 2), FILL, dtype=cuda.uint8, device="cuda")
    r.render_views(color, depth, sa.input(gsm), [gsm.CameraParams.from_dict(c) for c in cams], w, h)
    cuda.cuda.synchronize()
    for v, c in enumerate(cams):
        s = Spec(sa, c, w, h)
        fresh = single_handle(gsm, s)
        want = render_single(gsm, cuda, fresh, s)
        fresh.close()
        assert np.array_equal(color[v].cpu().numpy(), want[0]) and np.array_equal(depth[v].cpu().numpy(), want[1])
    check_batch(gsm, cuda, oracle, B, batch=r, oracle_views=(0,))
    check_batch(gsm, cuda, oracle, A, batch=r, oracle_views=())
    single_on_r(Spec(sb, cb, 200, 100))
    r.close()


# ---- 13. colour formats ----
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 4, 5])
def test_colour_formats_two_views_of_different_sizes(gsm, cuda, fmt):
    from gsm_amd import scenes
    sa, ca = gen(cuda, scenes, 2000, 97, 45, 1, 1, 57)
    sb, cb = gen(cuda, scenes, 1500, 66, 30, 1, 1, 58)
    specs = [Spec(sa, ca, 97, 45), Spec(sb, cb, 66, 30)]
    rb = batch_handle(gsm, specs, fmt=fmt)
    got = render_batch(gsm, cuda, rb, specs, bpp=BPP[fmt])
    rb.close()
    for v, s in enumerate(specs):
        rs = single_handle(gsm, s, fmt=fmt)
        c, d, _ = render_single(gsm, cuda, rs, s, bpp=BPP[fmt])
        rs.close()
        assert np.array_equal(got[v][0], c), f"view {v} colour: " + diff(got[v][0], c)
        assert np.array_equal(got[v][1], d), f"view {v} depth: " + diff(got[v][1], d)


# ---- 14. errors ----
@pytest.mark.gpu
def test_errors_before_enqueue_in_precedence(gsm, cuda):
    from gsm_amd import scenes
    torch = cuda
    w, h, n = 96, 48, 1000  # 3 x 3 = 9 tiles; 1024 items
    world, harm, cam = scenes.gen_scene(n, w, h, 1, 0, seed=59)
    sc = Scene(torch, world, harm, 1)
    cp = gsm.CameraParams.from_dict(cam)
    r = gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=3 * 1024, max_width=w, max_height=3 * h,
                                                     precision=0))  # 27 tiles, 3072 items
    color = torch.full((3, 3 * h, (w + 1) * 8), FILL, dtype=torch.uint8, device="cuda")
    depth = torch.full((3, 3 * h, (w + 1) * 2), FILL, dtype=torch.uint8, device="cuda")

    def view(v=0, width=w, height=h, count=n, sh=1, color_ok=True, depth_ok=True, world_ok=True, **kw):
        inp = gsm.GaussianInput(sc.world if world_ok else None, sc.harm, count, sh)
        return gsm.BatchView(inp, cp, width, height, color[v] if color_ok else None, depth[v] if depth_ok else None, **kw)

    def status(views):
        try:
            r.render_batch(views)
        except gsm.RendererError as e:
            return e.status
        return 0

    ok = view()
    assert status([view(0), view(1), view(2)]) == 0    # every bound at its limit: 3072 items, 27 tiles
    torch.cuda.synchronize()
    color.fill_(FILL)
    depth.fill_(FILL)
    # one case per row
    assert status([]) == ERR_COUNT                                 # view_count == 0
    assert status([ok, view(1, count=3 * 1024 + 1)]) == ERR_COUNT  # a count above max_gaussians
    assert status([ok, view(1), view(2, count=1025)]) == ERR_COUNT  # 1024 + 1024 + 1280 items > 3072
    assert status([ok, view(1, width=w + 1)]) == ERR_DIMS
    assert status([ok, view(1, height=0)]) == ERR_DIMS
    assert status([ok, view(1, height=2 * h), view(2, height=h + 1)]) == ERR_TILES  # 9 + 18 + 12 tiles > 27
    assert status(None) == ERR_MISSING                             # NULL views
    assert status([ok, view(1, color_ok=False)]) == ERR_MISSING
    assert status([ok, view(1, world_ok=False)]) == ERR_MISSING
    assert status([ok, view(1, color_pitch=w * 8 - 4)]) == ERR_SIZE
    assert status([ok, view(1, depth_pitch=w * 2 - 2)]) == ERR_SIZE
    assert status([ok, view(1, color_pitch=w * 8 + 2)]) == ERR_SIZE  # a pitch that misaligns the rows
    assert status([ok, view(1, sh=4)]) == ERR_ARG
    r.set_tile_rows(0, 2)
    assert status([ok, view(1)]) == ERR_UNSUPPORTED
    # precedence: two rows violated at once, the earlier row's status
    assert status([view(0, sh=4), view(1)]) == ERR_ARG              # sh_components before the tile rows
    r.set_tile_rows(0, 0)
    assert status([view(0, width=w + 1), view(1), view(2), view(0, count=n)]) == ERR_COUNT  # count before dimensions
    assert status([view(0, color_ok=False), view(1, height=3 * h), view(2)]) == ERR_TILES   # tiles before a buffer
    assert status([view(0, color_pitch=8), view(1, color_ok=False)]) == ERR_MISSING  # a buffer before sizes,
    #                                                                                   whatever the view index
    assert status([view(0, sh=4, color_pitch=8), view(1)]) == ERR_SIZE  # sizes before sh_components
    torch.cuda.synchronize()
    assert (color == FILL).all() and (depth == FILL).all(), "a refused call wrote to a target"
    assert status([ok, view(1, height=2 * h)]) == 0    # 27 tiles: at the limit
    torch.cuda.synchronize()
    r.close()
    # the 65535-tile bound: a handle of 65536 tiles (the largest gsm_global_create allows)
    big = gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=256, max_width=32 * 256, max_height=16 * 256,
                                                       precision=0))
    inp = gsm.GaussianInput(sc.world, sc.harm, 0, 1)
    with pytest.raises(gsm.RendererError) as e:
        big.render_batch([gsm.BatchView(inp, cp, 32 * 256, 16 * 256, color, None)])  # 65536 tiles
    assert e.value.status == ERR_TILES
    big.close()


# ---- 15. capacity overflow ----
@pytest.mark.gpu
def test_batch_over_the_shared_capacity_sets_the_overflow_counter(gsm, cuda):
    """Two views whose assignments together exceed 4 * max_gaussians: GSM_OK and the overflow counter; no
    parity is promised (none is asserted)."""
    from gsm_amd import scenes
    w, h = 320, 180
    world, harm, cam = scenes.gen_scene(512, w, h, 1, 0, seed=60, scale_px=40.0)
    sc = Scene(cuda, world, harm, 1)
    specs = [Spec(sc, cam, w, h), Spec(sc, scenes.orbit_camera(w, h, 5.0), w, h)]
    rb = batch_handle(gsm, specs)  # 1024 items: a capacity of 4096 assignments
    render_batch(gsm, cuda, rb, specs)
    c = rb.counters()
    rb.close()
    assert c["overflow"] == 1 and c["total_assignments"] == c["max_capacity"] == 4096
