"""gsm_global_render_pick, gsm_global_render_composite_pick and gsm_global_pick_owner.  Every frame
asserts three things: colour and depth bytes equal the plain entry's on a second handle; the pick equals the
checker's (tests/pick/pick_ref.c, whose own blend must equal the oracle's: "differ" == 0); the pick target's
padding -- columns past the width, rows past the height -- still holds its sentinel.  Shapes are the smallest that
reach each path of the walk."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

ERR_SIZE, ERR_RENDER_FAILED, ERR_MISSING, ERR_UNSUPPORTED = 8, 11, 13, 15
FILL, GAP = 0xA5, 3
PFILL = 0xA5A5A5A5
NONE = 0xFFFFFFFF


# ---- helpers ----
def to_dev(torch, arr):
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def roundup256(n):
    return (n + 255) // 256 * 256


class Scene:
    def __init__(self, torch, world, harm, sh):
        self.world_np, self.harm_np, self.sh = world, np.asarray(harm).reshape(-1), sh
        self.n = len(world)
        self.prec = 1 if world.dtype.itemsize == 32 else 0
        if torch is not None and self.n:
            self.world, self.harm = to_dev(torch, world), to_dev(torch, self.harm_np)
        else:
            self.world = self.harm = None

    def input(self, gsm):
        return gsm.GaussianInput(self.world, self.harm, self.n, self.sh)


def gen(torch, n, w, h, sh, prec, seed, opacity=None, **kw):
    from gsm_amd import scenes
    world, harm, _ = scenes.gen_scene(n, w, h, sh, prec, seed=seed, **kw)
    if opacity is not None:  # overwrite the opacities with uniform values of [lo, hi]
        op = np.random.default_rng(seed + 1).uniform(opacity[0], opacity[1], n).astype(np.float32)
        world["opacity"] = op if prec == 0 else op.astype(np.float16).view(np.uint16)
    return Scene(torch, world, harm, sh)


def handle(gsm, max_gaussians, mw, mh, prec):
    return gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=max(max_gaussians, 1), max_width=mw,
                                                        max_height=mh, precision=prec, color_format=0,
                                                        gaussian_color_space=0))


class Targets:
    """Sentinel-filled colour, depth and pick targets; the pick rows are `pad` words longer than the width."""

    def __init__(self, torch, w, h, pad=2):
        self.torch, self.w, self.h, self.pad = torch, w, h, pad
        self.color = torch.full((h + GAP, w * 8), FILL, dtype=torch.uint8, device="cuda")
        self.depth = torch.full((h + GAP, w * 2), FILL, dtype=torch.uint8, device="cuda")
        self.pick = torch.full((h + GAP, (w + pad) * 4), FILL, dtype=torch.uint8, device="cuda")
        self.pick_pitch = (w + pad) * 4

    def refill(self):
        for t in (self.color, self.depth, self.pick):
            t.fill_(FILL)

    def read(self, with_pick=True):
        """(colour rows, depth rows, pick image): the sentinel rows and the pick padding checked."""
        self.torch.cuda.synchronize()
        c, d = self.color.cpu().numpy(), self.depth.cpu().numpy()
        p = self.pick.cpu().numpy().view(np.uint32)
        assert (c[self.h:] == FILL).all() and (d[self.h:] == FILL).all(), "sentinel rows were written"
        assert (p[self.h:] == PFILL).all(), "pick rows past the height were written"
        assert (p[:, self.w:] == PFILL).all(), "pick bytes past 4 * width were written"
        if with_pick:
            assert not (p[:self.h, :self.w] == PFILL).any(), "a pixel of the pick target was not written"
        return c[:self.h], d[:self.h], p[:self.h, :self.w].copy()

    def untouched(self):
        self.torch.cuda.synchronize()
        return all((t.cpu().numpy() == FILL).all() for t in (self.color, self.depth, self.pick))


def pick_frame(gsm, torch, r, sc, cam, w, h, pad=2):
    t = Targets(torch, w, h, pad)
    r.render_pick(t.color, t.depth, t.pick, sc.input(gsm), gsm.CameraParams.from_dict(cam), w, h,
                  pick_pitch=t.pick_pitch)
    return t.read()


def plain_frame(gsm, torch, r, sc, cam, w, h):
    t = Targets(torch, w, h)
    r.render(t.color, t.depth, sc.input(gsm), gsm.CameraParams.from_dict(cam), w, h)
    c, d, _ = t.read(with_pick=False)
    return c, d


def checker(sc, cam, w, h, M, mw, mh):
    import pick_ref
    fr = pick_ref.render(sc.world_np, sc.harm_np, sc.sh, cam, w, h, max_gaussians=M, max_width=mw, max_height=mh)
    assert fr["status"] == 0 and fr["overflow"] == 0
    assert fr["differ"] == 0, "the checker's blend is not the oracle's"
    return fr


def frame_bytes(fr, h):
    return fr["color"].view(np.uint8).reshape(h, -1), fr["depth"].view(np.uint8).reshape(h, -1)


def check_render_pick(gsm, torch, sc, cam, w, h, mw=None, mh=None, M=None, kind=None, pad=2):
    """One render_pick against the plain entry on a second handle and against the checker; returns the checker's
    frame and the GPU's pick."""
    mw, mh, M = mw or w, mh or h, M or max(sc.n, 1)
    rp = handle(gsm, M, mw, mh, sc.prec)
    gc, gd, gp = pick_frame(gsm, torch, rp, sc, cam, w, h, pad)
    assert rp.counters()["overflow"] == 0
    if kind is not None:
        assert rp.blend_kernel_kind() == kind
    obj, gid = rp.pick_owner(gp)
    rp.close()
    rs = handle(gsm, M, mw, mh, sc.prec)
    sc_, sd_ = plain_frame(gsm, torch, rs, sc, cam, w, h)
    rs.close()
    assert np.array_equal(gc, sc_), "colour differs from the plain entry's"
    assert np.array_equal(gd, sd_), "depth differs from the plain entry's"
    fr = checker(sc, cam, w, h, M, mw, mh)
    oc, od = frame_bytes(fr, h)
    assert np.array_equal(gc, oc) and np.array_equal(gd, od), "the frame differs from the oracle's"
    bad = np.argwhere(gp != fr["pick"])
    assert len(bad) == 0, f"{len(bad)} picks differ, first (y, x) {bad[:4].tolist()}"
    # the owner of a single frame's item: object 0 and the id itself; none for none
    hit = gp != NONE
    assert (obj[hit] == 0).all() and np.array_equal(gid[hit], gp[hit])
    assert (obj[~hit] == NONE).all() and (gid[~hit] == NONE).all()
    return fr, gp


def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def handle_size_for_tiles(tiles):
    """A handle size of at least `tiles` 32 x 16 tiles: 64 tile rows (1024 pixels) of as many tiles as it takes."""
    return 32 * ((tiles + 63) // 64), 1024


# ---- 0. declaration, export, binding (no GPU) ----
def test_pick_entries_are_declared_exported_and_bound(gsm):
    import re
    import subprocess
    root = os.path.dirname(HERE)
    src = open(os.path.join(root, "include", "gsm_renderer.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    for name in ("gsm_global_render_pick", "gsm_global_render_composite_pick", "gsm_global_pick_owner"):
        assert re.search(r"gsm_status\s+%s\s*\(" % name, src), name
        assert f" T {name}\n" in out, name
        assert name in gsm._SIGNATURES
    assert re.search(r"#define\s+GSM_PICK_NONE\s+0xFFFFFFFFu", src) and gsm.PICK_NONE == NONE
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    for name in ("render_pick", "render_composite_pick", "pick_owner"):
        assert callable(getattr(gsm.GlobalRenderer, name, None)), name


# ---- 1. render_pick ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec,sh", [(1, 16), (0, 1)])
@pytest.mark.parametrize("w,h,pad", [(320, 180, 2), (203, 77, 2), (203, 77, 3)])
def test_render_pick_matches_the_checker(gsm, cuda, prec, sh, w, h, pad):
    """320x180: 12 tile rows, the last one partial; aligned targets (16-byte colour, 8-byte pick stores).  203x77:
    an odd width that is no multiple of 32 -- the colour pitch is no multiple of 16, the last pair of a row has
    px + 1 == W; with 2 words of padding the pick pitch is no multiple of 8 (4-byte pick stores), with 3 it is."""
    from gsm_amd import scenes
    sc = gen(cuda, 4096, w, h, sh, prec, 3)
    fr, gp = check_render_pick(gsm, cuda, sc, scenes.make_camera(w, h), w, h, pad=pad)
    assert (gp != NONE).any() and (gp == NONE).any()


# ---- 2. both unit shapes, every instance ----
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["quadrant-8", "quadrant-12", "quadrant-16", "half-8", "half-12", "half-16"])
def test_both_unit_shapes_and_every_wave_count(gsm, cuda, monkeypatch, case):
    """The host's rule (gsm_blend.hip, blend_pairs_per_lane and blend_waves_per_wg), the plain frame's: with T the
    tiles of the handle's grid and C the device's CUs, quadrant units (4 per tile) while T <= 8 C, half-tile units
    (2 per tile) beyond; 16 waves per workgroup from 96 C units, 12 from 24 C, else 8.  The frame stays 320x180;
    the handle's size sets T.  Quadrant units never reach 96 C units, so that instance takes the handle's
    GSM_BLEND_WAVES=16 override."""
    from gsm_amd import scenes
    C_ = cus(cuda)
    w, h = 320, 180
    shape, waves = case.split("-")
    if shape == "quadrant":
        kind = 1
        tiles = {"8": 120, "12": 6 * C_, "16": 120}[waves]   # 4 T >= 24 C
        if waves == "16":
            monkeypatch.setenv("GSM_BLEND_WAVES", "16")
    else:
        kind = 2
        tiles = {"8": 8 * C_ + 1, "12": 12 * C_, "16": 48 * C_}[waves]   # 2 T >= 24 C, 2 T >= 96 C
    mw, mh = (w, h) if tiles == 120 else handle_size_for_tiles(tiles)
    T = ((mw + 31) // 32) * ((mh + 15) // 16)
    assert (T <= 8 * C_) == (kind == 1) and T <= 65536
    sc = gen(cuda, 4096, w, h, 1, 0, 4)
    check_render_pick(gsm, cuda, sc, scenes.make_camera(w, h), w, h, mw=mw, mh=mh, kind=kind)


# ---- 3. long walks ----
LONG = dict(n=8192, w=64, h=32, spread=0.5, scale_px=1.2)


def _units(cuda, kind):
    return (64, 32) if kind == 1 else handle_size_for_tiles(8 * cus(cuda) + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("prec", [0, 1])
def test_long_walks_pick_in_every_batch_position(gsm, cuda, kind, prec):
    """Opacities of [0.02, 0.05] on 8192 small gaussians over 64x32: nothing saturates, the tile lists run to
    hundreds of entries, and the walk's four-batch pipeline (256 entries deep) turns over more than once.  The
    conditions on the input, from the checker: a group walks past 256 entries, and winners sit at list positions
    >= 192, >= 256 and in every quarter of the 256-entry cycle."""
    from gsm_amd import scenes
    w, h = LONG["w"], LONG["h"]
    sc = gen(cuda, LONG["n"], w, h, 1, prec, 21, opacity=(0.02, 0.05), spread=LONG["spread"],
             scale_px=LONG["scale_px"])
    mw, mh = _units(cuda, kind)
    fr, gp = check_render_pick(gsm, cuda, sc, scenes.make_camera(w, h), w, h, mw=mw, mh=mh, M=4 * sc.n, kind=kind)
    pos = fr["pick_pos"][fr["pick_pos"] != NONE]
    assert fr["group_iters"].max() > 256, "the test's premise: a walk longer than the pipeline is deep"
    assert (pos >= 192).any() and (pos >= 256).any()
    assert (np.histogram(pos % 256, bins=4, range=(0, 256))[0] > 0).all(), "winners in every batch position"


# ---- 4. early break ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
def test_groups_that_break_early_keep_their_pick(gsm, cuda, kind):
    """The default opacities (0.5 - 1.0) at that density: groups saturate long before their list's end."""
    from gsm_amd import scenes
    w, h = LONG["w"], LONG["h"]
    sc = gen(cuda, 2048, w, h, 1, 0, 21, spread=LONG["spread"], scale_px=LONG["scale_px"])
    mw, mh = _units(cuda, kind)
    fr, gp = check_render_pick(gsm, cuda, sc, scenes.make_camera(w, h), w, h, mw=mw, mh=mh, M=4 * sc.n, kind=kind)
    counts = fr["headers"][:, 1]
    tiles = (np.arange(h)[:, None] // 16) * fr["tiles_x"] + np.arange(w)[None, :] // 32
    iters = fr["group_iters"][tiles, (np.arange(h)[:, None] % 16) // 2, (np.arange(w)[None, :] % 32) // 4]
    broke = iters < counts[tiles]
    assert broke.any() and not broke.all(), "the test's premise: some groups broke before their list's end"
    assert np.array_equal(gp[broke], fr["pick"][broke]) and (gp[broke] != NONE).all()


# ---- 5. the exact rewalk ----
def far_scene(torch, prec):
    """3000 ordinary gaussians; 24 of them moved past fp16's depth range (view depth 6.6e4 .. 2e5: an fp16 depth
    of inf) and made large enough to cover pixels there, 16 given a NaN opacity (the projection culls those)."""
    from gsm_amd import scenes
    w, h, n = 320, 180, 3000
    world, harm, cam = scenes.gen_scene(n, w, h, 1, prec, seed=9)
    val = (lambda v: np.float32(v)) if prec == 0 else (lambda v: np.float16(v).view(np.uint16))
    far = np.arange(24)
    world["pz"][far] = np.linspace(6.6e4, 2e5, 24).astype(np.float32)
    world["px"][far] = np.linspace(-3e4, 3e4, 24).astype(np.float32)
    world["py"][far] = np.linspace(-1.5e4, 1.5e4, 24).astype(np.float32)
    for axis in ("sx", "sy", "sz"):
        world[axis][far] = val(3000.0)
    world["opacity"][far] = val(0.9)
    world["opacity"][np.arange(24, 40)] = val(np.nan)
    return Scene(torch, world, harm, 1), cam, far


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("prec", [0, 1])
def test_units_walked_again_exactly_rewrite_their_pick(gsm, cuda, prec, kind):
    """Records of inf fp16 depth: every unit that stages one is walked again by walk_unit_exact, which rewrites
    all of its pixels, the pick with them.  The conditions on the input, from the checker: such records are
    listed, they leave inf and NaN depth pixels, and some of them are picked."""
    w, h = 320, 180
    sc, cam, far = far_scene(cuda, prec)
    mw, mh = (w, h) if kind == 1 else handle_size_for_tiles(8 * cus(cuda) + 1)
    fr, gp = check_render_pick(gsm, cuda, sc, cam, w, h, mw=mw, mh=mh, M=4 * sc.n, kind=kind)
    listed = np.unique(fr["sorted_values"][fr["sorted_values"] >= 0])
    assert ((fr["records"][listed, 9] & 0x7C00) == 0x7C00).any(), "the test's premise: a listed record of inf depth"
    dep = fr["depth"].view(np.float16)
    assert np.isinf(dep).any() and np.isnan(dep).any()
    assert np.isin(gp, far).any() and (gp == NONE).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,w,h,sh,seed", [("f32", 20_000, 640, 360, 16, 5), ("f16", 20_000, 640, 360, 16, 6)])
def test_adversarial_scenes_keep_their_pick(gsm, cuda, kind, n, w, h, sh, seed):
    """tests/adversarial.py at test_adversarial_scenes_bit_exact's 640x360 sizes: extreme, inf and NaN positions,
    scales, rotations, opacities and SH coefficients.  (At these sizes the projection culls every gaussian whose
    depth or opacity is not finite -- the checker lists none -- so the rewalk's own case is the test above.)"""
    import adversarial
    case = adversarial.scene(kind, n, w, h, sh, seed)
    sc = Scene(cuda, case["world"], case["harm"], sh)
    check_render_pick(gsm, cuda, sc, case["cam"], w, h, M=case["max_gaussians"])


# ---- 6. the composite ----
def composite_pick(gsm, torch, r, pairs, w, h, pad=2):
    t = Targets(torch, w, h, pad)
    objs = [gsm.SceneObject(s.input(gsm), gsm.CameraParams.from_dict(c)) for s, c in pairs]
    r.render_composite_pick(t.color, t.depth, t.pick, objs, w, h, pick_pitch=t.pick_pitch)
    return t.read()


def composite_plain(gsm, torch, r, pairs, w, h):
    t = Targets(torch, w, h)
    objs = [gsm.SceneObject(s.input(gsm), gsm.CameraParams.from_dict(c)) for s, c in pairs]
    r.render_composite(t.color, t.depth, objs, w, h)
    c, d, _ = t.read(with_pick=False)
    return c, d


def split_ids(ids, counts):
    """concatenated ids -> (object, gaussian id), NONE for NONE; objects of count 0 own no id"""
    ends = np.cumsum(counts)
    first = ends - np.asarray(counts)
    hit = ids != NONE
    obj = np.full(ids.shape, NONE, np.uint32)
    gid = np.full(ids.shape, NONE, np.uint32)
    o = np.searchsorted(ends, ids[hit], side="right")
    obj[hit], gid[hit] = o, ids[hit] - first[o]
    return obj, gid


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_composite_pick_owners_match_the_checker(gsm, cuda, prec):
    """Counts 300, 0, 1000, 257 -- no multiple of 256, an empty object in between -- under three distinct poses."""
    import pick_ref
    from gsm_amd import scenes
    w, h = 320, 180
    counts = (300, 0, 1000, 257)
    scs = [gen(cuda, n, w, h, 4, prec, 30 + i) for i, n in enumerate(counts)]
    cam = scenes.make_camera(w, h)
    poses = []
    for i, t in enumerate(((0.3, -0.2, 0.4), (0, 0, 0), (-0.4, 0.1, -0.3), (0.1, 0.3, 0.6))):
        M = np.eye(4)
        a = np.radians(9.0 * (i + 1))
        M[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        p = np.array([0.0, 0.0, 5.5])
        M[:3, 3] = p - M[:3, :3] @ p + np.asarray(t)
        poses.append(M.T.reshape(-1))
    pairs = [(s, scenes.object_camera(cam, m)) for s, m in zip(scs, poses)]
    assert len({pairs[i][1]["view"].tobytes() for i in (0, 2, 3)}) == 3
    M_ = sum(roundup256(n) for n in counts)
    rp = handle(gsm, M_, w, h, prec)
    gc, gd, gp = composite_pick(gsm, cuda, rp, pairs, w, h)
    assert rp.counters()["overflow"] == 0
    obj, gid = rp.pick_owner(gp)
    # items that name nothing: none, the frame's item count, and object 0's items past its count
    o2, g2 = rp.pick_owner(np.array([NONE, M_, 300, 511, 299, 512], np.uint32))
    assert o2.tolist() == [NONE, NONE, NONE, NONE, 0, 2] and g2.tolist() == [NONE, NONE, NONE, NONE, 299, 0]
    rp.close()
    rs = handle(gsm, M_, w, h, prec)
    sc_, sd_ = composite_plain(gsm, cuda, rs, pairs, w, h)
    rs.close()
    assert np.array_equal(gc, sc_) and np.array_equal(gd, sd_), "colour / depth differ from the plain entry's"
    fr = pick_ref.render_composite([(s.world_np, s.harm_np, c) for s, c in pairs], 4, w, h, max_gaussians=M_)
    assert fr["status"] == 0 and fr["differ"] == 0 and fr["overflow"] == 0 and fr["total_assignments"] > 0
    oc, od = frame_bytes(fr, h)
    assert np.array_equal(gc, oc) and np.array_equal(gd, od)
    wo, wg = split_ids(fr["pick"], counts)
    assert np.array_equal(obj, wo) and np.array_equal(gid, wg)
    assert set(np.unique(obj).tolist()) == {0, 2, 3, NONE}, "every object with gaussians is picked somewhere"
    # the items themselves follow the composite's layout: 256 * B_o + id
    base = np.cumsum([0] + [roundup256(n) for n in counts])[:-1]
    hit = gp != NONE
    assert np.array_equal(gp[hit], (base[wo[hit]] + wg[hit]).astype(np.uint32))


@pytest.mark.gpu
def test_composite_pick_under_one_camera_is_render_pick_of_the_concatenation(gsm, cuda):
    from gsm_amd import scenes
    w, h = 203, 77
    counts = (300, 0, 1000, 257)
    scs = [gen(cuda, n, w, h, 1, 0, 40 + i) for i, n in enumerate(counts)]
    cam = scenes.make_camera(w, h)
    M_ = sum(roundup256(n) for n in counts)
    rp = handle(gsm, M_, w, h, 0)
    gc, gd, gp = composite_pick(gsm, cuda, rp, [(s, cam) for s in scs], w, h)
    rp.close()
    cat = Scene(cuda, np.concatenate([s.world_np for s in scs]), np.concatenate([s.harm_np for s in scs]), 1)
    rs = handle(gsm, M_, w, h, 0)
    sc_, sd_, sp = pick_frame(gsm, cuda, rs, cat, cam, w, h)
    rs.close()
    assert np.array_equal(gc, sc_) and np.array_equal(gd, sd_)
    wo, wg = split_ids(sp, counts)
    base = np.cumsum([0] + [roundup256(n) for n in counts])[:-1]
    want = np.full(sp.shape, NONE, np.uint32)
    hit = sp != NONE
    want[hit] = base[wo[hit]] + wg[hit]
    assert np.array_equal(gp, want) and hit.any()


# ---- 7. empty frames ----
@pytest.mark.gpu
def test_empty_frames_hold_no_pick(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    A = gen(None, 4, w, h, 1, 0, 50)
    E = Scene(cuda, A.world_np[:0].copy(), A.harm_np[:0].copy(), 1)
    cam = scenes.make_camera(w, h)
    clear = np.zeros((h, w, 4), np.uint16)
    clear[..., 3] = 0x3C00
    r = handle(gsm, 256, w, h, 0)
    for frame in (lambda: pick_frame(gsm, cuda, r, E, cam, w, h),
                  lambda: composite_pick(gsm, cuda, r, [(E, cam), (E, cam)], w, h)):
        gc, gd, gp = frame()
        assert (gp == NONE).all()
        assert np.array_equal(gc, clear.view(np.uint8).reshape(h, -1)) and (gd == 0).all()
        obj, gid = r.pick_owner(np.array([0, 1, NONE], np.uint32))
        assert (obj == NONE).all() and (gid == NONE).all()
    r.close()


# ---- 8. state ----
@pytest.mark.gpu
def test_pick_and_plain_frames_share_a_handle_and_replay(gsm, cuda):
    """pick, plain, pick with three scenes on one handle, twice (the second round meets the first's schedule), then
    the same three frames replayed from a captured graph: each equals the frame of a fresh handle."""
    from gsm_amd import scenes
    w, h = 203, 77
    scs = [gen(cuda, n, w, h, 1, 0, 60 + i) for i, n in enumerate((3000, 2000, 4000))]
    cams = [scenes.orbit_camera(w, h, a) for a in (0.0, 7.0, -5.0)]
    M_ = 4096
    fresh = []
    for i, (sc, cam) in enumerate(zip(scs, cams)):
        r = handle(gsm, M_, w, h, 0)
        fresh.append(plain_frame(gsm, cuda, r, sc, cam, w, h) if i == 1 else pick_frame(gsm, cuda, r, sc, cam, w, h))
        r.close()
    assert checker(scs[0], cams[0], w, h, M_, w, h)["pick"].tolist() == fresh[0][2].tolist(), "the yardstick"

    def same(a, b):
        return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))

    r = handle(gsm, M_, w, h, 0)
    for _ in range(2):
        assert same(pick_frame(gsm, cuda, r, scs[0], cams[0], w, h), fresh[0])
        r.pick_owner(np.array([0], np.uint32))
        assert same(plain_frame(gsm, cuda, r, scs[1], cams[1], w, h), fresh[1])
        with pytest.raises(gsm.RendererError) as e:
            r.pick_owner(np.array([0], np.uint32))
        assert int(e.value.status) == ERR_RENDER_FAILED
        assert same(pick_frame(gsm, cuda, r, scs[2], cams[2], w, h), fresh[2])
    # captured and replayed
    ts = [Targets(cuda, w, h) for _ in range(3)]
    cps = [gsm.CameraParams.from_dict(c) for c in cams]
    s = cuda.cuda.Stream()
    cuda.cuda.synchronize()
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        r.render_pick(ts[0].color, ts[0].depth, ts[0].pick, scs[0].input(gsm), cps[0], w, h, stream=s,
                      pick_pitch=ts[0].pick_pitch)
        r.render(ts[1].color, ts[1].depth, scs[1].input(gsm), cps[1], w, h, stream=s)
        r.render_pick(ts[2].color, ts[2].depth, ts[2].pick, scs[2].input(gsm), cps[2], w, h, stream=s,
                      pick_pitch=ts[2].pick_pitch)
    cuda.cuda.synchronize()
    for _ in range(2):
        for t in ts:
            t.refill()
        g.replay()
        got = [t.read(with_pick=i != 1) for i, t in enumerate(ts)]
        assert same(got[0], fresh[0]) and same(got[1][:2], fresh[1]) and same(got[2], fresh[2])
    obj, gid = r.pick_owner(np.array([5, 4000, NONE], np.uint32))  # (the last enqueued frame: 4000 gaussians)
    assert obj.tolist() == [0, NONE, NONE] and gid.tolist() == [5, NONE, NONE]
    r.close()


# ---- 9. refusals ----
@pytest.mark.gpu
def test_refusals_enqueue_nothing(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    A, B = gen(cuda, 300, w, h, 1, 0, 70), gen(cuda, 500, w, h, 1, 0, 71)
    cam = gsm.CameraParams.from_dict(scenes.make_camera(w, h))
    r = handle(gsm, 1024, w, h, 0)
    t = Targets(cuda, w, h, pad=0)
    objs = [gsm.SceneObject(A.input(gsm), cam), gsm.SceneObject(B.input(gsm), cam)]

    def status(composite, pick=t.pick, color=t.color, **kw):
        try:
            if composite:
                r.render_composite_pick(color, t.depth, pick, objs, w, h, **kw)
            else:
                r.render_pick(color, t.depth, pick, A.input(gsm), cam, w, h, **kw)
        except gsm.RendererError as e:
            return int(e.status)
        return 0

    for comp in (False, True):
        assert status(comp, pick=None) == ERR_MISSING
        assert status(comp, pick_pitch=4 * w - 4) == ERR_SIZE
        assert status(comp, pick_pitch=4 * w + 2) == ERR_SIZE
        assert status(comp, pick=int(t.pick.data_ptr()) + 2) == ERR_SIZE
        # the plain entry's order: a missing buffer before a size, colour's size with the pick's
        assert status(comp, pick=None, color_pitch=8 * w - 4) == ERR_MISSING
        assert status(comp, color=None, pick_pitch=4 * w - 4) == ERR_MISSING
        assert status(comp, color_pitch=8 * w - 4) == ERR_SIZE
        r.set_tile_rows(1, 2)
        assert status(comp) == ERR_UNSUPPORTED
        assert status(comp, pick_pitch=4 * w - 4) == ERR_SIZE, "the size before the tile rows"
        r.set_tile_rows(0, 0)
    assert t.untouched(), "a refused call wrote"
    assert status(False) == 0 and status(True) == 0
    c, d, p = t.read()
    assert (p != NONE).any()
    r.close()
