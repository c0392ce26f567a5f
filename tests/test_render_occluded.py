"""gsm_global_render_occluded and gsm_global_render_composite_occluded.  Every frame is compared,
byte for byte, with the checker's (tests/occlude/occlude_ref.c, whose own blend must equal the oracle's under an
occluder of all +inf): colour, depth, the targets' padding -- columns past the width, rows past the height -- and
the occluder itself, which the frame only reads.  Shapes are the smallest that reach each path of the walk."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_render_pick import Scene, cus, far_scene, gen, handle, handle_size_for_tiles, roundup256  # noqa: E402

ERR_SIZE, ERR_MISSING, ERR_UNSUPPORTED = 8, 13, 15
FILL, GAP = 0xA5, 3
INF = np.float32(np.inf)


# ---- helpers ----
class Targets:
    """Sentinel-filled colour and depth targets, their rows `pad` pixels longer than the width, and the occluder
    on the device, its rows `opad` floats longer (the padding holds a value that would close every pixel)."""

    def __init__(self, torch, w, h, occ, opad=0, pad=2):
        self.torch, self.w, self.h = torch, w, h
        self.color = torch.full((h + GAP, (w + pad) * 8), FILL, dtype=torch.uint8, device="cuda")
        self.depth = torch.full((h + GAP, (w + pad) * 2), FILL, dtype=torch.uint8, device="cuda")
        self.color_pitch, self.depth_pitch = (w + pad) * 8, (w + pad) * 2
        self.occ_np = None
        if occ is not None:
            self.occ_np = np.full((h + GAP, w + opad), -1.0, np.float32)
            self.occ_np[:h, :w] = occ
            self.occ = torch.from_numpy(self.occ_np.copy()).cuda()
            self.occ_pitch = (w + opad) * 4

    def refill(self):
        self.color.fill_(FILL)
        self.depth.fill_(FILL)

    def read(self):
        """(colour bytes, depth bytes) of the frame; the padding and the occluder checked."""
        self.torch.cuda.synchronize()
        c, d = self.color.cpu().numpy(), self.depth.cpu().numpy()
        assert (c[self.h:] == FILL).all() and (d[self.h:] == FILL).all(), "rows past the height were written"
        assert (c[:, self.w * 8:] == FILL).all(), "colour bytes past the width were written"
        assert (d[:, self.w * 2:] == FILL).all(), "depth bytes past the width were written"
        if self.occ_np is not None:
            assert np.array_equal(self.occ.cpu().numpy().view(np.uint32), self.occ_np.view(np.uint32)), \
                "the occluder was written"
        return c[:self.h, :self.w * 8].copy(), d[:self.h, :self.w * 2].copy()

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.color.cpu().numpy() == FILL).all() and (self.depth.cpu().numpy() == FILL).all())


def occluded_frame(gsm, torch, r, sc, cam, w, h, occ, opad=0):
    t = Targets(torch, w, h, occ, opad)
    r.render_occluded(t.color, t.depth, t.occ, sc.input(gsm), gsm.CameraParams.from_dict(cam), w, h,
                      color_pitch=t.color_pitch, depth_pitch=t.depth_pitch, occluder_pitch=t.occ_pitch)
    return t.read()


def plain_frame(gsm, torch, r, sc, cam, w, h):
    t = Targets(torch, w, h, None)
    r.render(t.color, t.depth, sc.input(gsm), gsm.CameraParams.from_dict(cam), w, h, color_pitch=t.color_pitch,
             depth_pitch=t.depth_pitch)
    return t.read()


def ref_bytes(res, h):
    return res["color"].view(np.uint8).reshape(h, -1), res["depth"].view(np.uint8).reshape(h, -1)


def oracle_frame(sc, cam, w, h, M=None, mw=None, mh=None):
    import occlude_ref
    fr = occlude_ref.frame(sc.world_np, sc.harm_np, sc.sh, cam, w, h, max_gaussians=M or max(sc.n, 1),
                           max_width=mw or w, max_height=mh or h)
    assert fr.base["overflow"] == 0
    return fr


def visible_depths(base):
    """fp16 depths (as float32, ascending) of the gaussians the frame lists"""
    ids = np.unique(base["sorted_values"][base["sorted_values"] >= 0])
    return np.sort(base["records"][ids, 9].view(np.float16).astype(np.float32))


def quantile(deps, q):
    return np.float32(deps[min(len(deps) - 1, int(q * len(deps)))])


def random_occluder(deps, w, h, seed, qs=(0.15, 0.35, 0.6)):
    """Per-pixel draws from {below near, three quantiles of the scene's own fp16 depths, +inf, NaN, 0, a negative
    value, 1e30}."""
    palette = np.array([0.01] + [quantile(deps, q) for q in qs] + [np.inf, np.nan, 0.0, -3.0, 1e30], np.float32)
    return palette[np.random.default_rng(seed).integers(0, len(palette), (h, w))]


def ramp_occluder(deps, w, h):
    """A horizontal ramp from the near plane's side of every depth to past the farthest."""
    return np.broadcast_to(np.linspace(0.05, float(deps[-1]) * 1.05, w, dtype=np.float32), (h, w)).copy()


def checker_occluder(w, h):
    """A one-pixel checkerboard of "in front of everything" and +inf."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((xx + yy) % 2 == 0, np.float32(0.01), INF).astype(np.float32)


def assert_not_vacuous(fr, res, what):
    """The conditions on the input, from the checker alone: the occluder closes 20 % to 80 % of the pixels of active
    tiles, changes at least 10 % of them, breaks groups that transmittance alone would not, and leaves groups with
    closed and open pixels side by side."""
    active = fr.active_pixels()
    n = int(active.sum())
    assert res["closure_breaks"] > 0, what
    assert res["mixed_groups"] > 0, what
    assert 0.2 * n <= res["closed_pixels"] <= 0.8 * n, (what, res["closed_pixels"], n)
    changed = ((res["color"] != fr.base["color"]).any(axis=2) | (res["depth"] != fr.base["depth"])) & active
    assert changed.sum() >= 0.1 * n, (what, int(changed.sum()), n)


def check_render_occluded(gsm, torch, sc, cam, w, h, occ, fr, mw=None, mh=None, M=None, kind=None, opad=0):
    """One render_occluded against the checker's frame under `occ`; returns the checker's result."""
    mw, mh, M = mw or w, mh or h, M or max(sc.n, 1)
    r = handle(gsm, M, mw, mh, sc.prec)
    gc, gd = occluded_frame(gsm, torch, r, sc, cam, w, h, occ, opad)
    assert r.counters()["overflow"] == 0
    if kind is not None:
        assert r.blend_kernel_kind() == kind
    r.close()
    res = fr.occlude(occ)
    oc, od = ref_bytes(res, h)
    bad = np.argwhere(gc.reshape(h, w, 8) != oc.reshape(h, w, 8))
    assert len(bad) == 0, f"{len(bad)} colour bytes differ, first (y, x, byte) {bad[:4].tolist()}"
    bad = np.argwhere(gd.reshape(h, w, 2) != od.reshape(h, w, 2))
    assert len(bad) == 0, f"{len(bad)} depth bytes differ, first (y, x, byte) {bad[:4].tolist()}"
    return res


# ---- 0. declaration, export, binding (no GPU) ----
def test_occluded_entries_are_declared_exported_and_bound(gsm):
    import re
    import subprocess
    root = os.path.dirname(HERE)
    src = open(os.path.join(root, "include", "gsm_renderer.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    for name in ("gsm_global_render_occluded", "gsm_global_render_composite_occluded"):
        m = re.search(r"gsm_status\s+%s\s*\(([^;]*)\);" % name, src)
        assert m, name
        assert re.search(r"const\s+void\s*\*\s*occluder_r32f\s*,\s*size_t\s+occluder_pitch_bytes\s*$", m.group(1)), name
        assert f" T {name}\n" in out, name
        assert name in gsm._SIGNATURES
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    for name in ("render_occluded", "render_composite_occluded"):
        assert callable(getattr(gsm.GlobalRenderer, name, None)), name


# ---- 1. against the checker ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec,sh", [(1, 16), (0, 1)])
@pytest.mark.parametrize("w,h", [(320, 180), (203, 77)])
def test_render_occluded_matches_the_checker(gsm, cuda, prec, sh, w, h):
    """320x180: 12 tile rows, the last one partial.  203x77: an odd width that is no multiple of 32 -- the last pair
    of a row has px + 1 == W.  Occluder rows padded by 0, 1 and 3 floats: at 320 the pitch is a multiple of 8 bytes
    with no padding only, at 203 with 1 and 3 floats of it (8-byte loads of the limits there, 4-byte ones
    otherwise)."""
    from gsm_amd import scenes
    sc = gen(cuda, 4096, w, h, sh, prec, 3)
    cam = scenes.make_camera(w, h)
    with oracle_frame(sc, cam, w, h) as fr:
        assert fr.occlude(np.full((h, w), INF, np.float32))["differ"] == 0, "the checker's blend is not the oracle's"
        deps = visible_depths(fr.base)
        occluders = [("random", random_occluder(deps, w, h, 17)), ("ramp", ramp_occluder(deps, w, h)),
                     ("checkerboard", checker_occluder(w, h))]
        for name, occ in occluders:
            if name != "ramp":
                assert_not_vacuous(fr, fr.occlude(occ), name)
            for opad in (0, 1, 3):
                check_render_occluded(gsm, cuda, sc, cam, w, h, occ, fr, opad=opad)


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
    cam = scenes.make_camera(w, h)
    with oracle_frame(sc, cam, w, h, mw=mw, mh=mh) as fr:
        occ = random_occluder(visible_depths(fr.base), w, h, 23)
        res = check_render_occluded(gsm, cuda, sc, cam, w, h, occ, fr, mw=mw, mh=mh, kind=kind)
    assert res["closed_pixels"] > 0 and res["closure_breaks"] > 0 and res["mixed_groups"] > 0


# ---- 3. no occluder ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("fill", [np.inf, np.nan])
def test_an_occluder_that_occludes_nothing_gives_the_plain_frame(gsm, cuda, kind, fill):
    from gsm_amd import scenes
    w, h = 203, 77
    sc = gen(cuda, 4096, w, h, 1, 0, 5)
    cam = scenes.make_camera(w, h)
    mw, mh = (w, h) if kind == 1 else handle_size_for_tiles(8 * cus(cuda) + 1)
    ro = handle(gsm, sc.n, mw, mh, 0)
    gc, gd = occluded_frame(gsm, cuda, ro, sc, cam, w, h, np.full((h, w), fill, np.float32), opad=1)
    assert ro.blend_kernel_kind() == kind
    ro.close()
    rs = handle(gsm, sc.n, mw, mh, 0)
    pc, pd = plain_frame(gsm, cuda, rs, sc, cam, w, h)
    rs.close()
    assert np.array_equal(gc, pc) and np.array_equal(gd, pd)
    assert (gd != 0).any()


# ---- 4. a second derivation: the scene without what lies behind a constant surface ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_a_constant_surface_equals_the_scene_without_what_lies_behind_it(gsm, cuda, oracle, prec):
    """A constant occluder D removes, from every pixel's walk, exactly the gaussians with H(f2h(D)) < H(dep): on the
    tiles the filtered scene still lists, the frame is gsm_global_render of the filtered scene; on the tiles that
    became empty it holds colour 0, alpha +0, depth 0 (they are still active: the occluder culls nothing)."""
    from gsm_amd import scenes
    w, h = 320, 180
    sc = gen(cuda, 6000, w, h, 1, prec, 8)
    cam = scenes.make_camera(w, h)
    with oracle_frame(sc, cam, w, h) as fr:
        base = fr.base
    deps = visible_depths(base)
    listed = np.unique(base["sorted_values"][base["sorted_values"] >= 0])
    dep_all = base["records"][:, 9].view(np.float16).astype(np.float32)
    tiles = (np.arange(h)[:, None] // 16) * base["tiles_x"] + np.arange(w)[None, :] // 32
    for label, D in [("below near", np.float32(0.01)), ("q25", quantile(deps, 0.25)), ("q50", quantile(deps, 0.5)),
                     ("q75", quantile(deps, 0.75)), ("above all", np.float32(float(deps[-1]) * 2))]:
        Dh = np.float32(np.float16(D))
        behind = Dh < dep_all
        if label == "q50":
            assert behind[listed].sum() >= len(listed) / 4, "the test's premise: a quarter of the visible removed"
        keep = ~behind
        fs = Scene(cuda, sc.world_np[keep].copy(), sc.harm_np.reshape(sc.n, -1)[keep].copy().reshape(-1), sc.sh)
        ro = handle(gsm, sc.n, w, h, prec)
        gc, gd = occluded_frame(gsm, cuda, ro, sc, cam, w, h, np.full((h, w), D, np.float32))
        ro.close()
        rs = handle(gsm, sc.n, w, h, prec)
        pc, pd = plain_frame(gsm, cuda, rs, fs, cam, w, h)
        rs.close()
        fhead = oracle.render(fs.world_np, fs.harm_np, fs.sh, cam, w, h, max_gaussians=sc.n)["headers"] \
            if fs.n else np.zeros_like(base["headers"])
        still = (fhead[:, 1] > 0)[tiles]
        emptied = (base["headers"][:, 1] > 0)[tiles] & ~still
        gc4, pc4 = gc.view(np.uint16).reshape(h, w, 4), pc.view(np.uint16).reshape(h, w, 4)
        gd1, pd1 = gd.view(np.uint16).reshape(h, w), pd.view(np.uint16).reshape(h, w)
        assert np.array_equal(gc4[still], pc4[still]) and np.array_equal(gd1[still], pd1[still]), label
        assert (gc4[emptied] == 0).all() and (gd1[emptied] == 0).all(), label
        if label == "below near":
            assert emptied.any() and not still.any()
        if label == "above all":
            assert not emptied.any()


# ---- 5. long walks ----
LONG = dict(n=8192, w=64, h=32, spread=0.5, scale_px=1.2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("prec", [0, 1])
def test_long_walks_are_cut_in_every_batch_position(gsm, cuda, kind, prec):
    """Opacities of [0.02, 0.05] on 8192 small gaussians over 64x32: nothing saturates, the tile lists run to
    hundreds of entries, and the walk's four-batch pipeline (256 entries deep) turns over more than once.  The
    surface moves through the stack: every 4x2 group gets one of 64 quantiles of the depths, a quarter of the
    pixels one of their own.  The conditions on the input, from the checker: groups walk past 256 entries, and
    groups end at their surface in every quarter of the 256-entry cycle."""
    from gsm_amd import scenes
    w, h = LONG["w"], LONG["h"]
    sc = gen(cuda, LONG["n"], w, h, 1, prec, 21, opacity=(0.02, 0.05), spread=LONG["spread"],
             scale_px=LONG["scale_px"])
    cam = scenes.make_camera(w, h)
    mw, mh = (64, 32) if kind == 1 else handle_size_for_tiles(8 * cus(cuda) + 1)
    with oracle_frame(sc, cam, w, h, M=4 * sc.n, mw=mw, mh=mh) as fr:
        deps = visible_depths(fr.base)
        rng = np.random.default_rng(31)
        qv = np.array([quantile(deps, (i + 0.5) / 64) for i in range(64)], np.float32)
        occ = np.kron(qv[rng.integers(0, 64, (h // 2, w // 4))], np.ones((2, 4), np.float32)).astype(np.float32)
        own = rng.random((h, w)) < 0.25
        occ[own] = qv[rng.integers(0, 64, int(own.sum()))]
        res = check_render_occluded(gsm, cuda, sc, cam, w, h, occ, fr, mw=mw, mh=mh, M=4 * sc.n, kind=kind)
        counts = fr.base["headers"][:, 1]
    iters = res["group_iters"]
    cut = iters[iters < counts[:, None, None]]
    assert iters.max() > 256, "the test's premise: a walk longer than the pipeline is deep"
    assert res["closure_breaks"] > 0 and (cut >= 256).any()
    assert (np.histogram(cut % 256, bins=4, range=(0, 256))[0] > 0).all(), "cuts in every batch position"


# ---- 6. the exact rewalk ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("prec", [0, 1])
def test_units_walked_again_exactly_are_cut_as_well(gsm, cuda, prec, kind):
    """Records of inf fp16 depth: every unit that stages one is walked again by walk_unit_exact, which rewrites all
    of its pixels.  A finite surface stands in front of those records on a random half of the pixels (behind every
    ordinary gaussian on half of these, among them on the other half); +inf elsewhere.  The conditions on the
    input, from the checker: such records are listed, they still leave inf and NaN depth pixels, and the surface
    changes pixels."""
    w, h = 320, 180
    sc, cam, far = far_scene(cuda, prec)
    mw, mh = (w, h) if kind == 1 else handle_size_for_tiles(8 * cus(cuda) + 1)
    with oracle_frame(sc, cam, w, h, M=4 * sc.n, mw=mw, mh=mh) as fr:
        base = fr.base
        listed = np.unique(base["sorted_values"][base["sorted_values"] >= 0])
        assert ((base["records"][listed, 9] & 0x7C00) == 0x7C00).any(), "the test's premise: a listed record of inf depth"
        deps = visible_depths(base)
        finite = deps[np.isfinite(deps)]
        # 65519 is the largest float that rounds to a finite fp16 (65504: in front of an inf record), 65520 the
        # smallest that rounds to +inf (occludes nothing); 6e-8 and 3e-8 round to the smallest fp16 denormal and
        # to +0, 6.1e-5 lies just above the largest denormal (all three close every pixel they sit on)
        palette = np.array([np.inf, np.inf, np.inf, 6.0e4, 6.0e4, quantile(finite, 0.5), quantile(finite, 0.5),
                            65519.0, 65520.0, 6e-8, 3e-8, 6.1e-5], np.float32)
        occ = palette[np.random.default_rng(41).integers(0, len(palette), (h, w))]
        res = check_render_occluded(gsm, cuda, sc, cam, w, h, occ, fr, mw=mw, mh=mh, M=4 * sc.n, kind=kind)
    dep = res["depth"].view(np.float16)
    assert np.isinf(dep).any() and np.isnan(dep).any()
    plain_dep = base["depth"].view(np.float16)
    assert (np.isinf(plain_dep) & np.isfinite(dep) & (occ == np.float32(6.0e4))).any(), \
        "a surface in front of an inf-depth record alone changed a pixel"
    assert (np.isinf(plain_dep) & np.isfinite(dep) & (occ == np.float32(65519.0))).any(), \
        "65519 rounds to 65504 and stands in front of an inf-depth record"
    at_inf = occ == np.float32(65520.0)
    assert (np.isinf(plain_dep) & at_inf).any() and np.array_equal(dep.view(np.uint16)[at_inf & np.isinf(plain_dep)],
                                                                   plain_dep.view(np.uint16)[at_inf & np.isinf(plain_dep)])
    assert res["closed_pixels"] > 0 and res["mixed_groups"] > 0


# ---- 6b. dense scenes: entries that a half-tile list drops close pixels ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec,seed,kind", [(0, 102, 1), (1, 100, 2), (0, 102, 2)])
def test_dense_scenes_where_dropped_entries_close_pixels(gsm, cuda, prec, seed, kind):
    """20 000 gaussians at 320x180: tile lists of several hundred entries, about half of them with alpha 0 on a
    whole 16-column half of their tile -- the entries the plain frame's half-tile lists leave out.  Under the
    contract such an entry still closes the pixels whose surface lies before it, and the break of the entries
    after it sees them closed; a walk over the half lists would close them one kept entry later and blend that
    entry into the group's nearly saturated open pixels.  The condition on the input, from the checker: the frame
    of that wrong model (occlude_ref.c, half_model) differs from the contract's on this scene, so a frame equal
    to the contract's cannot come from the half lists."""
    from gsm_amd import scenes
    w, h = 320, 180
    sc = gen(cuda, 20_000, w, h, 1, prec, seed)
    cam = scenes.make_camera(w, h)
    mw, mh = (w, h) if kind == 1 else handle_size_for_tiles(8 * cus(cuda) + 1)
    with oracle_frame(sc, cam, w, h, mw=mw, mh=mh) as fr:
        occ = random_occluder(visible_depths(fr.base), w, h, 17)
        res = check_render_occluded(gsm, cuda, sc, cam, w, h, occ, fr, mw=mw, mh=mh, kind=kind)
        wrong = fr.occlude(occ, half_model=True)
        assert fr.occlude(np.full((h, w), INF, np.float32), half_model=True)["differ"] == 0, \
            "the model drops only entries that change nothing without an occluder"
    told_apart = (res["color"] != wrong["color"]).any(axis=2) | (res["depth"] != wrong["depth"])
    assert told_apart.sum() >= 3, "the test's premise: pixels that tell the tile's whole list from its half lists"
    assert res["closure_breaks"] > 0 and res["mixed_groups"] > 0


# ---- 7. the composite ----
def composite_occluded(gsm, torch, r, pairs, w, h, occ, opad=0):
    t = Targets(torch, w, h, occ, opad)
    objs = [gsm.SceneObject(s.input(gsm), gsm.CameraParams.from_dict(c)) for s, c in pairs]
    r.render_composite_occluded(t.color, t.depth, t.occ, objs, w, h, color_pitch=t.color_pitch,
                                depth_pitch=t.depth_pitch, occluder_pitch=t.occ_pitch)
    return t.read()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_composite_occluded_matches_the_checker(gsm, cuda, prec):
    """Counts 300, 0, 1000, 257 -- no multiple of 256, an empty object in between -- under three distinct poses."""
    import occlude_ref
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
    with occlude_ref.frame_composite([(s.world_np, s.harm_np, c) for s, c in pairs], 4, w, h,
                                     max_gaussians=M_) as fr:
        assert fr.base["overflow"] == 0 and fr.base["total_assignments"] > 0
        assert fr.occlude(np.full((h, w), INF, np.float32))["differ"] == 0
        occ = random_occluder(visible_depths(fr.base), w, h, 43)
        res = fr.occlude(occ)
    assert res["closed_pixels"] > 0 and res["mixed_groups"] > 0
    r = handle(gsm, M_, w, h, prec)
    gc, gd = composite_occluded(gsm, cuda, r, pairs, w, h, occ, opad=1)
    assert r.counters()["overflow"] == 0
    r.close()
    oc, od = ref_bytes(res, h)
    assert np.array_equal(gc, oc) and np.array_equal(gd, od)


@pytest.mark.gpu
def test_composite_occluded_under_one_camera_is_render_occluded_of_the_concatenation(gsm, cuda):
    from gsm_amd import scenes
    w, h = 203, 77
    counts = (300, 0, 1000, 257)
    scs = [gen(cuda, n, w, h, 1, 0, 40 + i) for i, n in enumerate(counts)]
    cam = scenes.make_camera(w, h)
    M_ = sum(roundup256(n) for n in counts)
    cat = Scene(cuda, np.concatenate([s.world_np for s in scs]), np.concatenate([s.harm_np for s in scs]), 1)
    with oracle_frame(cat, cam, w, h, M=M_) as fr:
        occ = random_occluder(visible_depths(fr.base), w, h, 47)
        res = fr.occlude(occ)
    rp = handle(gsm, M_, w, h, 0)
    gc, gd = composite_occluded(gsm, cuda, rp, [(s, cam) for s in scs], w, h, occ)
    rp.close()
    rs = handle(gsm, M_, w, h, 0)
    sc_, sd_ = occluded_frame(gsm, cuda, rs, cat, cam, w, h, occ)
    rs.close()
    assert np.array_equal(gc, sc_) and np.array_equal(gd, sd_)
    oc, od = ref_bytes(res, h)
    assert np.array_equal(gc, oc) and np.array_equal(gd, od) and res["closed_pixels"] > 0


# ---- 8. empty frames, state, refusals ----
@pytest.mark.gpu
def test_empty_frames_hold_the_clear_value(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    A = gen(None, 4, w, h, 1, 0, 50)
    E = Scene(cuda, A.world_np[:0].copy(), A.harm_np[:0].copy(), 1)
    cam = scenes.make_camera(w, h)
    clear = np.zeros((h, w, 4), np.uint16)
    clear[..., 3] = 0x3C00
    occ = np.full((h, w), 0.01, np.float32)
    r = handle(gsm, 256, w, h, 0)
    for frame in (lambda: occluded_frame(gsm, cuda, r, E, cam, w, h, occ),
                  lambda: composite_occluded(gsm, cuda, r, [(E, cam), (E, cam)], w, h, occ)):
        gc, gd = frame()
        assert np.array_equal(gc, clear.view(np.uint8).reshape(h, -1)) and (gd == 0).all()
    r.close()


@pytest.mark.gpu
def test_occluded_and_plain_frames_share_a_handle_and_replay(gsm, cuda):
    """occluded, plain, occluded with three scenes on one handle, twice (the second round meets the first's
    schedule), then the same three frames replayed from a captured graph: each equals the frame of a fresh handle."""
    from gsm_amd import scenes
    w, h = 203, 77
    scs = [gen(cuda, n, w, h, 1, 0, 60 + i) for i, n in enumerate((3000, 2000, 4000))]
    cams = [scenes.orbit_camera(w, h, a) for a in (0.0, 7.0, -5.0)]
    M_ = 4096
    occs, fresh = [], []
    for i, (sc, cam) in enumerate(zip(scs, cams)):
        with oracle_frame(sc, cam, w, h, M=M_) as fr:
            occ = random_occluder(visible_depths(fr.base), w, h, 80 + i)
            want = ref_bytes(fr.base if i == 1 else fr.occlude(occ), h)
        occs.append(occ)
        r = handle(gsm, M_, w, h, 0)
        fresh.append(plain_frame(gsm, cuda, r, sc, cam, w, h) if i == 1
                     else occluded_frame(gsm, cuda, r, sc, cam, w, h, occ))
        r.close()
        assert np.array_equal(fresh[i][0], want[0]) and np.array_equal(fresh[i][1], want[1]), "the yardstick"

    def same(a, b):
        return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))

    r = handle(gsm, M_, w, h, 0)
    for _ in range(2):
        assert same(occluded_frame(gsm, cuda, r, scs[0], cams[0], w, h, occs[0]), fresh[0])
        assert same(plain_frame(gsm, cuda, r, scs[1], cams[1], w, h), fresh[1])
        assert same(occluded_frame(gsm, cuda, r, scs[2], cams[2], w, h, occs[2]), fresh[2])
    # captured and replayed
    ts = [Targets(cuda, w, h, None if i == 1 else occs[i]) for i in range(3)]
    cps = [gsm.CameraParams.from_dict(c) for c in cams]
    s = cuda.cuda.Stream()
    cuda.cuda.synchronize()
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        for i, t in enumerate(ts):
            if i == 1:
                r.render(t.color, t.depth, scs[i].input(gsm), cps[i], w, h, stream=s, color_pitch=t.color_pitch,
                         depth_pitch=t.depth_pitch)
            else:
                r.render_occluded(t.color, t.depth, t.occ, scs[i].input(gsm), cps[i], w, h, stream=s,
                                  color_pitch=t.color_pitch, depth_pitch=t.depth_pitch, occluder_pitch=t.occ_pitch)
    cuda.cuda.synchronize()
    for _ in range(2):
        for t in ts:
            t.refill()
        g.replay()
        got = [t.read() for t in ts]
        assert all(same(got[i], fresh[i]) for i in range(3))
    r.close()


@pytest.mark.gpu
def test_refusals_enqueue_nothing(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    A, B = gen(cuda, 300, w, h, 1, 0, 70), gen(cuda, 500, w, h, 1, 0, 71)
    cam = gsm.CameraParams.from_dict(scenes.make_camera(w, h))
    r = handle(gsm, 1024, w, h, 0)
    t = Targets(cuda, w, h, np.full((h, w), 4.0, np.float32), pad=0)
    objs = [gsm.SceneObject(A.input(gsm), cam), gsm.SceneObject(B.input(gsm), cam)]
    UNSET = object()

    def status(composite, occ=UNSET, color=UNSET, **kw):
        occ = t.occ if occ is UNSET else occ
        color = t.color if color is UNSET else color
        try:
            if composite:
                r.render_composite_occluded(color, t.depth, occ, objs, w, h, **kw)
            else:
                r.render_occluded(color, t.depth, occ, A.input(gsm), cam, w, h, **kw)
        except gsm.RendererError as e:
            return int(e.status)
        return 0

    for comp in (False, True):
        assert status(comp, occ=None) == ERR_MISSING
        assert status(comp, occluder_pitch=4 * w - 4) == ERR_SIZE
        assert status(comp, occluder_pitch=4 * w + 2) == ERR_SIZE
        assert status(comp, occ=int(t.occ.data_ptr()) + 2) == ERR_SIZE
        # the plain entry's order: a missing buffer before a size, colour's size with the occluder's
        assert status(comp, occ=None, color_pitch=8 * w - 4) == ERR_MISSING
        assert status(comp, color=None, occluder_pitch=4 * w - 4) == ERR_MISSING
        assert status(comp, color_pitch=8 * w - 4) == ERR_SIZE
        r.set_tile_rows(1, 2)
        assert status(comp) == ERR_UNSUPPORTED
        assert status(comp, occluder_pitch=4 * w - 4) == ERR_SIZE, "the size before the tile rows"
        r.set_tile_rows(0, 0)
    assert t.untouched(), "a refused call wrote"
    assert status(False) == 0 and status(True) == 0
    c, d = t.read()
    assert (d != 0).any()
    r.close()
