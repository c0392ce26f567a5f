"""The checkers of the composite, pick, occluded, styled and all-options frames and of the selects against the
float64 model (tests/f64_model.py): CPU only.

tests/{compose,pick,occlude,style,frame}/*_ref.c restate the project's own contract and were
written with the kernels they check; the reference has none of these features.  Here they are held to a second
derivation that takes a pose from the model matrix (not from scenes.object_camera), the occluder, the pick and
the styles from the contract's sentences, with the checks, helpers and constants of tests/test_f64_model.py.
tests/test_f64_features_gpu.py applies the same functions to what the HIP path returns.

PICK_TOL is twice the largest model-weight deficit of a checker's pick over the scenes below.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_model as M  # noqa: E402
import test_f64_model as T  # noqa: E402

NONE = 0xFFFFFFFF
# the largest amount by which the model weight (alpha * T_before, float64) of a checker's pick falls short of the
# pixel's largest model weight; the checkers compare fp16 products.  Constant = 2 x the measured maximum.
PICK_TOL = {
    # measured: 7.85e-4 (sparse_sh1_f16_200x150: pick_ref on the plain frame, frame_ref under every occluder)
    "sparse": 1.57e-3,
    # measured: 3.26e-4 (dense_sh0_f32_128x64: pick_ref on the plain frame, frame_ref under the tile-step occluder)
    "dense": 6.5e-4,
}
MIN_CLEAR_SHARE = 0.75  # of the picked pixels, the share whose runner-up is more than 2 PICK_TOL below the winner


# ---- scenes ------------------------------------------------------------------------------------------------
def pose(axis, degrees, translate=(0.0, 0.0, 0.0), scale=1.0, pivot=(0.0, 0.0, 5.5)):
    """T(pivot + translate) S(scale) R(axis, degrees) T(-pivot), column-major flat (object -> world)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(degrees)
    R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    m = np.eye(4)
    m[:3, :3] = scale * R
    p = np.asarray(pivot, np.float64)
    m[:3, 3] = p + np.asarray(translate, np.float64) - scale * R @ p
    return m.T.reshape(-1)


IDENTITY = np.eye(4).reshape(-1)
# name: (width, height, SH components, precision, [(gaussians, seed, model matrix)])
COMPOSITES = {
    # an object under a rotation about an oblique axis with a translation, an empty object, an object under a
    # similarity of scale 1.25, and one gaussian (an object shorter than a block) at the identity
    "composite_3_sh1_f16_200x150": (200, 150, 4, 1, [
        (700, 41, pose((1.0, 2.0, 0.5), 25.0, (0.3, -0.2, 0.4))),
        (0, 0, IDENTITY),
        (300, 42, pose((0.3, -1.0, 0.4), -35.0, (-0.2, 0.1, -0.3), scale=1.25)),
        (1, 43, IDENTITY)]),
    # the second object turned by a quarter: SH directions taken in the wrong frame move its colours
    "composite_2_sh3_f32_128x64": (128, 64, 16, 0, [
        (250, 44, IDENTITY),
        (200, 45, pose((0.2, 0.3, 1.0), 90.0))]),
}
SINGLES = ["sparse_sh1_f16_200x150", "dense_sh0_f32_128x64", "plane_ties_128x64", "opaque_splat_64x64"]
# scenes only the GPU tests use: the 200x150 view of a batch whose other views are f32 SH0 (one batch, one layout),
# and test_render_pick's LONG scene (lists deeper than the walk's 256-entry pipeline)
EXTRA = {
    "sparse_sh0_f32_200x150": ("gen", 2000, 200, 150, 1, 0, 0, 11, None, {}),
    "small_sh0_f32_64x64": ("gen", 300, 64, 64, 1, 0, 0, 18, None, {}),
    "long_sh0_f32_64x32": ("gen", 8192, 64, 32, 1, 0, 0, 21, None, {"spread": 0.5, "scale_px": 1.2}),
}

# the style table of the styled tests: (tint r, g, b, amount, opacity scale, hidden)
STYLES = [(0, 0, 0, 0, 255, 0), (255, 40, 10, 255, 255, 0), (20, 200, 90, 128, 255, 0), (0, 0, 0, 0, 0, 0),
          (0, 0, 0, 0, 128, 0), (0, 0, 0, 0, 255, 1)]


def states_for(n, seed):
    """States over the 6-entry table, a tenth of them at or above style_count (6 .. 255: the identity)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, len(STYLES), n).astype(np.uint8)
    high = rng.random(n) < 0.1
    s[high] = rng.integers(len(STYLES), 256, int(high.sum())).astype(np.uint8)
    return s


@functools.lru_cache(maxsize=None)
def case_of(name):
    """objects [(world, harmonics, model matrix)] under one frame camera."""
    from gsm_amd import scenes
    if name in COMPOSITES:
        w, h, sh, prec, objs = COMPOSITES[name]
        objects = []
        for n, seed, model in objs:
            world, harm, _ = scenes.gen_scene(max(n, 1), w, h, sh, prec, seed=seed)
            if n == 1:  # on the axis, among the nearer gaussians of the other two: listed between them, and picked
                world["px"], world["py"], world["pz"] = 0.0, 0.0, 3.0
            objects.append((world[:n], np.asarray(harm).reshape(max(n, 1), -1)[:n].reshape(-1), model))
        # a frame camera that is not the identity: view * M and M * view are then different matrices
        return dict(objects=objects, sh=sh, cam=scenes.orbit_camera(w, h, 20.0), width=w, height=h, color_space=0)
    c = T.make_case(EXTRA[name]) if name in EXTRA else T.case_of(name)
    if name.startswith("long"):  # opacities of [0.02, 0.05]: nothing saturates (tests/test_render_pick.py, gen)
        op = np.random.default_rng(EXTRA[name][7] + 1).uniform(0.02, 0.05, len(c["world"])).astype(np.float32)
        c["world"]["opacity"] = op
    return dict(objects=[(c["world"], c["harm"], None)], sh=c["sh"], cam=c["cam"], width=c["width"],
                height=c["height"], color_space=c["color_space"])


def counts_of(case):
    return [len(o[0]) for o in case["objects"]]


@functools.lru_cache(maxsize=None)
def projection_of(name):
    """(model projection indexed by item, owner [items, 2]); a single scene keeps its n entries."""
    c = case_of(name)
    pr, _, owner = M.project_composite(c["objects"], c["sh"], c["cam"], c["width"], c["height"], c["color_space"])
    if len(c["objects"]) == 1:
        n = len(c["objects"][0][0])
        pr = {k: ({m: v[:n] for m, v in val.items()} if k == "margins" else val[:n]) for k, val in pr.items()}
        owner = owner[:n]
    return pr, owner


def styled_projection(name, states, styles=STYLES):
    pr, owner = projection_of(name)
    return M.apply_styles(pr, item_states(case_of(name), states, len(owner)), styles), owner


def item_states(case, states, items):
    """Per-object states (arrays or ints) laid out by item."""
    base, _ = M.item_layout(counts_of(case))
    out = np.zeros(items, np.uint8)
    for b, n, s in zip(base, counts_of(case), states):
        out[b:b + n] = s
    return out


# ---- occluders, from the model's depths ------------------------------------------------------------------------
def model_depths(pr):
    return np.sort(M.round_h(pr["depth"][pr["visible"]]))


def ramp_occluder(pr, w, h):
    """A horizontal ramp from the near plane's side of every depth to past the farthest."""
    d = model_depths(pr)
    return np.broadcast_to(np.linspace(0.05, float(d[-1]) * 1.05, w, dtype=np.float32), (h, w)).copy()


def step_occluder(pr, w, h, seed):
    """One random quantile of the scene's depths per 32x16 tile; about a tile in eight lies in front of them all."""
    d = model_depths(pr)
    rng = np.random.default_rng(seed)
    q = rng.uniform(-0.12, 0.9, ((h + 15) // 16, (w + 31) // 32))
    z = np.where(q < 0, 0.05, d[(np.maximum(q, 0) * (len(d) - 1)).astype(int)])
    return np.repeat(np.repeat(z, 16, 0), 32, 1)[:h, :w].astype(np.float32)


def special_occluder(pr, w, h, seed):
    """The ramp with a quarter of its pixels replaced by +inf, NaN, 0 and a value below the near plane."""
    occ = ramp_occluder(pr, w, h)
    rng = np.random.default_rng(seed)
    hit = rng.random((h, w)) < 0.25
    occ[hit] = np.array([np.inf, np.nan, 0.0, 0.01], np.float32)[rng.integers(0, 4, int(hit.sum()))]
    return occ


def occluder_of(name, kind):
    pr, _ = projection_of(name)
    c = case_of(name)
    w, h = c["width"], c["height"]
    return {"ramp": lambda: ramp_occluder(pr, w, h), "step": lambda: step_occluder(pr, w, h, 7),
            "special": lambda: special_occluder(pr, w, h, 8)}[kind]()


# ---- views: what a checker or the HIP path returned, indexed by item ---------------------------------------------
def feature_view(case, render_data, mask, headers, sorted_values, color_bits, depth_bits, pick=None):
    """T.global_view of item-indexed arrays, plus 'pick' [h, w] int64 (items; -1 for none)."""
    v = T.global_view(render_data, mask, headers, sorted_values, color_bits, depth_bits)
    if pick is not None:
        p = np.asarray(pick).astype(np.int64)
        v["pick"] = np.where(p == NONE, M.PICK_NONE, p)
    return v


def _checker_objects(case, states=None):
    from gsm_amd import scenes
    out = []
    for i, (world, harm, model) in enumerate(case["objects"]):
        cam = case["cam"] if model is None else scenes.object_camera(case["cam"], model)
        out.append((world, harm, cam) if states is None else (world, harm, cam, states[i]))
    return out


def _to_items(case, r, color, depth, pick):
    """A checker's dictionary (concatenated ids) as an item-indexed view."""
    counts = counts_of(case)
    base, items = M.item_layout(counts)
    if len(counts) == 1:
        items = counts[0]
    idx = np.concatenate([b + np.arange(n) for b, n in zip(base, counts)]).astype(np.int64)
    rd = np.zeros(items, r["render_data"].dtype)
    rd[idx] = r["render_data"]
    mask = np.zeros(items, bool)
    mask[idx] = r["mask"] != 0
    p = None
    if pick is not None:
        p = np.asarray(pick).astype(np.int64)
        p = np.where(p == NONE, NONE, idx[np.minimum(p, len(idx) - 1)])
    return feature_view(case, rd, mask, r["headers"], idx[r["sorted_values"]], color, depth, p)


def checker_view(name, occ=None, states=None, styles=None):
    """The checkers' frame: style_ref (its records, lists and pick_ref's pick) and, under an occluder, frame_ref's
    walk of the same frame (colour, depth, pick)."""
    import frame_ref
    import style_ref
    c = case_of(name)
    st = [0] * len(c["objects"]) if states is None else states
    table = style_ref.style_table([M.IDENTITY_STYLE] if styles is None else styles)
    objs = _checker_objects(c, st)
    r = style_ref.render_composite(objs, c["sh"], c["width"], c["height"], table, color_space=c["color_space"])
    assert r["status"] == 0 and r["overflow"] == 0 and r["differ"] == 0
    color, depth, pick = r["color"], r["depth"], r["pick"]
    if occ is not None:
        with frame_ref.frame(objs, c["sh"], c["width"], c["height"], styles=table,
                             color_space=c["color_space"]) as fr:
            res = fr.walk(occ)
        color, depth, pick = res["color"], res["depth"], res["pick"]
    return _to_items(c, r, color, depth, pick)


# ---- checks (shared with tests/test_f64_features_gpu.py) --------------------------------------------------------
def measure_pick(view, w, h, occ=None):
    """The model's weights on the view's own records and lists against its pick image.  Returns a dict of
    figures and arrays; asserts the exact part: a picked item is a live, unoccluded entry of its pixel's list."""
    tw, th = view["rules"]["tile"]
    m = M.blend_lists(view["rec"], view["lists"], tw, th, w, h, view["clear"], view["rules"], occluder=occ,
                      pick=True, pick_query=view["pick"])
    has = view["pick"] >= 0
    bad = np.argwhere(has & ~m["query_open"])
    assert len(bad) == 0, (f"{len(bad)} picked items are no live, unoccluded entry of their pixel's list, first "
                           f"(y, x) {bad[:4].tolist()}: items {view['pick'][tuple(bad[:4].T)].tolist()}")
    deficit = float((m["pick_weight"] - m["query_weight"])[has].max(initial=0.0))
    missed = float(m["pick_weight"][~has].max(initial=0.0))
    return dict(model=m, has=has, deficit=deficit, missed=missed)


def check_pick(view, w, h, occ=None, what=""):
    tol = PICK_TOL[T.regime(view)]
    f = measure_pick(view, w, h, occ)
    m, has = f["model"], f["has"]
    clear = has & (m["pick_weight"] - m["pick_second"] > 2.0 * tol)
    share = float(clear.sum()) / max(int(has.sum()), 1)
    print(f"pick {what} ({T.regime(view)}): {int(has.sum())} picked, deficit {f['deficit']:.3g}, largest weight of a "
          f"'none' {f['missed']:.3g} (bound {tol}), {share:.1%} clear winners")
    assert has.any() and f["deficit"] <= tol, (f["deficit"], tol)
    assert f["missed"] <= tol, (f["missed"], tol)
    assert share >= MIN_CLEAR_SHARE, f"the scene's premise: {share:.1%} of the picks are clear winners"
    bad = np.argwhere(clear & (view["pick"] != m["pick"]))
    assert len(bad) == 0, (f"{len(bad)} clear winners are not picked, first (y, x) {bad[:4].tolist()}: picked "
                           f"{view['pick'][tuple(bad[:4].T)].tolist()}, model {m['pick'][tuple(bad[:4].T)].tolist()}")
    return f


def check_frame(name, view, pr, owner, occ=None, whole=True, pick=False, what=""):
    """Visibility, records, order, compositing on the view's lists and the whole frame from the model alone; the
    pick by weight.  Returns the model's whole frame (or None)."""
    c = case_of(name)
    w, h = c["width"], c["height"]
    view["mask"] = view["mask"] & (owner[:, 0] >= 0)  # entries of no gaussian are unspecified
    T.check_visibility(pr, view["mask"])
    T.check_records(pr, view, w, h)
    T.check_order(pr, view, owner)
    listed = np.unique(np.concatenate([ids for _, ids in view["lists"]] + [np.zeros(0, np.int64)])).astype(np.int64)
    assert pr["visible"][listed][~T.left_out(pr)[listed]].all(), "a list names a gaussian the model culls or hides"
    if "no_tiles" in pr:
        assert pr["no_tiles"].any() and not pr["no_tiles"][listed].any(), "a styled opacity byte of 0 has no tiles"
        assert view["mask"][pr["no_tiles"] & ~T.left_out(pr)].all(), "... and stays visible"
    T.check_blend("lists", T.measure_lists(view, w, h, occluder=occ), view)
    out = None
    if whole:
        out = {}
        T.check_blend("frame", T.measure_frame(pr, view, w, h, occluder=occ, model_out=out), view)
    if pick:
        check_pick(view, w, h, occ, what)
    return out


def assert_occluder_not_vacuous(model, what):
    """From the model's whole frame alone: the compared pixels hold open and closed ones, pixels closed before
    their first entry and pixels closed in mid-list."""
    where = model["where"]
    n = int(where.sum())
    closed, first = model["cut_any"] & where, model["cut_first"] & where
    opened = model["drawn_any"] & ~model["cut_any"] & where
    mid = model["cut_any"] & model["drawn_any"] & ~model["cut_first"] & where
    print(f"occluder {what}: of {n} pixels (entries of alpha >= 1/255) {int(opened.sum())} open, {int(closed.sum())} "
          f"closed, {int(first.sum())} before the first entry, {int(mid.sum())} in mid-list")
    assert closed.sum() >= 0.1 * n and opened.sum() >= 0.1 * n, what
    assert first.sum() >= 0.02 * n and mid.sum() >= 0.05 * n, what


def interleaved_tiles(view, owner):
    """Tiles whose list holds an entry of each of three objects before and after an entry of another object."""
    found = []
    for t, ids in view["lists"]:
        obj = owner[ids, 0]
        if len(np.unique(obj)) < 3:
            continue
        runs = 1 + int((obj[1:] != obj[:-1]).sum())
        if runs >= 6:  # three objects in order would be three runs
            found.append(t)
    return found


def check_select(name, got_states, got_count, before, model_states, model_count, doubt, what):
    """States equal the model's outside the in-doubt set, the count within the in-doubt count, unmatched bytes
    unchanged, the in-doubt set small."""
    n = len(before)
    sure = ~doubt[:n]
    print(f"select {what}: matched {got_count} (model {model_count}), {int(doubt.sum())} in doubt")
    assert doubt.sum() <= T.MAX_LEFT_OUT * n
    bad = np.nonzero((got_states != model_states) & sure)[0]
    assert bad.size == 0, f"{what}: {bad.size} states differ from the model's, first {bad[:5].tolist()}"
    assert abs(got_count - model_count) <= int(doubt.sum()), (what, got_count, model_count)
    same = (model_states == before) & sure
    assert np.array_equal(got_states[same], before[same])


# ---- 0. the scenes' premises -------------------------------------------------------------------------------------
ALL = SINGLES + sorted(COMPOSITES)


@pytest.fixture(scope="module")
def refs(oracle):
    import style_ref
    style_ref.lib()
    return True


def test_scene_regimes(refs):
    depths = {s: T.deepest(checker_view(s)) for s in ALL}
    print(depths)
    assert all(d <= T.SPARSE_MAX or d >= T.DENSE_MIN for d in depths.values()), depths
    assert depths["dense_sh0_f32_128x64"] >= T.DENSE_MIN


def test_pose_is_not_the_reference_scene_transform():
    """project(pose=True) against the two readings it must tell apart, from the model alone: the DepthFirst scene
    transform (covariance not turned) and SH directions taken from the frame camera's own position."""
    c = case_of("composite_2_sh3_f32_128x64")
    world, harm, model = c["objects"][1]
    args = (world, harm, c["sh"], c["cam"], c["width"], c["height"])
    right = M.project(*args, scene_transform=model, pose=True)
    wrong_sh = M.project(*args, scene_transform=model, pose=True, sh_center=c["cam"]["position"])
    moved = np.abs(right["color"] - wrong_sh["color"]).max(1)
    print(f"SH frame: {int((moved > 0.05).sum())} of {len(world)} colours differ by more than 0.05")
    assert (moved[right["visible"]] > 0.05).sum() >= 100
    unturned = M.project(*args, scene_transform=model)
    assert np.abs(right["theta"] - unturned["theta"])[right["visible"]].max() > 0.5
    assert np.allclose(right["mean"], unturned["mean"], equal_nan=True)


# ---- 1. the composite ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COMPOSITES))
def test_composite(refs, name):
    """compose_ref's frame (its own entry, not the styled checker's) under the model."""
    import compose_ref
    c = case_of(name)
    pr, owner = projection_of(name)
    r = compose_ref.render(_checker_objects(c), c["sh"], c["width"], c["height"], color_space=c["color_space"])
    assert r["status"] == 0 and r["overflow"] == 0
    v = _to_items(c, r, r["color"], r["depth"], None)
    check_frame(name, v, pr, owner)
    if len(c["objects"]) > 2:
        tiles = interleaved_tiles(v, owner)
        print(f"{len(tiles)} tiles interleave three objects")
        assert tiles, "the scene's premise: some list interleaves all three objects"
        # from the model: the whole-frame order interleaves them too
        vis = np.nonzero(pr["visible"])[0]
        order = owner[M.depth_order(M.round_h(pr["depth"]), vis), 0]
        assert 1 + int((order[1:] != order[:-1]).sum()) >= 6


# ---- 2. the occluder, 3. equality at the surface, 6. the flag against the comparison ---------------------------------
OCCLUDED = ["sparse_sh1_f16_200x150", "dense_sh0_f32_128x64", "composite_3_sh1_f16_200x150"]


@pytest.mark.parametrize("kind", ["ramp", "step", "special"])
@pytest.mark.parametrize("name", OCCLUDED)
def test_occluded(refs, name, kind):
    pr, owner = projection_of(name)
    occ = occluder_of(name, kind)
    v = checker_view(name, occ=occ)
    model = check_frame(name, v, pr, owner, occ=occ, pick=True, what=f"{name} {kind}")
    assert_occluder_not_vacuous(model, f"{name} {kind}")


def test_occlude_ref_agrees_with_frame_ref(refs):
    """The occluded entries' own checker gives the bytes the all-options checker gives (so the model holds both)."""
    import occlude_ref
    name = "sparse_sh1_f16_200x150"
    c = case_of(name)
    occ = occluder_of(name, "special")
    v = checker_view(name, occ=occ)
    world, harm, _ = c["objects"][0]
    with occlude_ref.frame(world, harm, c["sh"], c["cam"], c["width"], c["height"]) as fr:
        res = fr.occlude(occ)
    assert np.array_equal(M.h2d(res["color"])[..., :3], v["color"]) and np.array_equal(M.h2d(res["depth"]), v["depth"])


def test_a_splat_at_the_surface_is_drawn(refs):
    """An occluder equal, bit for bit, to the splat's fp16 depth draws it; one fp16 step below draws none of it."""
    name = "opaque_splat_64x64"
    c = case_of(name)
    w, h = c["width"], c["height"]
    pr, owner = projection_of(name)
    plain = checker_view(name)
    z = np.float16(plain["rec"]["depth"][0])
    assert float(z) == plain["rec"]["depth"][0] == M.round_h(pr["depth"][0])
    q = M.quantise_global(pr)
    order = M.depth_order(q["depth"], np.nonzero(pr["visible"])[0])
    for limit, drawn in ((z, True), (np.nextafter(z, np.float16(0)), False)):
        occ = np.full((h, w), np.float32(limit), np.float32)
        v = checker_view(name, occ=occ)
        m = M.blend_untiled(q, order, w, h, M.GLOBAL_CLEAR, occluder=occ)
        print(f"Z = {float(limit)}: alpha at the centre {v['alpha'][23, 23]:.4f} (model {m['alpha'][23, 23]:.4f})")
        for alpha in (v["alpha"], m["alpha"]):
            assert abs(alpha[23, 23] - 0.99) < 5e-3 if drawn else alpha[23, 23] < 1e-3
        if not drawn:  # none of it: the frame of the scene without the splat (and the lists check holds the checker)
            rest = M.blend_untiled(q, order[order != 0], w, h, M.GLOBAL_CLEAR, occluder=occ)
            assert np.array_equal(m["alpha"], rest["alpha"]) and np.array_equal(m["color"], rest["color"])
        T.check_blend("lists", T.measure_lists(v, w, h, occluder=occ), v)


@pytest.mark.parametrize("name", OCCLUDED)
def test_sticky_flag_equals_the_comparison(name):
    """DESIGN.md 21's claim, on the model alone: the flag and the entry-by-entry comparison give one frame."""
    c = case_of(name)
    w, h = c["width"], c["height"]
    pr, _ = projection_of(name)
    q = M.quantise_global(pr)
    order = M.depth_order(q["depth"], np.nonzero(pr["visible"])[0])
    for kind in ("ramp", "step", "special"):
        occ = occluder_of(name, kind)
        a = M.blend_untiled(q, order, w, h, M.GLOBAL_CLEAR, occluder=occ, pick=True)
        b = M.blend_untiled(q, order, w, h, M.GLOBAL_CLEAR, occluder=occ, pick=True, occlusion_form="entry")
        for key in ("color", "alpha", "depth", "pick", "pick_weight", "closed"):
            assert np.array_equal(a[key], b[key]), (kind, key)
        assert a["cut_any"].any() and not a["cut_any"].all()


# ---- 4. the pick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse_sh1_f16_200x150", "dense_sh0_f32_128x64", "plane_ties_128x64",
                                  "composite_3_sh1_f16_200x150"])
def test_pick(refs, name):
    c = case_of(name)
    pr, owner = projection_of(name)
    v = checker_view(name)
    f = check_pick(v, c["width"], c["height"], what=name)
    has = f["has"]
    assert (owner[v["pick"][has], 0] >= 0).all(), "a pick that belongs to no object"
    if name.startswith("composite"):
        assert len(np.unique(owner[v["pick"][has], 0])) == 3, "every object is picked somewhere"
    if name.startswith("plane"):
        # one depth: every list is one tie run, and where several entries share the largest weight the first wins
        m = f["model"]
        tie = has & (m["pick_weight"] == m["pick_second"])
        print(f"{int(tie.sum())} pixels with two entries of the largest weight")
        assert np.array_equal(v["pick"][tie], m["pick"][tie])


def test_pick_whole_frame(refs):
    """The pick against the model alone (projection, quantisation, every gaussian on every pixel): on the pixels
    the whole-frame check keeps, a winner more than 2 PICK_TOL clear of its runner-up is the checker's pick."""
    name = "sparse_sh1_f16_200x150"
    c = case_of(name)
    w, h = c["width"], c["height"]
    pr, owner = projection_of(name)
    v = checker_view(name)
    keep = {}
    T.measure_frame(pr, v, w, h, model_out=keep)
    q = M.quantise_global(pr)
    m = M.blend_untiled(q, M.depth_order(q["depth"], np.nonzero(pr["visible"])[0]), w, h, M.GLOBAL_CLEAR, pick=True)
    # (what the whole-frame blend tolerance allows for an alpha also bounds what a weight may differ by)
    margin = 2.0 * PICK_TOL["sparse"] + 2.0 * T.BLEND_TOL[("frame", "sparse")][1]
    clear = keep["where"] & (m["pick_weight"] - m["pick_second"] > margin)
    print(f"{int(clear.sum())} of {int(keep['where'].sum())} compared pixels have a clear winner")
    assert clear.sum() >= 0.5 * keep["where"].sum()
    assert np.array_equal(v["pick"][clear], m["pick"][clear])


# ---- 5. styles -------------------------------------------------------------------------------------------------------
def test_styled(refs):
    name = "sparse_sh1_f16_200x150"
    n = counts_of(case_of(name))[0]
    states = [states_for(n, 51)]
    spr, owner = styled_projection(name, states)
    assert (states[0] >= len(STYLES)).sum() > 50 and all((states[0] == s).sum() > 50 for s in range(len(STYLES)))
    v = checker_view(name, states=states, styles=STYLES)
    check_frame(name, v, spr, owner, pick=True, what="styled")
    assert not spr["visible"][v["pick"][v["pick"] >= 0]].__invert__().any(), "a hidden gaussian is picked"


def test_styled_occluded_pick_composite(refs):
    """Item 2's occluder and item 5's styles on the three-object composite, one object styled as a whole by a
    {NULL, default_state} entry: the all-options walk."""
    name = "composite_3_sh1_f16_200x150"
    counts = counts_of(case_of(name))
    states = all_options_states(counts)
    spr, owner = styled_projection(name, states)
    occ = occluder_of(name, "step")
    v = checker_view(name, occ=occ, states=states, styles=STYLES)
    check_frame(name, v, spr, owner, occ=occ, pick=True, what="composite, all options")


def all_options_states(counts):
    """The rotated object half-tinted as a whole, the similarity object under per-gaussian states, the single
    gaussian tinted."""
    return [2, 0, states_for(counts[2], 52), 1]


# ---- 7. the selects --------------------------------------------------------------------------------------------------
def masks(w, h, at=None):
    """at: the (x, y) of the one-pixel mask."""
    yy, xx = np.mgrid[0:h, 0:w]
    one = np.zeros((h, w), np.uint8)
    x, y = (w // 2, h // 2) if at is None else at
    one[y, x] = 1
    return {"checkerboard": (((xx // 3) + (yy // 3)) % 2).astype(np.uint8) * 255, "one pixel": one,
            "empty": np.zeros((h, w), np.uint8)}


SELECT = "sparse_sh1_f16_200x150"


def select_cases():
    """(what, mask name, and, xor, with styles): a set, a toggle and an assign."""
    return [("set bit 3", "checkerboard", ~8, 8, False), ("toggle", "checkerboard", 0xFF, 1, True),
            ("assign", "one pixel", 0, 77, False), ("nothing", "empty", 0, 77, True)]


def test_select_mask(refs, oracle):
    import style_ref
    c = case_of(SELECT)
    w, h = c["width"], c["height"]
    pr, _ = projection_of(SELECT)
    world, harm, _ = c["objects"][0]
    r = oracle.render(world, harm, c["sh"], c["cam"], w, h)
    n = len(world)
    before = states_for(n, 53)
    total = 0
    g = np.nonzero(pr["visible"] & (M.styles_of(before, STYLES)[:, 5] == 0))[0][0]  # under the one-pixel mask
    at = tuple(np.floor(M.round_h(pr["mean"][g]) + 0.5).astype(int))
    for what, mname, am, xm, styled in select_cases():
        mask = masks(w, h, at)[mname]
        got, cnt = style_ref.select_mask(r["render_data"], r["mask"], w, h, mask, before, am, xm,
                                         styles=style_ref.style_table(STYLES) if styled else None)
        want, mcnt, doubt = M.select_mask(pr, before, mask, w, h, am, xm, styles=STYLES if styled else None,
                                          eps=T.BOUNDARY_EPS["mean"] * max(w, h))
        doubt = doubt | T.left_out(pr)
        check_select(SELECT, got, cnt, before, want, mcnt, doubt, what)
        total += mcnt
        assert (mcnt == 0) == (mname == "empty")
    assert total > 100


def test_select_pick(refs):
    """frame_ref's set rule against the model's, on the checker's pick image of the composite."""
    import frame_ref
    name = "composite_3_sh1_f16_200x150"
    c = case_of(name)
    w, h = c["width"], c["height"]
    counts = counts_of(c)
    base, _ = M.item_layout(counts)
    v = checker_view(name, occ=occluder_of(name, "step"))
    items = np.where(v["pick"] < 0, NONE, v["pick"]).astype(np.uint32)
    for o in (0, 2, 3):
        n = counts[o]
        before = states_for(n, 54 + o)
        for what, mname, am, xm, _ in select_cases():
            mask = masks(w, h)[mname]
            for gc in (n, max(n - 100, 1)):
                got, cnt = frame_ref.select_pick(items, mask, int(base[o]), n, before, gc, am, xm)
                want, mcnt, doubt = M.select_pick(items.astype(np.int64), counts, o, before, gc, am, xm, mask=mask)
                check_select(name, got, cnt, before, want, mcnt, doubt, f"object {o} {what}")
    got, cnt = frame_ref.select_pick(items, None, 0, counts[0], np.zeros(counts[0], np.uint8), counts[0], 0, 1)
    assert 0 < cnt < counts[0] and cnt == int(got.sum())
