"""The orthographic frames' checker (tests/ortho/ortho_ref.c) against the float64 model of the orthographic rule
(tests/f64_ortho_model.py): CPU only.

The checker restates DESIGN.md 26 and was written with the kernels it checks, at the same four places.  Here it is
held to a second derivation from the mathematics -- an affine mean, J R S^2 R^T J^T + 0.3 I with the map's constant
linear part, one parallel ray found as that linear part's null direction, depth along the axis -- with the checks and
helpers of tests/test_f64_model.py and tests/test_f64_features_model.py and the blend, quantisation, pick, occluder
and style functions of tests/f64_model.py.  tests/test_f64_ortho_gpu.py applies the same functions and constants to
what the HIP path returns.

Constants (DESIGN.md 16's rule, DESIGN.md 26's table): twice the largest difference measured between the checker and
the model over the scenes below, the measured value beside each; F32 stands in where the measured excess of a record
field is not positive.  Gaussians within T.EPS_MARGIN of a cull threshold or in a repair branch are left out of the
comparison, at most T.MAX_LEFT_OUT of a scene: the rule and the cap of the perspective frames.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_model as M  # noqa: E402
import f64_ortho_model as OM  # noqa: E402
import test_f64_features_model as F  # noqa: E402
import test_f64_model as T  # noqa: E402

F32 = T.F32
# measured excess beyond the storage step (units: T.RECORD_TOL's): mean 1.68e-9 (the composite), depth 5.98e-9
# (ortho_sparse_sh1_f16_200x150); conic (-8.9e-5 at best), colour and opacity (0) not positive
RECORD_TOL = dict(mean=3.4e-9, depth=1.2e-8, conic=F32, color=F32, opacity=F32)
# measured blend differences: (check, regime) -> (rgb, alpha, depth)
BLEND_TOL = {
    # measured: rgb 1.62e-3 (ortho_sparse_sh1_f16_200x150), alpha 1.78e-3 (the same, step occluder), depth 1.10e-2
    # (ortho_composite_3_sh3_f16_200x150)
    ("lists", "sparse"): (3.24e-3, 3.57e-3, 2.2e-2),
    # measured: rgb 4.16e-3, alpha 1.86e-3 (ramp occluder), depth 2.23e-2 (all ortho_dense_sh0_f32_128x64)
    ("lists", "dense"): (8.32e-3, 3.72e-3, 4.46e-2),
    # measured: rgb 4.80e-3, alpha 6.02e-3, depth 5.44e-2 (all ortho_sparse_sh1_f16_200x150)
    ("frame", "sparse"): (9.6e-3, 1.21e-2, 1.09e-1),
    # measured: rgb 6.05e-3, alpha 3.91e-3, depth 3.33e-2 (ortho_dense_sh0_f32_128x64)
    ("frame", "dense"): (1.21e-2, 7.82e-3, 6.66e-2),
}
# the largest model-weight deficit of the checker's pick (F.PICK_TOL's quantity)
PICK_TOL = {
    "sparse": 5.18e-4,  # measured: 2.59e-4 (ortho_composite_3_sh3_f16_200x150)
    "dense": 1.19e-3,   # measured: 5.92e-4 (ortho_dense_sh0_f32_128x64, plain and under both occluders)
}

# A vacuity guard, not a tolerance: of the picked pixels, the share whose runner-up is more than 2 PICK_TOL below the
# winner (only those are held to the model's pick).  An orthographic view draws the whole cloud at one size, stacked
# along the axis, so runner-ups lie closer than under the perspective camera (F.MIN_CLEAR_SHARE is 0.75): the scenes
# below have 51% to 100%.
MIN_CLEAR_SHARE = 0.4

# ---- scenes ------------------------------------------------------------------------------------------------
def camera(w, h, half_height, angle=0.0, flipped=False, near=0.1, far=10.0):
    """scenes.ortho_camera turned by `angle` (radians) about the y axis through gen_scene's middle (0, 0, 5.5).
    flipped: the same camera in the other convention -- it looks down its own -z (the view turned by half a turn
    about y) and proj[10] < 0, so sigma = -1."""
    from gsm_amd import scenes
    c, s = np.cos(angle), np.sin(angle)
    V = np.eye(4)
    V[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    pivot = np.array([0.0, 0.0, 5.5])
    V[:3, 3] = pivot - V[:3, :3] @ pivot
    if flipped:
        V = np.diag([-1.0, 1.0, -1.0, 1.0]) @ V
    cam = scenes.ortho_camera(w, h, half_height, near=near, far=far, view=V.T.reshape(-1).astype(np.float32))
    if flipped:
        cam["proj"][10] = -cam["proj"][10]
    return cam


# name: (width, height, SH components, precision, colour space, camera arguments, [(gaussians, seed, model matrix)])
CASES = {
    "ortho_sparse_sh1_f16_200x150": (200, 150, 4, 1, 0, dict(half_height=3.0, angle=0.35), [(700, 11, None)]),
    # sigma = -1, a view that is no identity and no symmetric matrix, every SH band
    "ortho_flipped_sh3_f32_128x64": (128, 64, 16, 0, 0, dict(half_height=3.0, angle=-0.5, flipped=True),
                                          [(250, 13, None)]),
    "ortho_dense_sh0_f32_128x64": (128, 64, 1, 0, 0, dict(half_height=3.0), [(3000, 12, None)]),
    # F.COMPOSITES' poses: a rotation about an oblique axis with a translation, an empty object, a similarity of
    # scale 1.25 (A^-1 and A^T then differ by a factor, not a direction) and one gaussian at the identity
    "ortho_composite_3_sh3_f16_200x150": (200, 150, 16, 1, 0, dict(half_height=3.5, angle=0.2), [
        (250, 41, F.pose((1.0, 2.0, 0.5), 25.0, (0.3, -0.2, 0.4))),
        (0, 0, F.IDENTITY),
        (120, 42, F.pose((0.3, -1.0, 0.4), -35.0, (-0.2, 0.1, -0.3), scale=1.25)),
        (1, 43, F.IDENTITY)]),
}
SINGLES = [n for n in CASES if "composite" not in n]
COMPOSITE = "ortho_composite_3_sh3_f16_200x150"
ALL = sorted(CASES)


@functools.lru_cache(maxsize=None)
def case_of(name):
    from gsm_amd import scenes
    w, h, sh, prec, cs, cam_kw, objs = CASES[name]
    objects = []
    for n, seed, model in objs:
        world, harm, _ = scenes.gen_scene(max(n, 1), w, h, sh, prec, seed=seed)
        if n == 1:  # on the axis through the pivot, in front of the other two objects
            world["px"], world["py"], world["pz"] = 0.0, 0.0, 3.0
        objects.append((world[:n], np.asarray(harm).reshape(max(n, 1), -1)[:n].reshape(-1), model))
    return dict(objects=objects, sh=sh, cam=camera(w, h, **cam_kw), width=w, height=h, color_space=cs)


@functools.lru_cache(maxsize=None)
def projection_of(name):
    """(model projection indexed by item, owner [items, 2]); a single scene keeps its n entries."""
    c = case_of(name)
    pr, _, owner = OM.project_composite(c["objects"], c["sh"], c["cam"], c["width"], c["height"], c["color_space"])
    if len(c["objects"]) == 1:
        n = len(c["objects"][0][0])
        pr = {k: ({m: v[:n] for m, v in val.items()} if k == "margins" else val[:n]) for k, val in pr.items()}
        owner = owner[:n]
    return pr, owner


def styled_projection(name, states, styles=F.STYLES):
    pr, owner = projection_of(name)
    return M.apply_styles(pr, F.item_states(case_of(name), states, len(owner)), styles), owner


def occluder_of(name, kind):
    pr, _ = projection_of(name)
    c = case_of(name)
    w, h = c["width"], c["height"]
    return {"ramp": lambda: F.ramp_occluder(pr, w, h), "step": lambda: F.step_occluder(pr, w, h, 7),
            "special": lambda: F.special_occluder(pr, w, h, 8)}[kind]()


def checker_view(name, occ=None, states=None, styles=None, lib=None):
    """ortho_ref's frame of the case (records, lists) and its walk (colour, depth, pick), indexed by item.
    lib: another build of the checker (ortho_ref._bind's pair)."""
    import ortho_ref
    c = case_of(name)
    st = [0] * len(c["objects"]) if states is None else states
    table = ortho_ref.style_table([M.IDENTITY_STYLE] if styles is None else styles)
    objs = F._checker_objects(c, st)
    with ortho_ref.frame(objs, c["sh"], c["width"], c["height"], styles=table, color_space=c["color_space"],
                         _lib_override=lib) as fr:
        r, res = fr.data(), fr.walk(occ)
    assert r["overflow"] == 0
    return F._to_items(c, r, res["color"], res["depth"], res["pick"])


# ---- checks (shared with tests/test_f64_ortho_gpu.py) -------------------------------------------------------
def check_records(pr, view, w, h):
    fig = T.measure_records(pr, view, w, h)
    print("records beyond the storage step:", {k: float(f"{v:.3g}") for k, v in fig.items()})
    for k, v in fig.items():
        assert v <= RECORD_TOL[k], (k, v, RECORD_TOL[k])
    return fig


def check_blend(which, fig, view):
    tol = BLEND_TOL[(which, T.regime(view))]
    print(f"{which} ({T.regime(view)}, deepest {T.deepest(view)}): rgb {fig[0]:.3g} alpha {fig[1]:.3g} depth "
          f"{fig[2]:.3g}" + (f" stray alpha {fig[3]:.3g}" if len(fig) > 3 else ""), "bounds", tol)
    assert fig[0] <= tol[0] and fig[1] <= tol[1] and fig[2] <= tol[2], (fig, tol)
    if len(fig) > 3:
        assert fig[3] <= tol[1], ("alpha outside the drawn tiles", fig[3], tol[1])


def check_pick(view, w, h, occ=None, what=""):
    """F.check_pick with this file's constants."""
    tol = PICK_TOL[T.regime(view)]
    f = F.measure_pick(view, w, h, occ)
    m, has = f["model"], f["has"]
    clear = has & (m["pick_weight"] - m["pick_second"] > 2.0 * tol)
    share = float(clear.sum()) / max(int(has.sum()), 1)
    print(f"pick {what} ({T.regime(view)}): {int(has.sum())} picked, deficit {f['deficit']:.3g}, largest weight of a "
          f"'none' {f['missed']:.3g} (bound {tol}), {share:.1%} clear winners")
    assert has.any() and f["deficit"] <= tol, (f["deficit"], tol)
    assert f["missed"] <= tol, (f["missed"], tol)
    assert share >= MIN_CLEAR_SHARE, f"the scene's premise: {share:.1%} of the picks are clear winners"
    bad = np.argwhere(clear & (view["pick"] != m["pick"]))
    assert len(bad) == 0, (f"{len(bad)} clear winners are not picked, first (y, x) {bad[:4].tolist()}")
    return f


def check_frame(name, view, pr, owner, occ=None, whole=True, pick=False, what=""):
    """F.check_frame for an orthographic case: visibility (with the cull-margin cap), records, order, compositing
    on the view's lists, the whole frame from the model alone, and the pick by weight."""
    c = case_of(name)
    w, h = c["width"], c["height"]
    view["mask"] = view["mask"] & (owner[:, 0] >= 0)
    T.check_visibility(pr, view["mask"])
    check_records(pr, view, w, h)
    T.check_order(pr, view, owner)
    listed = np.unique(np.concatenate([ids for _, ids in view["lists"]] + [np.zeros(0, np.int64)])).astype(np.int64)
    assert pr["visible"][listed][~T.left_out(pr)[listed]].all(), "a list names a gaussian the model culls or hides"
    if "no_tiles" in pr:
        assert pr["no_tiles"].any() and not pr["no_tiles"][listed].any(), "a styled opacity byte of 0 has no tiles"
    check_blend("lists", T.measure_lists(view, w, h, occluder=occ), view)
    out = None
    if whole:
        out = {}
        check_blend("frame", T.measure_frame(pr, view, w, h, occluder=occ, model_out=out), view)
    if pick:
        check_pick(view, w, h, occ, what)
    return out


@pytest.fixture(scope="module")
def refs(oracle):
    import ortho_ref
    ortho_ref.lib()
    return True


# ---- 0. the scenes' premises, from the model alone -------------------------------------------------------------
def test_scene_premises(refs):
    depths = {s: T.deepest(checker_view(s)) for s in ALL}
    print(depths)
    assert all(d <= T.SPARSE_MAX or d >= T.DENSE_MIN for d in depths.values()), depths
    assert depths["ortho_dense_sh0_f32_128x64"] >= T.DENSE_MIN
    for name in ALL:
        pr, _ = projection_of(name)
        n = len(pr["margin"])
        vis = pr["visible"]
        culled = {k: int((v <= 0).sum()) for k, v in pr["margins"].items()}
        print(name, f"{int(vis.sum())} of {n} visible; culled by", culled)
        assert vis.sum() >= 0.3 * n, name
        assert culled["screen"] > 0, "some gaussians leave by the screen cull"
        assert T.left_out(pr).sum() <= T.MAX_LEFT_OUT * n, "the cap on the share within the model's margin of a cull"


def test_axis_and_sign_of_the_model():
    """The model's own derivation on cameras whose answer is known by construction."""
    from gsm_amd import scenes
    cam = scenes.ortho_camera(64, 32, 1.0)
    toward, sign = OM.camera_axis(M._mat(cam["view"]), M._mat(cam["proj"]))
    assert sign == 1.0 and np.allclose(toward, [0, 0, -1])       # looks down +z: the camera is toward -z
    a = 0.35
    cam = camera(64, 32, 1.0, angle=a)
    toward, _ = OM.camera_axis(M._mat(cam["view"]), M._mat(cam["proj"]))
    # the camera-to-world rotation is the view's transpose: its axis (0, 0, 1) in world space is V^T e_z
    looks = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]).T @ [0, 0, 1.0]
    assert np.allclose(toward, -looks, atol=1e-6) and abs(looks[0]) > 0.3
    cam = camera(64, 32, 1.0, angle=a, flipped=True)
    toward2, sign = OM.camera_axis(M._mat(cam["view"]), M._mat(cam["proj"]))
    assert sign == -1.0 and np.allclose(toward2, toward, atol=1e-6)  # the same camera in the other convention


# ---- 1. the plain frame, the pick, the composite --------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_frame_and_pick(refs, name):
    pr, owner = projection_of(name)
    v = checker_view(name)
    check_frame(name, v, pr, owner, pick=True, what=name)
    if name == COMPOSITE:
        has = v["pick"] >= 0
        assert len(np.unique(owner[v["pick"][has], 0])) == 3, "every object is picked somewhere"
        assert F.interleaved_tiles(v, owner), "the scene's premise: some list interleaves all three objects"


def test_flipped_camera_is_the_same_frame(refs):
    """From the model alone: the flipped convention (sigma = -1) of a camera gives the projection of the Metal one
    mirrored in x -- the same depths, footprints' sigmas and colours."""
    name = "ortho_flipped_sh3_f32_128x64"
    c = case_of(name)
    w, h, sh, prec, cs, kw, _ = CASES[name]
    world, harm, _ = c["objects"][0]
    a = OM.project(world, harm, sh, c["cam"], w, h, cs)
    b = OM.project(world, harm, sh, camera(w, h, **dict(kw, flipped=False)), w, h, cs)
    assert np.allclose(a["depth"], b["depth"], atol=1e-6) and np.allclose(a["sigma"], b["sigma"], atol=1e-6)
    assert np.allclose(a["color"], b["color"], atol=1e-6)
    assert np.allclose(a["mean"][:, 0], (w - 1.0) - b["mean"][:, 0], atol=1e-4)
    assert np.allclose(a["mean"][:, 1], b["mean"][:, 1], atol=1e-4)


# ---- 2. the options --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ramp", "step"])
@pytest.mark.parametrize("name", ["ortho_sparse_sh1_f16_200x150", "ortho_dense_sh0_f32_128x64"])
def test_occluded(refs, name, kind):
    pr, owner = projection_of(name)
    occ = occluder_of(name, kind)
    v = checker_view(name, occ=occ)
    model = check_frame(name, v, pr, owner, occ=occ, pick=True, what=f"{name} {kind}")
    if "sparse" in name:  # (the dense scene's lists are deep enough that nearly every pixel closes somewhere)
        F.assert_occluder_not_vacuous(model, f"{name} {kind}")


def test_styled_occluded_pick_composite(refs):
    counts = F.counts_of(case_of(COMPOSITE))
    states = F.all_options_states(counts)
    spr, owner = styled_projection(COMPOSITE, states)
    occ = occluder_of(COMPOSITE, "step")
    v = checker_view(COMPOSITE, occ=occ, states=states, styles=F.STYLES)
    check_frame(COMPOSITE, v, spr, owner, occ=occ, pick=True, what="composite, all options")


# ---- 3. the select ---------------------------------------------------------------------------------------------------
SELECT = "ortho_sparse_sh1_f16_200x150"


def select_inputs():
    c = case_of(SELECT)
    pr, _ = projection_of(SELECT)
    n = len(c["objects"][0][0])
    before = F.states_for(n, 53)
    g = np.nonzero(pr["visible"] & (M.styles_of(before, F.STYLES)[:, 5] == 0))[0][0]  # under the one-pixel mask
    at = tuple(np.floor(M.round_h(pr["mean"][g]) + 0.5).astype(int))
    return c, pr, before, at


def test_select_mask(refs):
    """style_ref's select rule over the orthographic checker's records, against the model's."""
    import style_ref
    c, pr, before, at = select_inputs()
    w, h = c["width"], c["height"]
    v = checker_view(SELECT)
    import ortho_ref
    world, harm, _ = c["objects"][0]
    r = ortho_ref.render(world, harm, c["sh"], c["cam"], w, h)
    total = 0
    for what, mname, am, xm, styled in F.select_cases():
        mask = F.masks(w, h, at)[mname]
        got, cnt = style_ref.select_mask(r["render_data"], r["mask"], w, h, mask, before, am, xm,
                                         styles=style_ref.style_table(F.STYLES) if styled else None)
        want, mcnt, doubt = M.select_mask(pr, before, mask, w, h, am, xm, styles=F.STYLES if styled else None,
                                          eps=T.BOUNDARY_EPS["mean"] * max(w, h))
        F.check_select(SELECT, got, cnt, before, want, mcnt, doubt | T.left_out(pr), what)
        total += mcnt
        assert (mcnt == 0) == (mname == "empty")
    assert total > 100 and v["mask"].sum() > 100
