"""The HIP path's composite, pick, occluded, styled, all-options and batch frames and its selects against the
float64 model (tests/f64_model.py), through the C ABI.

The checks and constants of tests/test_f64_features_model.py applied to what the library returns: colour, depth
and pick targets, RENDER_DATA, BOUNDS, HEADERS and SORTED_VALUES of render_composite / render_frame /
render_frames, and the state bytes of select_mask / select_pick.  No checker and no oracle is consulted.  Every
frame asserts the blend instance it ran by blend_kernel_kind(); the unit shape is set by the handle's size.
"""
import numpy as np
import pytest

import f64_model as M
import test_f64_features_model as F
import test_f64_model as T
from test_render_pick import Scene, Targets, cus, handle, handle_size_for_tiles

pytestmark = pytest.mark.gpu

QUADRANT, HALF_TILE = 1, 2  # gsm_blend_kernel (include/gsm_debug.h)


def _styles(gsm, styles):
    return [gsm.Style(tint=s[:3], tint_amount=s[3], opacity_scale=s[4], hidden=bool(s[5])) for s in styles]


def _dev_states(torch, states):
    return [int(s) if np.isscalar(s) else torch.from_numpy(np.ascontiguousarray(s, np.uint8).copy()).cuda()
            for s in states]


def _objects(gsm, torch, case):
    """(Scene list kept alive, SceneObject list): every pose through scenes.object_camera, the thing under test."""
    from gsm_amd import scenes
    scs = [Scene(torch, world, harm, case["sh"]) for world, harm, _ in case["objects"]]
    cams = [case["cam"] if model is None else scenes.object_camera(case["cam"], model)
            for _, _, model in case["objects"]]
    return scs, [gsm.SceneObject(s.input(gsm), gsm.CameraParams.from_dict(c)) for s, c in zip(scs, cams)]


def _handle_for(gsm, torch, case, kind, items):
    w, h = case["width"], case["height"]
    mw, mh = (w, h) if kind == QUADRANT else handle_size_for_tiles(8 * cus(torch) + 1)
    prec = 1 if case["objects"][0][0].dtype.itemsize == 32 else 0
    r = handle(gsm, 4 * max(items, 256), mw, mh, prec)
    r.set_profiling(stage_events=False, capture=True)
    return r, mw


def _frame_grid(headers, w, h, mw):
    """The handle's tile grid (set by its maximal width) cut to the frame's; tiles outside the frame hold nothing."""
    hx, fx, fy = (mw + 31) // 32, (w + 31) // 32, (h + 15) // 16
    grid = np.asarray(headers).reshape(-1, hx, 2)
    keep = np.zeros(grid.shape[:2], bool)
    keep[:fy, :fx] = True
    assert (grid[..., 1][~keep] == 0).all(), "a tile outside the frame has entries"
    return grid[:fy, :fx].reshape(-1, 2)


def _captured_view(gsm, r, case, items, mw, color, depth, pick):
    w, h = case["width"], case["height"]
    rd = r.copy_buffer(gsm.BufferId.RENDER_DATA)[:items]
    b = r.copy_buffer(gsm.BufferId.BOUNDS)[:items]
    mask = (b[:, 0] <= b[:, 1]) & (b[:, 2] <= b[:, 3])
    headers = _frame_grid(r.copy_buffer(gsm.BufferId.HEADERS), w, h, mw)
    sv = r.copy_buffer(gsm.BufferId.SORTED_VALUES).astype(np.int64)
    return F.feature_view(case, rd, mask, headers, sv, color.view(np.uint16).reshape(h, w, 4),
                          depth.view(np.uint16).reshape(h, w), pick)


def gpu_frame(gsm, torch, name, kind, entry="frame", pick=False, occ=None, states=None, styles=None):
    """One render_frame (or render_composite) of the case into sentinel targets, captured; returns the view and,
    for a pick frame, pick_owner's (object, gaussian) images."""
    case = F.case_of(name)
    w, h = case["width"], case["height"]
    items = len(F.projection_of(name)[1])
    scs, objects = _objects(gsm, torch, case)
    r, mw = _handle_for(gsm, torch, case, kind, items)
    t = Targets(torch, w, h)
    if entry == "composite":
        r.render_composite(t.color, t.depth, objects, w, h)
    else:
        r.render_frame(t.color, t.depth, objects, w, h, pick=t.pick if pick else None,
                       occluder=None if occ is None else torch.from_numpy(np.ascontiguousarray(occ, np.float32)).cuda(),
                       states=None if states is None else _dev_states(torch, states),
                       styles=None if styles is None else _styles(gsm, styles), pick_pitch=t.pick_pitch)
    c, d, p = t.read(with_pick=pick)
    assert r.counters()["overflow"] == 0
    assert r.blend_kernel_kind() == kind
    view = _captured_view(gsm, r, case, items, mw, c, d, p if pick else None)
    owner = r.pick_owner(p) if pick else None
    r.close()
    return view, owner


def check_owner(view, owner_images, owner):
    """gsm_global_pick_owner against the model's item map."""
    obj, gid = owner_images
    has = view["pick"] >= 0
    assert np.array_equal(obj[has], owner[view["pick"][has], 0]) and np.array_equal(gid[has], owner[view["pick"][has], 1])
    assert (obj[~has] == F.NONE).all() and (gid[~has] == F.NONE).all()


# ---- the composite -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(F.COMPOSITES))
def test_composite(gsm, cuda, name):
    pr, owner = F.projection_of(name)
    v, _ = gpu_frame(gsm, cuda, name, QUADRANT, entry="composite")
    F.check_frame(name, v, pr, owner)


# ---- k_blend_px_pick, k_blend_px_occ: both shapes ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", [QUADRANT, HALF_TILE])
@pytest.mark.parametrize("name", ["sparse_sh1_f16_200x150", "plane_ties_128x64"])
def test_pick_only(gsm, cuda, name, kind):
    c = F.case_of(name)
    pr, owner = F.projection_of(name)
    v, own = gpu_frame(gsm, cuda, name, kind, pick=True)
    F.check_frame(name, v, pr, owner, whole=kind == QUADRANT, pick=True, what=f"{name} kind {kind}")
    check_owner(v, own, owner)


@pytest.mark.parametrize("kind,occ", [(QUADRANT, "ramp"), (QUADRANT, "special"), (HALF_TILE, "step")])
@pytest.mark.parametrize("name", ["sparse_sh1_f16_200x150", "dense_sh0_f32_128x64"])
def test_occluder_only(gsm, cuda, name, kind, occ):
    pr, owner = F.projection_of(name)
    o = F.occluder_of(name, occ)
    v, _ = gpu_frame(gsm, cuda, name, kind, occ=o)
    model = F.check_frame(name, v, pr, owner, occ=o, whole=kind == QUADRANT)
    if model is not None:
        F.assert_occluder_not_vacuous(model, f"{name} {occ}")


def test_a_splat_at_the_surface_is_drawn(gsm, cuda):
    name = "opaque_splat_64x64"
    c = F.case_of(name)
    w, h = c["width"], c["height"]
    pr, owner = F.projection_of(name)
    z = np.float16(M.round_h(pr["depth"][0]))
    for limit, drawn in ((z, True), (np.nextafter(z, np.float16(0)), False)):
        occ = np.full((h, w), np.float32(limit), np.float32)
        v, _ = gpu_frame(gsm, cuda, name, QUADRANT, occ=occ)
        assert v["rec"]["depth"][0] == float(z)
        print(f"Z = {float(limit)}: alpha at the centre {v['alpha'][23, 23]:.4f}")
        assert abs(v["alpha"][23, 23] - 0.99) < 5e-3 if drawn else v["alpha"][23, 23] < 1e-3
        # (on the lists only: the whole-frame rule leaves out every pixel of a splat that lies at its surface)
        F.check_frame(name, v, pr, owner, occ=occ, whole=False)


# ---- the all-options walk (k_blend_px_occ_pick), both shapes -------------------------------------------------------------
@pytest.mark.parametrize("kind", [QUADRANT, HALF_TILE])
def test_all_options_composite(gsm, cuda, kind):
    name = "composite_3_sh1_f16_200x150"
    states = F.all_options_states(F.counts_of(F.case_of(name)))
    spr, owner = F.styled_projection(name, states)
    occ = F.occluder_of(name, "step")
    v, own = gpu_frame(gsm, cuda, name, kind, pick=True, occ=occ, states=states, styles=F.STYLES)
    F.check_frame(name, v, spr, owner, occ=occ, whole=kind == QUADRANT, pick=True, what=f"all options kind {kind}")
    check_owner(v, own, owner)
    assert spr["visible"][v["pick"][v["pick"] >= 0]].all(), "a hidden gaussian is picked"


def test_styled(gsm, cuda):
    name = "sparse_sh1_f16_200x150"
    states = [F.states_for(F.counts_of(F.case_of(name))[0], 51)]
    spr, owner = F.styled_projection(name, states)
    v, _ = gpu_frame(gsm, cuda, name, QUADRANT, pick=True, states=states, styles=F.STYLES)
    F.check_frame(name, v, spr, owner, pick=True, what="styled")


# ---- a list deeper than the walk's pipeline, closed in mid-walk ------------------------------------------------------------
def test_long_walk_closed_in_mid_walk(gsm, cuda):
    name = "long_sh0_f32_64x32"
    c = F.case_of(name)
    w, h = c["width"], c["height"]
    pr, owner = F.projection_of(name)
    occ = F.ramp_occluder(pr, w, h)
    v, _ = gpu_frame(gsm, cuda, name, QUADRANT, pick=True, occ=occ)
    assert T.deepest(v) > 256
    T.check_visibility(pr, v["mask"])
    T.check_order(pr, v)
    f = F.check_pick(v, w, h, occ, what=name)
    m = f["model"]
    assert (m["closed"] & ~m["closed_first"]).sum() > 0.2 * w * h, "the premise: pixels closed in mid-walk"


# ---- the batch instances: three descriptors of three sizes -----------------------------------------------------------------
def test_batch_of_three_frames(gsm, cuda):
    """One plain 200x150 view, a 128x64 view with pick and occluder, a 64x64 view with styles and pick.  Colour,
    depth and pick come from the batch; records and lists from the same descriptor rendered alone with capture
    (the batch's bytes equal the single frame's by contract, and the checks would show a view that departs)."""
    names = ["sparse_sh0_f32_200x150", "dense_sh0_f32_128x64", "small_sh0_f32_64x64"]
    cases = [F.case_of(n) for n in names]
    n2 = F.counts_of(cases[2])[0]
    states2 = [F.states_for(n2, 55)]
    occ1 = F.occluder_of(names[1], "step")
    options = [dict(), dict(pick=True, occ=occ1), dict(pick=True, states=states2, styles=F.STYLES)]
    r = handle(gsm, 8192, 320, 180, 0)
    keep, frames, targets = [], [], []
    for c, o in zip(cases, options):
        scs, objects = _objects(gsm, cuda, c)
        t = Targets(cuda, c["width"], c["height"])
        occ = None if "occ" not in o else cuda.from_numpy(o["occ"]).cuda()
        st = None if "states" not in o else _dev_states(cuda, o["states"])
        keep.append((scs, occ, st))
        frames.append(gsm.Frame((objects[0].input, objects[0].camera), c["width"], c["height"], t.color, t.depth,
                                pick=t.pick if o.get("pick") else None, occluder=occ,
                                states=None if st is None else st[0],
                                styles=_styles(gsm, o["styles"]) if "styles" in o else None,
                                pick_pitch=t.pick_pitch))
        targets.append(t)
    r.render_frames(frames)
    got = [t.read(with_pick=bool(o.get("pick"))) for t, o in zip(targets, options)]
    assert r.counters()["overflow"] == 0 and r.blend_kernel_kind() == QUADRANT
    r.close()
    for name, c, o, (col, dep, pick) in zip(names, cases, options, got):
        w, h = c["width"], c["height"]
        pr, owner = F.projection_of(name)
        if "states" in o:
            pr, owner = F.styled_projection(name, o["states"])
        alone, _ = gpu_frame(gsm, cuda, name, QUADRANT, pick=bool(o.get("pick")), occ=o.get("occ"),
                             states=o.get("states"), styles=o.get("styles"))
        v = dict(alone, color=M.h2d(col.view(np.uint16).reshape(h, w, 4))[..., :3],
                 alpha=M.h2d(col.view(np.uint16).reshape(h, w, 4))[..., 3], depth=M.h2d(dep.view(np.uint16).reshape(h, w)))
        if o.get("pick"):
            p = pick.astype(np.int64)
            v["pick"] = np.where(p == F.NONE, M.PICK_NONE, p)
            assert v["pick"].max() < len(c["objects"][0][0]), "a batch pick holds gaussian ids, not batch items"
        F.check_frame(name, v, pr, owner, occ=o.get("occ"), pick=bool(o.get("pick")), what=f"batch view {name}")


# ---- the selects ----------------------------------------------------------------------------------------------------------
def test_select_mask(gsm, cuda):
    name = F.SELECT
    c = F.case_of(name)
    w, h = c["width"], c["height"]
    pr, _ = F.projection_of(name)
    scs, objects = _objects(gsm, cuda, c)
    n = scs[0].n
    r = handle(gsm, n, w, h, scs[0].prec)
    before = F.states_for(n, 53)
    g = np.nonzero(pr["visible"] & (M.styles_of(before, F.STYLES)[:, 5] == 0))[0][0]
    at = tuple(np.floor(M.round_h(pr["mean"][g]) + 0.5).astype(int))
    matched = cuda.zeros(1, dtype=cuda.int32, device="cuda")
    for what, mname, am, xm, styled in F.select_cases():
        mask = F.masks(w, h, at)[mname]
        dev = cuda.from_numpy(before.copy()).cuda()
        r.select_mask(objects[0].input, objects[0].camera, w, h, cuda.from_numpy(mask.copy()).cuda(), dev, am, xm,
                      styles=_styles(gsm, F.STYLES) if styled else None, matched=matched)
        cuda.cuda.synchronize()
        want, mcnt, doubt = M.select_mask(pr, before, mask, w, h, am, xm, styles=F.STYLES if styled else None,
                                          eps=T.BOUNDARY_EPS["mean"] * max(w, h))
        F.check_select(name, dev.cpu().numpy(), int(matched.item()), before, want, mcnt, doubt | T.left_out(pr), what)
    r.close()


def test_select_pick(gsm, cuda):
    """select_pick over the pick image of the occluded composite the handle has just rendered."""
    name = "composite_3_sh1_f16_200x150"
    c = F.case_of(name)
    w, h = c["width"], c["height"]
    counts = F.counts_of(c)
    items = len(F.projection_of(name)[1])
    scs, objects = _objects(gsm, cuda, c)
    r, _ = _handle_for(gsm, cuda, c, QUADRANT, items)
    t = Targets(cuda, w, h)
    occ = cuda.from_numpy(F.occluder_of(name, "step")).cuda()
    r.render_frame(t.color, t.depth, objects, w, h, pick=t.pick, occluder=occ, pick_pitch=t.pick_pitch)
    _, _, gp = t.read()
    assert r.blend_kernel_kind() == QUADRANT
    matched = cuda.zeros(1, dtype=cuda.int32, device="cuda")
    total = 0
    for o in (0, 2, 3):
        n = counts[o]
        before = F.states_for(n, 54 + o)
        for what, mname, am, xm, _ in F.select_cases():
            mask = F.masks(w, h)[mname]
            dev = cuda.from_numpy(before.copy()).cuda()
            r.select_pick(t.pick, w, h, o, dev, n, am, xm, mask=cuda.from_numpy(mask.copy()).cuda(), matched=matched,
                          pick_pitch=t.pick_pitch)
            cuda.cuda.synchronize()
            want, mcnt, doubt = M.select_pick(gp.astype(np.int64), counts, o, before, n, am, xm, mask=mask)
            F.check_select(name, dev.cpu().numpy(), int(matched.item()), before, want, mcnt, doubt, f"object {o} {what}")
            total += mcnt
    r.close()
    assert total > 100
