"""The oracle and the Local restatement against the float64 model (tests/f64_model.py): CPU only.

Every other test compares an implementation with a restatement of the reference's shaders written by the
same hands.  These compare the restatements with a second derivation: visibility, the packed records, the
blend order, per-tile compositing of the implementation's own lists, and the whole frame from the model
alone (projection -> record quantisation -> untiled compositing), which nothing of the oracle's enters.

Tolerances: every constant is twice the largest difference measured between the oracle and
the model over the scenes below; the measured value stands beside it.  tests/test_f64_gpu.py applies the
same checks, with the same constants, to what the HIP path returns.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_model as M  # noqa: E402
import local_scenes as LS  # noqa: E402

EPS_MARGIN = 1e-5        # cull margins closer to zero than this may fall either way in float32
MAX_LEFT_OUT = 0.01      # at most 1% of a scene may be left out of the visibility comparison
SPARSE_MAX, DENSE_MIN = 150, 400   # deepest tile list of the two depth regimes

# ---- measured float32 evaluation error of the record fields, beyond the storage step -----------------
# (units: mean / frame's longer side; depth / depth; conic / max(1/sigma^2); colour and opacity absolute)
F32 = 2.0 ** -20  # stands in where the measured excess is not positive: a few float32 ulps of the field's scale
RECORD_TOL = {
    "global": dict(mean=F32, depth=F32, conic=F32, color=F32, opacity=F32),
    # conic: measured 1.25e-4 (local_plane_ties_100x70), beyond the half ulp and the determinant's cancellation
    "local": dict(mean=F32, depth=F32, conic=2.5e-4, color=F32, opacity=F32),
}
# measured excess, largest over the scenes (global / local): mean 1.4e-8 / 9.7e-9, depth, colour and opacity
# not positive, Global conic not positive (-1.6e-5 at best): F32 stands in for all of those
# ---- measured blend differences: (check, regime) -> (rgb, alpha, depth) ------------------------------
BLEND_TOL = {
    # measured: rgb 3.44e-3 (local_sh1_f16_100x70), alpha 2.08e-3 (opaque_splat_64x64), depth 1.54e-2 (sparse_sh1_f16_200x150)
    ("lists", "sparse"): (6.9e-3, 4.2e-3, 3.1e-2),
    # measured: rgb 5.36e-3, alpha 3.58e-3, depth 2.14e-2 (all dense_sh1_f16_200x150)
    ("lists", "dense"): (1.07e-2, 7.2e-3, 4.3e-2),
    # measured: rgb 4.44e-3, alpha 5.83e-3 (local_plane_ties_100x70), depth 2.83e-2 (sparse_sh1_f16_200x150)
    ("frame", "sparse"): (8.9e-3, 1.17e-2, 5.7e-2),
    # measured: rgb 6.61e-3, alpha 3.91e-3, depth 2.56e-2 (dense_sh0_f32_128x64)
    ("frame", "dense"): (1.32e-2, 7.8e-3, 5.1e-2),
}

# name: (kind, gaussians, width, height, SH components, precision (1 = f16), colour space, seed, camera seed, kw)
SCENES = {
    "sparse_sh1_f16_200x150": ("gen", 2000, 200, 150, 4, 1, 0, 11, None, {}),
    "sparse_sh2_f32_srgb_128x64": ("gen", 450, 128, 64, 9, 0, 1, 13, None, {}),
    "sparse_sh3_f16_rolled_200x150": ("gen", 2500, 200, 150, 16, 1, 0, 14, 5, {"spread": 1.0}),
    "dense_sh0_f32_128x64": ("gen", 3000, 128, 64, 1, 0, 0, 12, None, {}),
    "dense_sh1_f16_200x150": ("gen", 8000, 200, 150, 4, 1, 0, 15, None, {}),
    "plane_ties_128x64": ("plane", 500, 128, 64, 1, 0, 0, 16, None, {}),
    "opaque_splat_64x64": ("stack", 1, 64, 64, 1, 0, 0, 17, None, {}),
}
FRAME_SCENES = [s for s in SCENES if s != "dense_sh1_f16_200x150"]  # 8000 x 30000 untiled is too slow
LOCAL_SCENES = {
    "local_sh1_f16_100x70": ("gen", 900, 100, 70, 4, 1, 0, 32, None, {}),
    "local_plane_ties_100x70": ("plane", 400, 100, 70, 1, 0, 0, 33, None, {}),
}


def make_case(spec):
    kind, n, w, h, sh, prec, cs, seed, cam_seed, kw = spec
    from gsm_amd import scenes
    if kind == "gen":
        world, harm, cam = scenes.gen_scene(n, w, h, sh, prec, seed=seed, **kw)
    elif kind == "plane":  # one view depth: every list is one run of equal keys (tie order)
        world, harm = LS.plane(n, w, h, seed)
        cam = LS.cam(w, h)
    else:  # one opaque gaussian on a pixel centre: alpha reaches the 0.99 clamp (record opacity 255); a second
        # one on top would hide the clamp, since 0.01 * 0.01 of transmittance is below fp16's step at 1
        world, harm = LS.stack(n, w, h, centre=(23.0, 23.0), sigma_px=5.0, opacity=1.0, dc=0.5, others=200,
                               seed=seed)
        cam = LS.cam(w, h)
    if cam_seed is not None:
        from test_gpu_parity import _random_camera
        cam = _random_camera(w, h, cam_seed)
    return dict(world=world, harm=harm, sh=sh, cam=cam, width=w, height=h, max_gaussians=len(world),
                color_space=cs)


@functools.lru_cache(maxsize=None)
def case_of(name):
    return make_case(SCENES[name] if name in SCENES else LOCAL_SCENES[name])


@functools.lru_cache(maxsize=None)
def projection_of(name):
    c = case_of(name)
    return M.project(c["world"], c["harm"], c["sh"], c["cam"], c["width"], c["height"], c["color_space"],
                     renderer="local" if name in LOCAL_SCENES else "global")


def global_view(render_data, mask, headers, sorted_values, color_bits, depth_bits):
    """What a Global frame returned, widened: the same for the oracle and for the HIP path."""
    col = M.h2d(color_bits)
    return dict(kind="global", rec=M.from_global_records(render_data), ids=np.arange(len(render_data)),
                mask=np.asarray(mask).astype(bool), lists=M.lists_from_headers(headers, sorted_values),
                color=col[..., :3], alpha=col[..., 3], depth=M.h2d(depth_bits),
                rules=M.GLOBAL_RULES, clear=M.GLOBAL_CLEAR)


def local_view(projected, source, mask, tile_counts, tile_lists, color_bits, depth_bits):
    """A Local frame: records are compacted (record i belongs to gaussian source[i])."""
    col = M.h2d(color_bits)
    return dict(kind="local", rec=M.from_local_records(projected), ids=np.asarray(source),
                mask=np.asarray(mask).astype(bool), lists=M.lists_from_local(tile_counts, tile_lists),
                color=col[..., :3], alpha=col[..., 3], depth=M.h2d(depth_bits),
                rules=M.LOCAL_RULES, clear=M.LOCAL_CLEAR)


@functools.lru_cache(maxsize=None)
def oracle_view(name):
    c = case_of(name)
    if name in LOCAL_SCENES:
        import local_ref
        r = local_ref.render(c["world"], c["harm"], c["sh"], c["cam"], c["width"], c["height"],
                             color_space=c["color_space"])
        assert r["status"] == 0 and r["overflow"] == 0
        return local_view(r["projected"], r["source"], r["mask"], r["tile_counts"], r["tile_lists"], r["color"],
                          r["depth"])
    import oracle as O
    r = O.render(c["world"], c["harm"], c["sh"], c["cam"], c["width"], c["height"],
                 color_space=c["color_space"])
    assert r["status"] == 0 and r["overflow"] == 0
    return global_view(r["render_data"], r["mask"], r["headers"], r["sorted_values"], r["color"], r["depth"])


def deepest(view):
    return max((len(ids) for _, ids in view["lists"]), default=0)


def regime(view):
    d = deepest(view)
    assert d <= 1000, f"deepest list {d}: beyond the depths the dense constants were measured at"
    return "sparse" if d <= SPARSE_MAX else "dense"


# ---- the checks: each measure_* returns figures, each check_* prints them and asserts ------------------
def left_out(pr):
    # (tile_doubt: a DepthFirst mono gaussian whose only passing tiles are in doubt, tests/test_f64_df_model.py)
    return (np.abs(pr["margin"]) < EPS_MARGIN) | pr["repair"] | pr.get("tile_doubt", False)


def check_visibility(pr, mask):
    out = left_out(pr)
    n = len(mask)
    print(f"visibility: {int(pr['visible'].sum())} of {n} visible in the model, {int(out.sum())} left out")
    assert out.sum() <= MAX_LEFT_OUT * n, f"{out.sum()} of {n} gaussians within eps of a cull or in a repair branch"
    bad = np.nonzero((mask != pr["visible"]) & ~out)[0]
    assert bad.size == 0, (f"{bad.size} gaussians differ, first {bad[:5].tolist()}: model margins "
                           f"{ {k: v[bad[:3]].tolist() for k, v in pr['margins'].items()} }")
    return mask & pr["visible"] & ~out


def measure_records(pr, view, w, h):
    """Per field, the largest difference beyond the storage step (<= 0: inside the step everywhere)."""
    rec, ids = view["rec"], view["ids"]
    keep = (view["mask"] & pr["visible"] & ~left_out(pr))[ids] if view["kind"] == "local" else \
        (view["mask"] & pr["visible"] & ~left_out(pr))
    g = ids[keep]
    r = {k: v[keep] for k, v in rec.items()}
    half_step = lambda v: 0.5 * M.h_ulp(v)
    out = {}
    out["mean"] = ((np.abs(r["mean"] - pr["mean"][g]) - half_step(pr["mean"][g])) / max(w, h)).max()
    out["depth"] = ((np.abs(r["depth"] - pr["depth"][g]) - half_step(pr["depth"][g])) / pr["depth"][g]).max()
    i1, i2 = 1.0 / pr["sigma"][g, 0] ** 2, 1.0 / pr["sigma"][g, 1] ** 2
    dc = np.abs(r["conic"] - pr["conic"][g])
    if view["kind"] == "global":
        # half a theta step turns the conic by at most |i2 - i1| per radian; half an fp16 ulp of a sigma
        # (2^-11 relative) moves its 1/sigma^2 by 2^-10 relative, and A, B, C are convex mixes of the two
        step = (M.PI / 65535.0 / 2.0) * np.abs(i2 - i1) + 2.0 ** -10 * i2
        # the shader takes the axis from (b, lambda1 - a) in float32.  lambda1 = mid + sqrt(mid^2 - det): the
        # subtraction under the root loses mid^2 / root^2 of its precision, so lambda1 - a is uncertain by
        # about 2^-24 mid^2 / root (four roundings allowed), and theta by that over |b| -- up to a quarter turn
        # for a nearly axis-aligned splat with a small cross term (measured: 0.11 rad at b = 4.6e-5)
        a_, b_, d_ = pr["cov2d"][g].T
        mid = 0.5 * (a_ + d_)
        root = np.sqrt(np.maximum(mid * mid - (a_ * d_ - b_ * b_), 1e-300))
        dtheta = np.minimum(4.0 * 2.0 ** -24 * mid * mid / (root * np.maximum(np.abs(b_), 1e-300)), M.PI / 2.0)
        step += dtheta * np.abs(i2 - i1)
        out["conic"] = ((dc.max(1) - step) / i2).max()
        trunc = lambda got, want: np.maximum(got - want, want - 1.0 / 255.0 - got).max()  # got in (want - 1/255, want]
        if "styled_bytes" in pr:
            # a styled projection (M.apply_styles) holds whole bytes: equal, except where the byte the style
            # started from is in doubt (the plain value within float32's reach of a truncation boundary)
            sure = ~_u8_doubt(pr["plain_color"][g], BOUNDARY_EPS["color"]).any(1)
            out["color"] = np.abs(r["color"] - pr["color"][g])[sure].max(initial=0.0)
            sure = ~_u8_doubt(pr["plain_opacity"][g], BOUNDARY_EPS["opacity"])
            out["opacity"] = np.abs(r["opacity"] - pr["opacity"][g])[sure].max(initial=0.0)
            return out
        out["color"] = trunc(r["color"], np.minimum(pr["color"][g], 1.0))
        out["opacity"] = trunc(r["opacity"], np.minimum(pr["opacity"][g], 1.0))
    else:
        # the Local conic is cov^-1 = adj / det with det = a d - b^2 formed in float32: the subtraction loses
        # a d / det of its relative precision (three roundings of 2^-24 each), and so does every entry
        a, b, d = pr["cov2d"][g].T
        cancel = (3.0 * 2.0 ** -24 * a * d / (a * d - b * b))[:, None] * np.abs(pr["conic"][g])
        out["conic"] = ((dc - half_step(pr["conic"][g]) - cancel) / i2[:, None]).max()
        out["color"] = (np.abs(r["color"] - pr["color"][g]) - half_step(pr["color"][g])).max()
        out["opacity"] = (np.abs(r["opacity"] - pr["opacity"][g]) - half_step(pr["opacity"][g])).max()
    return out


def check_records(pr, view, w, h):
    fig = measure_records(pr, view, w, h)
    print("records beyond the storage step:", {k: float(f"{v:.3g}") for k, v in fig.items()})
    for k, v in fig.items():
        assert v <= RECORD_TOL[view["kind"]][k], (k, v, RECORD_TOL[view["kind"]][k])


def check_order(pr, view, owner=None):
    """Each list ascends in (fp16(model depth) ^ 0x8000, id).  For a composite the ids are items, which ascend
    by object and then by gaussian -- the composite's tie rule; owner [items, 2] (M.project_composite) names the
    (object, gaussian) pairs in the message.  A model depth within 2^-20 relative of a
    rounding boundary (float32 evaluates clip w to about 2^-23) may round either way: such a gaussian is
    left out and the sequence is judged by the others."""
    d = pr["depth"]
    with np.errstate(invalid="ignore"):
        key = (M.h_bits(d).astype(np.int64) ^ 0x8000) & 0xFFFF
        unsure = np.abs(np.abs(d - M.round_h(d)) - 0.5 * M.h_ulp(d)) < np.abs(d) * 2.0 ** -20
    ids_of = view["ids"]
    worst = 0
    for tile, lst in view["lists"]:
        g = ids_of[lst]
        g = g[~unsure[g]]
        k = key[g] * (1 << 32) + g
        bad = np.nonzero(k[1:] <= k[:-1])[0]
        assert bad.size == 0, (f"tile {tile}: entries {bad[:3].tolist()} out of order, ids {g[bad[:3]].tolist()}"
                               + ("" if owner is None else f", (object, gaussian) {owner[g[bad[:3]]].tolist()} before "
                                  f"{owner[g[bad[:3] + 1]].tolist()}"))
        worst = max(worst, len(lst))
    print(f"order: {len(view['lists'])} lists, deepest {worst}, {int(unsure.sum())} gaussians at a rounding boundary")


def _diffs(view, model, where):
    where = where & np.isfinite(view["color"]).all(-1)
    rgb = np.abs(view["color"] - model["color"])[where].max()
    al = np.abs(view["alpha"] - model["alpha"])[where].max()
    dw = where & ~model["depth_unsure"]
    dep = np.abs(view["depth"] - model["depth"])[dw].max()
    return float(rgb), float(al), float(dep)


def measure_lists(view, w, h, lists=None, occluder=None):
    tw, th = view["rules"]["tile"]
    lists = view["lists"] if lists is None else lists
    m = M.blend_lists(view["rec"], lists, tw, th, w, h, view["clear"], view["rules"], occluder=occluder)
    if len(lists) == len(view["lists"]):  # the whole frame: the clear value outside the lists too
        where = np.ones((h, w), bool)
    else:
        where = m["covered"]
    return _diffs(view, m, where)


def _u8_doubt(v, eps):
    """v * 255 within eps * 255 of a whole number: the truncated byte may be the neighbour."""
    with np.errstate(invalid="ignore"):
        f = np.mod(np.clip(v, 0.0, 1.0) * 255.0, 1.0)
        return (np.minimum(f, 1.0 - f) / 255.0 < eps) & (v < 1.0 + eps)


def at_rounding_boundary(pr, kind, w, h):
    """Gaussians one of whose stored fields the model puts so close to a rounding boundary of the record's
    format that float32 may store the neighbouring value: mean and depth (fp16; a flipped mean moves a splat
    by up to an eighth of a pixel at these sizes, a flipped depth can swap neighbours in the order), colour
    and opacity (1/255 steps in the Global record, fp16 in the Local one).  Sigma and theta are left in: a
    flipped sigma moves alpha by at most 7e-4, a flipped theta the conic by 5e-5 of its largest entry.
    Decided from the model alone; eps is BOUNDARY_EPS."""
    tol = BOUNDARY_EPS

    def fp16(v, eps):
        return np.abs(np.abs(v - M.round_h(v)) - 0.5 * M.h_ulp(v)) < eps

    u8 = _u8_doubt
    with np.errstate(invalid="ignore"):
        near = fp16(pr["mean"], tol["mean"] * max(w, h)).any(1) | fp16(pr["depth"], tol["depth"] * np.abs(pr["depth"]))
        if kind == "global":
            # (a styled projection is judged by the values its bytes started from: the styled byte of a plain
            # byte in doubt is in doubt)
            col, opa = pr.get("plain_color", pr["color"]), pr.get("plain_opacity", pr["opacity"])
            # an opacity whose 255-fold is a whole number (1.0) is exact in float32 too: no doubt there
            near |= u8(col, tol["color"]).any(1) | \
                (u8(opa, tol["opacity"]) & (np.mod(opa * 255.0, 1.0) != 0.0))
        else:
            near |= fp16(pr["color"], tol["color"]).any(1) | fp16(pr["opacity"], tol["opacity"])
    return near & pr["visible"]


# how far float32 lands from the model, in the units of RECORD_TOL: 2.5 times the largest mean error measured
# (3.9e-8 of the frame's side), four float32 ulps for the depth (one matrix row), eight for the colour (up to
# 16 SH terms, or the sRGB power) and for the opacity times 255
BOUNDARY_EPS = dict(mean=1e-7, depth=2.0 ** -22, color=2.0 ** -21, opacity=2.0 ** -21)
MAX_PIXELS_LEFT_OUT = 0.25  # the densest scene (3000 gaussians on 128x64) leaves out 17%


def measure_frame(pr, view, w, h, occluder=None, model_out=None):
    """The model alone: projection, record quantisation, one global order, every gaussian on every pixel;
    compared over the tiles the implementation drew, less the pixels on which a gaussian at a rounding
    boundary has an alpha of 1e-3 or more (what it can change elsewhere is below 1e-3 of a neighbour's alpha).
    Under an occluder, also less the pixels on which a gaussian of alpha >= 1e-3 has a model depth within
    BOUNDARY_EPS['depth'] (relative) of the pixel's Z.  A styled projection (M.apply_styles) is quantised with
    its bytes.  model_out: a dict that receives the model's frame and the pixels compared ('where')."""
    if view["kind"] != "global":
        q = M.quantise_local(pr)
    else:
        q = M.quantise_styled(pr) if "styled_bytes" in pr else M.quantise_global(pr)
    vis = np.nonzero(pr["visible"])[0]
    if occluder is None:
        m = M.blend_untiled(q, M.depth_order(q["depth"], vis), w, h, view["clear"], view["rules"])
    else:
        m = M.blend_untiled(q, M.depth_order(q["depth"], vis), w, h, view["clear"], view["rules"],
                            occluder=occluder, surface_doubt=(pr["depth"], BOUNDARY_EPS["depth"]))
    tw, th = view["rules"]["tile"]
    tiles_x = (w + tw - 1) // tw
    drawn = np.zeros((h, w), bool)
    for t, _ in view["lists"]:
        x0, y0 = (t % tiles_x) * tw, (t // tiles_x) * th
        drawn[y0:y0 + th, x0:x0 + tw] = True
    flip = np.nonzero(at_rounding_boundary(pr, view["kind"], w, h))[0]
    ys, xs = np.mgrid[0:h, 0:w]
    unsure = np.zeros((h, w), bool)
    if flip.size:
        a = M._alphas(q, flip, xs.reshape(-1).astype(float), ys.reshape(-1).astype(float), 1.0)
        unsure = (a >= 1e-3).any(0).reshape(h, w)
    if occluder is not None:
        unsure |= m["at_surface"]
    if model_out is not None:
        model_out.update(m, where=drawn & ~unsure)
    share = float((unsure & drawn).sum()) / max(int(drawn.sum()), 1)
    print(f"whole frame: {flip.size} gaussians at a rounding boundary, {share:.2%} of the drawn pixels left out")
    assert share <= MAX_PIXELS_LEFT_OUT, share
    # outside the drawn tiles the model must have nothing to draw either
    stray = float(m["alpha"][~drawn].max()) if (~drawn).any() else 0.0
    return _diffs(view, m, drawn & ~unsure) + (stray,)


def check_blend(which, fig, view):
    tol = BLEND_TOL[(which, regime(view))]
    print(f"{which} ({regime(view)}, deepest {deepest(view)}): rgb {fig[0]:.3g} alpha {fig[1]:.3g} depth {fig[2]:.3g}"
          + (f" stray alpha {fig[3]:.3g}" if len(fig) > 3 else ""), "bounds", tol)
    assert fig[0] <= tol[0] and fig[1] <= tol[1] and fig[2] <= tol[2], (fig, tol)
    if len(fig) > 3:
        assert fig[3] <= tol[1], ("alpha outside the drawn tiles", fig[3], tol[1])


# ---- the tests -------------------------------------------------------------------------------------------
ALL = sorted(SCENES) + sorted(LOCAL_SCENES)


def test_scene_regimes(oracle):
    """The scenes cover what the issue lists: a deepest list of at most 150 and one of at least 400."""
    depths = {s: deepest(oracle_view(s)) for s in ALL}
    print(depths)
    assert all(d <= SPARSE_MAX or d >= DENSE_MIN for d in depths.values()), depths
    assert max(depths[s] for s in SCENES if s.startswith("dense")) >= DENSE_MIN
    assert all(depths[s] <= SPARSE_MAX for s in SCENES if s.startswith("sparse"))
    assert 255 in oracle_view("opaque_splat_64x64")["rec"]["opacity"] * 255  # alpha reaches the 0.99 clamp


@pytest.mark.parametrize("name", ALL)
def test_visibility(oracle, name):
    check_visibility(projection_of(name), oracle_view(name)["mask"])


@pytest.mark.parametrize("name", ALL)
def test_records(oracle, name):
    c = case_of(name)
    check_records(projection_of(name), oracle_view(name), c["width"], c["height"])


@pytest.mark.parametrize("name", ALL)
def test_order(oracle, name):
    check_order(projection_of(name), oracle_view(name))


@pytest.mark.parametrize("name", ALL)
def test_lists(oracle, name):
    c, v = case_of(name), oracle_view(name)
    check_blend("lists", measure_lists(v, c["width"], c["height"]), v)


@pytest.mark.parametrize("name", FRAME_SCENES + sorted(LOCAL_SCENES))
def test_whole_frame(oracle, name):
    c, v = case_of(name), oracle_view(name)
    check_blend("frame", measure_frame(projection_of(name), v, c["width"], c["height"]), v)


def _closed_form_harmonics(ct, phi):
    """cos/sin(|m| phi) P_l^|m|(cos theta), normalised, no Condon-Shortley phase: [..., 16] in (l, m) order,
    from the Legendre recurrences, not from the Cartesian polynomials the model uses."""
    from math import factorial
    st = np.sqrt(1.0 - ct * ct)
    P = {(0, 0): np.ones_like(ct)}
    for m in range(1, 4):
        P[(m, m)] = (2 * m - 1) * st * P[(m - 1, m - 1)]
    for m in range(0, 4):
        if m + 1 <= 3:
            P[(m + 1, m)] = (2 * m + 1) * ct * P[(m, m)]
        for l in range(m + 2, 4):
            P[(l, m)] = ((2 * l - 1) * ct * P[(l - 1, m)] - (l + m - 1) * P[(l - 2, m)]) / (l - m)
    out = []
    for l, m in M.SH_LM:
        a = abs(m)
        N = np.sqrt((2 * l + 1) / (4 * np.pi) * factorial(l - a) / factorial(l + a))
        if m == 0:
            out.append(N * P[(l, 0)])
        else:
            out.append(np.sqrt(2.0) * N * P[(l, a)] * (np.cos(a * phi) if m > 0 else np.sin(a * phi)))
    return np.stack(out, -1)


def test_sh_basis_is_orthonormal_and_signed():
    """Guards the guard: the model's 16 functions are orthonormal over the sphere (Gauss-Legendre in cos
    theta times a uniform grid in phi, exact for these polynomials) and equal the closed-form real harmonics
    times the reference's per-function signs (-1)^m."""
    x, wx = np.polynomial.legendre.leggauss(8)
    phi = np.arange(16) * (2 * np.pi / 16)
    ct, ph = np.meshgrid(x, phi, indexing="ij")
    st = np.sqrt(1 - ct * ct)
    d = np.stack([st * np.cos(ph), st * np.sin(ph), ct], -1)
    B = M.sh_basis(d)
    wgt = (wx[:, None] * (2 * np.pi / 16)) * np.ones_like(ph)
    G = np.einsum("ijk,ijl,ij->kl", B, B, wgt)
    assert np.abs(G - np.eye(16)).max() < 1e-10
    rng = np.random.default_rng(5)
    ct, ph = rng.uniform(-1, 1, 200), rng.uniform(0, 2 * np.pi, 200)
    st = np.sqrt(1 - ct * ct)
    d = np.stack([st * np.cos(ph), st * np.sin(ph), ct], -1)
    assert np.abs(M.sh_basis(d) - _closed_form_harmonics(ct, ph) * M.SH_SIGNS).max() < 1e-12
