"""The DepthFirst restatements against the float64 model (tests/f64_df_model.py): CPU only.

The three restatements of DepthFirstShaders.metal (the df_* entries of the oracle, tests/df_mono and
tests/df_options) are held to a second derivation on the five checks of tests/test_f64_model.py: visibility
(of the union, and per eye through the sentinel), every field of the records, tile membership (the union
rectangle of the stereo frame, the passing tiles of the mono frame), the depth order with its keys, and
compositing on the frame's own lists and on the whole frame from the model alone (model records, model order,
model tile membership).

Tolerances ("DepthFirst"): every constant is twice the largest difference measured between a
restatement and the model over the scenes below, per regime; the measured value stands beside it.
tests/test_f64_df_gpu.py applies the same checks, with the same constants, to what the HIP path returns.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_df_model as DF  # noqa: E402
import f64_model as M  # noqa: E402
import local_scenes as LS  # noqa: E402
import test_f64_model as T  # noqa: E402
from test_f64_model import BOUNDARY_EPS, EPS_MARGIN, F32, MAX_LEFT_OUT, MAX_PIXELS_LEFT_OUT  # noqa: E402,F401

# ---- record fields beyond the storage step (units as in test_f64_model.RECORD_TOL) ------------------------------
# stereo, measured excess, largest over the scenes: mean 5.8e-8 of the frame's side; depth, centre depth, colour and
# opacity not positive; conic not positive (-3.8e-7) with a step of half an fp16 ulp of the entry plus the axis' float32
# uncertainty (DF.theta_reach, the Global record's estimate): F32 stands in for all of them.  The estimate is not a
# bound: on a spare seed one nearly round splat (sigmas 3.02 and 2.99) had its axis 0.18 rad off where it allows 0.10
# (DESIGN.md 16).
STEREO_RECORD_TOL = dict(mean=F32, depth=F32, center_depth=F32, conic=F32, color=F32, opacity=F32)
# ---- mono tile membership ---------------------------------------------------------------------------------------
# a pair whose float64 minimum lies within this relative distance of the cutoff is in doubt.  Measured on
# df_mono_ref and df_options_ref: no pair of the committed scenes was decided otherwise than the model decides it
# (largest distance 0), so twice that is 0 and F32 stands in, as it does for the record fields
TILE_REL = F32
MAX_PAIRS_LEFT_OUT = 0.01
# ---- order ------------------------------------------------------------------------------------------------------
DEPTH_REACH = 2.0 ** -20     # relative: float32 evaluates clip w to about 2^-23 (test_f64_model.check_order)
MAX_ORDER_IN_DOUBT = 0.01    # of the list entries
# ---- the stereo rim ---------------------------------------------------------------------------------------------
# the blend forms the quadratic form in fp16: three terms of two products each and two sums, every operation
# rounded to 2^-11 relative; four roundings on the terms' magnitudes bound what reaches the comparison with 9
RIM_REACH = 4.0 * 2.0 ** -11
RIM_ALPHA = 1e-3
# ---- measured blend differences: (frame, check, regime) -> (rgb, alpha, depth) -----------------------------------
BLEND_TOL = {
    # measured: rgb 2.80e-3 (stereo_opaque_splat_64x64), alpha 1.77e-3 (stereo_sh1_f16_200x150)
    ("stereo", "lists", "sparse"): (5.6e-3, 3.5e-3, 0.0),
    # measured: rgb 6.43e-3, alpha 2.33e-3 (stereo_dense_sh0_f32_128x96)
    ("stereo", "lists", "dense"): (1.29e-2, 4.7e-3, 0.0),
    # measured: rgb 2.80e-3 (stereo_opaque_splat_64x64), alpha 1.77e-3 (stereo_sh1_f16_200x150)
    ("stereo", "frame", "sparse"): (5.6e-3, 3.5e-3, 0.0),
    # measured: rgb 6.43e-3, alpha 2.33e-3 (stereo_dense_sh0_f32_128x96)
    ("stereo", "frame", "dense"): (1.29e-2, 4.7e-3, 0.0),
    # measured: rgb 2.64e-3, depth 1.58e-2 (mono_sh1_f16_200x150), alpha 5.04e-3 (mono_low_opacity_200x150)
    ("mono", "lists", "sparse"): (5.3e-3, 1.01e-2, 3.2e-2),
    # measured: rgb 5.27e-3, alpha 3.35e-3, depth 1.79e-2 (mono_dense_sh0_f32_128x64)
    ("mono", "lists", "dense"): (1.05e-2, 6.7e-3, 3.6e-2),
    # measured: rgb 2.64e-3, depth 1.58e-2 (mono_sh1_f16_200x150), alpha 5.04e-3 (mono_low_opacity_200x150)
    ("mono", "frame", "sparse"): (5.3e-3, 1.01e-2, 3.2e-2),
    # measured: rgb 4.49e-3, alpha 2.57e-3, depth 9.50e-3 (mono_dense_sh0_f32_128x64)
    ("mono", "frame", "dense"): (9.0e-3, 5.1e-3, 1.9e-2),
}

WIDE_IPD = 3.0               # the wide-baseline pair: eyes 3 scene units apart
MIN_ONE_EYE = 200            # ... must leave at least this many gaussians visible in one eye only
# name: (kind, gaussians, width, height, SH components, precision (1 = f16), colour space, seed, options)
STEREO_SCENES = {
    "stereo_sh1_f16_200x150": ("gen", 2000, 200, 150, 4, 1, 0, 41, {}),
    "stereo_dense_sh0_f32_128x96": ("gen", 3000, 128, 96, 1, 0, 0, 42, {"kw": {"spread": 0.05}}),
    "stereo_wide_sh2_f16_200x150": ("gen", 2000, 200, 150, 9, 1, 0, 43, {"ipd": WIDE_IPD}),
    "stereo_sh3_f16_srgb_transform_200x150": ("gen", 2500, 200, 150, 16, 1, 1, 46, {"transform": True}),
    "stereo_opaque_splat_64x64": ("stack", 1, 64, 64, 1, 0, 0, 45, {}),
    "stereo_plane_key16_128x64": ("ties", 500, 128, 64, 1, 0, 0, 46, {"bits": (16, 32)}),
}
MONO_SCENES = {
    "mono_sh1_f16_200x150": ("gen", 2000, 200, 150, 4, 1, 0, 51, {}),
    "mono_dense_sh0_f32_128x64": ("gen", 3000, 128, 64, 1, 0, 0, 54, {}),
    "mono_low_opacity_200x150": ("gen", 3000, 200, 150, 1, 1, 0, 53, {"kw": {"scale_px": 3.0}, "opacity": (0.005, 0.05)}),
    "mono_far_inside_200x150": ("gen", 2000, 200, 150, 4, 1, 0, 54, {"far": 6.0}),
    "mono_plane_key16_128x64": ("ties", 500, 128, 64, 1, 0, 0, 55, {"bits": (16, 32)}),
}
ALL = sorted(STEREO_SCENES) + sorted(MONO_SCENES)
IPD = 0.064


def ties_plane(n, w, h, seed):
    """LS.plane with view depths 5 + (k + 1/2) 2^-12, k a permutation of the ids: sixteen consecutive depths share one
    fp16 value (the fp16 step at 5 is 2^-8), and inside such a run ascending id is not ascending depth."""
    world, harm = LS.plane(n, w, h, seed)
    k = np.random.default_rng(seed + 3).permutation(n).astype(np.float32)
    # (the half keeps every depth off the fp16 ties, which lie at odd multiples of 2^-9)
    world["pz"] = np.float32(5.0) + (k + np.float32(0.5)) * np.float32(2.0 ** -12)
    return world, harm


def scene_transform():
    """test_depthfirst._scene_transform() (rotation about y, scale 1.25, a translation) with its second and third
    columns scaled by 0.8 and 1.1: the columns have the lengths 1.25, 1.0 and 1.375, so the one the gaussians'
    scales are multiplied by cannot be mistaken for another (a uniform scale gives every row and column one length)."""
    from test_depthfirst import _scene_transform
    S = _scene_transform().reshape(4, 4).copy()  # row k holds column k
    S[1, :3] *= np.float32(0.8)
    S[2, :3] *= np.float32(1.1)
    return S.reshape(-1)


def make_case(name, spec, seed_shift=0):
    from gsm_amd import scenes
    kind, n, w, h, sh, prec, cs, seed, opt = spec
    seed += seed_shift
    stereo = name.startswith("stereo")
    ipd = opt.get("ipd", IPD)
    if kind == "gen":
        world, harm, _ = scenes.gen_scene(n, w, h, sh, prec, seed=seed, **opt.get("kw", {}))
    elif kind == "ties":
        world, harm = ties_plane(n, w, h, seed)
    else:  # one opaque gaussian whose mean lands on the coordinate (23, 23) of the (left) eye, sigma 5 pixels: the
        # 0.99 clamp at its centre and the r^2 = 9 rim fifteen pixels out, across several tiles
        world, harm = LS.stack(n, w, h, centre=(22.5, 22.5), sigma_px=5.0, opacity=1.0, dc=0.5, others=200, seed=seed)
        if stereo:
            world["px"][:n] -= np.float32(ipd / 2)
    if "opacity" in opt:  # uniform over the range; the f16 world stores fp16 bits
        lo, hi = opt["opacity"]
        op = np.random.default_rng(seed + 5).uniform(lo, hi, n).astype(np.float32)
        world["opacity"] = op.astype(np.float16).view(np.uint16) if prec == 1 else op
    c = dict(world=world, harm=harm, sh=sh, width=w, height=h, color_space=cs, bits=opt.get("bits", (32, 16)),
             stereo=stereo, transform=None)
    if stereo:
        c["cams"] = (scenes.make_camera(w, h, -ipd / 2), scenes.make_camera(w, h, ipd / 2))
        if opt.get("transform"):
            c["transform"] = scene_transform()
    else:
        c["cam"] = scenes.make_camera(w, h, 0.0)
        if "far" in opt:
            c["cam"]["far"] = opt["far"]
    return c


@functools.lru_cache(maxsize=None)
def case_of(name, seed_shift=0):
    return make_case(name, (STEREO_SCENES if name in STEREO_SCENES else MONO_SCENES)[name], seed_shift)


@functools.lru_cache(maxsize=None)
def projection_of(name, seed_shift=0):
    c = case_of(name, seed_shift)
    if c["stereo"]:
        return DF.project_stereo(c["world"], c["harm"], c["sh"], c["cams"][0], c["cams"][1], c["width"], c["height"],
                                 c["color_space"], c["transform"], eps=EPS_MARGIN)
    return DF.project_mono(c["world"], c["harm"], c["sh"], c["cam"], c["width"], c["height"], c["color_space"],
                           rel=TILE_REL, eps=EPS_MARGIN)


# ---- what a frame returned, widened: the same for a restatement and for the HIP path ------------------------------
def _common_view(r, w, key_bits):
    tiles = np.repeat(np.arange(len(r["headers"])), r["headers"][:, 1])
    assert len(tiles) == len(r["inst_gids"]) and np.array_equal(tiles, r["inst_tiles"])
    sorted_keys = r["sorted_keys"] if "sorted_keys" in r else r["depth_keys"][r["depth_order"]]
    return dict(ids=np.arange(len(r["render_data"])), mask=np.asarray(r["touched"]) > 0, bounds=np.asarray(r["bounds"]),
                touched=np.asarray(r["touched"]), lists=M.lists_from_headers(r["headers"], r["inst_gids"]),
                pairs=np.asarray(r["inst_gids"], np.int64) * len(r["headers"]) + tiles, tile_count=len(r["headers"]),
                depth_order=np.asarray(r["depth_order"]), sorted_keys=np.asarray(sorted_keys, np.int64),
                key_bits=key_bits, clear=DF.CLEAR)


def stereo_view(r, w, h, key_bits=32):
    v = _common_view(r, w, key_bits)
    col = M.h2d(DF.split_side_by_side(r["color"], w))
    v.update(kind="stereo", frame="stereo", eyes=DF.from_stereo_records(r["render_data"]), color=col[..., :3],
             alpha=col[..., 3], rules=DF.STEREO_RULES)
    return v


def mono_view(r, w, h, key_bits=32):
    v = _common_view(r, w, key_bits)
    col = M.h2d(r["color"])
    v.update(kind="global", frame="mono", rec=M.from_global_records(r["render_data"]), color=col[..., :3],
             alpha=col[..., 3], depth=M.h2d(r["depth"]), rules=DF.MONO_RULES)
    return v


def restatement_frame(c):
    """The frame of the restatement that covers the case: the oracle's df entry or df_mono_ref at the default
    options, df_options_ref otherwise."""
    w, h, bits = c["width"], c["height"], c["bits"]
    if c["stereo"]:
        L, R = c["cams"]
        if bits == (32, 16):
            import oracle as O
            r = O.df_render_stereo(c["world"], c["harm"], c["sh"], L, R, w, h, scene_transform=c["transform"],
                                   color_space=c["color_space"], max_gaussians=8 * len(c["world"]))
        else:
            import df_options_ref
            r = df_options_ref.render_stereo(c["world"], c["harm"], c["sh"], L, R, w, h, bits[0], bits[1],
                                             scene_transform=c["transform"], color_space=c["color_space"],
                                             max_gaussians=8 * len(c["world"]), eye_color=False)
    elif bits == (32, 16):
        import df_mono_ref
        r = df_mono_ref.render(c["world"], c["harm"], c["sh"], c["cam"], w, h, color_space=c["color_space"],
                               max_gaussians=8 * len(c["world"]))
    else:
        import df_options_ref
        r = df_options_ref.render_mono(c["world"], c["harm"], c["sh"], c["cam"], w, h, bits[0], bits[1],
                                       color_space=c["color_space"], max_gaussians=8 * len(c["world"]))
    assert r["status"] == 0 and r["overflow"] == 0
    return r


@functools.lru_cache(maxsize=None)
def restatement_view(name, seed_shift=0):
    c = case_of(name, seed_shift)
    r = restatement_frame(c)
    return (stereo_view if c["stereo"] else mono_view)(r, c["width"], c["height"], c["bits"][0])


# ---- visibility --------------------------------------------------------------------------------------------------
def check_visibility(pr, view):
    """The union (or the mono gaussian with its tile test); then each eye through the sentinel."""
    keep = T.check_visibility(pr, view["mask"])
    if view["frame"] == "stereo":
        for e, rec in enumerate(view["eyes"]):
            bad = np.nonzero(keep & (rec["visible"] != pr["eye_visible"][e]))[0]
            assert bad.size == 0, (f"eye {e}: {bad.size} gaussians differ, first {bad[:5].tolist()}, margins "
                                   f"{pr['eyes'][e]['margin'][bad[:5]].tolist()}")
        print("one eye only:", int((keep & (pr["eye_visible"][0] != pr["eye_visible"][1])).sum()))
    return keep


# ---- records -----------------------------------------------------------------------------------------------------
def measure_stereo_records(ps, view, w, h):
    """Per field, the largest difference beyond the storage step over both eyes; the fields of an eye that is
    not visible must hold the sentinel (-inf means, zero conic and depth) exactly."""
    keep = view["mask"] & ps["visible"] & ~T.left_out(ps)
    half_step = lambda v: 0.5 * M.h_ulp(v)
    out = dict(mean=-np.inf, depth=-np.inf, conic=-np.inf)
    for e, (rec, pr) in enumerate(zip(view["eyes"], ps["eyes"])):
        g = np.nonzero(keep & ps["eye_visible"][e])[0]
        out["mean"] = max(out["mean"], ((np.abs(rec["mean"][g] - pr["mean"][g]) - half_step(pr["mean"][g])) / max(w, h)).max())
        out["depth"] = max(out["depth"], ((np.abs(rec["depth"][g] - pr["depth"][g]) - half_step(pr["depth"][g]))
                                          / pr["depth"][g]).max())
        i1, i2 = 1.0 / pr["sigma"][g, 0] ** 2, 1.0 / pr["sigma"][g, 1] ** 2
        # stored: half(Cxx), half(Cyy), half(2 Cxy); compared as (A, B, C), so B carries half the step of 2 B
        step = np.stack([half_step(pr["conic"][g, 0]), 0.5 * half_step(2.0 * pr["conic"][g, 1]),
                         half_step(pr["conic"][g, 2])], 1)
        # the conic goes through theta (conicFromThetaSigmas of the float32 axis): the Global record's cancellation
        step += (DF.theta_reach(pr)[g] * np.abs(i2 - i1))[:, None]
        out["conic"] = max(out["conic"], ((np.abs(rec["conic"][g] - pr["conic"][g]) - step) / i2[:, None]).max())
        gone = np.nonzero(keep & ~ps["eye_visible"][e])[0]
        assert np.all(np.isneginf(rec["raw_mean"][gone])) and not rec["conic"][gone].any() and not rec["depth"][gone].any(), \
            f"eye {e}: a record without the sentinel"
    g = np.nonzero(keep)[0]
    cd = view["eyes"][0]["center_depth"][g]
    out["center_depth"] = ((np.abs(cd - ps["center_depth"][g]) - half_step(ps["center_depth"][g])) / ps["center_depth"][g]).max()
    trunc = lambda got, want: np.maximum(got - want, want - 1.0 / 255.0 - got).max()  # got in (want - 1/255, want]
    out["color"] = trunc(view["eyes"][0]["color"][g], np.minimum(ps["color"][g], 1.0))
    out["opacity"] = trunc(view["eyes"][0]["record_opacity"][g], np.minimum(ps["opacity"][g], 1.0))
    return out


def check_records(pr, view, w, h):
    if view["frame"] == "mono":
        return T.check_records(pr, view, w, h)
    fig = measure_stereo_records(pr, view, w, h)
    print("records beyond the storage step:", {k: float(f"{v:.3g}") for k, v in fig.items()})
    for k, v in fig.items():
        assert v <= STEREO_RECORD_TOL[k], (k, v, STEREO_RECORD_TOL[k])


# ---- tile membership ---------------------------------------------------------------------------------------------
def model_pairs(pr, view, w):
    """(sure pairs, pairs in doubt, gaussians judged) of the model as gaussian * tile_count + tile."""
    keep = view["mask"] & pr["visible"] & ~T.left_out(pr)
    tc = view["tile_count"]
    if view["frame"] == "stereo":
        keep &= ~pr["rect_doubt"]
        g, t = DF.rect_pairs(pr["rect"], np.nonzero(keep)[0], w)
        return g * tc + t, np.zeros(0, np.int64), keep
    keep &= ~pr["rect_doubt"]
    p = pr["pairs"]
    k = keep[p["gaussian"]]
    code = p["gaussian"] * tc + p["tile"]
    return code[k & p["passes"] & ~p["doubt"]], code[k & p["doubt"]], keep


def measure_tile_doubt(pr, view):
    """Mono: the largest relative distance from the cutoff at which the frame decided otherwise than the model
    (computed with no doubt allowed), over the gaussians both keep."""
    p = pr["pairs"]
    keep = (view["mask"] & pr["culls_pass"] & ~pr["rect_doubt"] & (np.abs(pr["margin"]) >= EPS_MARGIN))[p["gaussian"]]
    code = p["gaussian"] * view["tile_count"] + p["tile"]
    differs = keep & (np.isin(code, view["pairs"]) != p["passes"])
    rel = np.abs(p["qmin"] - p["cutoff"]) / np.abs(p["cutoff"])
    return float(rel[differs].max(initial=0.0)), int(differs.sum())


def check_membership(pr, view, w):
    sure, doubt, keep = model_pairs(pr, view, w)
    frame = view["pairs"][keep[view["pairs"] // view["tile_count"]]]
    if view["frame"] == "stereo":
        share = float(pr["rect_doubt"].sum()) / max(int(pr["visible"].sum()), 1)
        g = np.nonzero(keep)[0]
        bad = g[(view["bounds"][g] != pr["rect"][g]).any(1)]
        assert bad.size == 0, (f"{bad.size} union rectangles differ, first {bad[:3].tolist()}: "
                               f"{view['bounds'][bad[:3]].tolist()} against {pr['rect'][bad[:3]].tolist()}")
        print(f"membership: {len(sure)} pairs, {share:.2%} of the gaussians with an edge in doubt")
    else:
        rel, n = measure_tile_doubt(pr, view)
        total = int(pr["culls_pass"][pr["pairs"]["gaussian"]].sum())
        share = (len(doubt) + int(pr["rect_doubt"][pr["pairs"]["gaussian"]].sum())) / max(total, 1)
        pruned = 1.0 - float(pr["pairs"]["passes"].sum()) / max(total, 1)
        print(f"membership: {len(sure)} sure pairs, {share:.2%} in doubt, {pruned:.1%} of the rectangles' tiles pruned; "
              f"the frame decided {n} otherwise, furthest {rel:.3g} (relative) from the cutoff")
    assert share <= MAX_PAIRS_LEFT_OUT, share
    missing = np.setdiff1d(sure, frame)
    extra = np.setdiff1d(frame, np.union1d(sure, doubt))
    tc = view["tile_count"]
    assert missing.size == 0 and extra.size == 0, \
        (f"{missing.size} pairs of the model missing, first (gaussian, tile) {[divmod(int(x), tc) for x in missing[:3]]}; "
         f"{extra.size} pairs the model does not have, first {[divmod(int(x), tc) for x in extra[:3]]}")


# ---- order -------------------------------------------------------------------------------------------------------
def check_order(pr, view):
    """The sorted keys are the model's keys of the depth order, and every list ascends in (key, id).  Two
    neighbours whose model depths differ by less than float32's reach may stand in either order; with 16-bit keys
    a depth within that reach of an fp16 rounding boundary may take either key."""
    d, bits = pr["depth"], view["key_bits"]
    key = DF.depth_keys(d, bits)
    with np.errstate(invalid="ignore"):
        unsure = np.abs(np.abs(d - M.round_h(d)) - 0.5 * M.h_ulp(d)) < np.abs(d) * DEPTH_REACH if bits == 16 \
            else np.zeros(len(d), bool)
    order = view["depth_order"]
    got = view["sorted_keys"]
    assert len(got) == len(order)
    if bits == 16:
        bad = np.nonzero((got != key[order]) & ~unsure[order])[0]
        assert bad.size == 0, f"{bad.size} sorted 16-bit keys differ, first {got[bad[:3]].tolist()} for {key[order][bad[:3]].tolist()}"
    else:  # the 32-bit key is the float32 depth's bits with the sign bit set: compare as depths
        assert np.all(got >= 0x80000000), "a 32-bit key of a positive depth without its sign bit"
        back = (got ^ 0x80000000).astype(np.uint32).view(np.float32).astype(np.float64)
        worst = np.abs(back - d[order]) / d[order]
        assert worst.max(initial=0.0) <= DEPTH_REACH, ("sorted 32-bit keys against the model's depths", worst.max())
    entries = doubt = 0
    for tile, lst in view["lists"]:
        k = key[lst]
        bad = np.nonzero((k[1:] < k[:-1]) | ((k[1:] == k[:-1]) & (lst[1:] <= lst[:-1])))[0]
        near = (np.abs(d[lst[bad]] - d[lst[bad + 1]]) < np.abs(d[lst[bad]]) * DEPTH_REACH) | unsure[lst[bad]] | unsure[lst[bad + 1]]
        assert near.all(), f"tile {tile}: entries {bad[~near][:3].tolist()} out of order, ids {lst[bad[~near][:3]].tolist()}"
        entries, doubt = entries + len(lst), doubt + int(near.sum())
    print(f"order: {len(view['lists'])} lists, {entries} entries, {doubt} neighbours within float32's reach, "
          f"{int(unsure.sum())} gaussians at a key's rounding boundary")
    assert doubt <= MAX_ORDER_IN_DOUBT * max(entries, 1), (doubt, entries)


# ---- compositing -------------------------------------------------------------------------------------------------
def _diffs(view, model, where):
    """(rgb, alpha, depth) largest differences over `where`; the frame must be finite everywhere."""
    assert np.isfinite(view["color"]).all() and np.isfinite(view["alpha"]).all(), "the frame holds a non-finite value"
    if view["frame"] == "stereo":
        mc, ma = np.stack([m["color"] for m in model]), np.stack([m["alpha"] for m in model])
        return (float(np.abs(view["color"] - mc)[where].max(initial=0.0)), float(np.abs(view["alpha"] - ma)[where].max(initial=0.0)), 0.0)
    return (float(np.abs(view["color"] - model["color"])[where].max(initial=0.0)),
            float(np.abs(view["alpha"] - model["alpha"])[where].max(initial=0.0)),
            float(np.abs(view["depth"] - model["depth"])[where].max(initial=0.0)))


class Rim:
    """Collects, while a stereo frame is blended, the pixels where an entry that the walk reaches has an alpha of
    RIM_ALPHA or more (before the cutoff) and a quadratic form within fp16's reach of 9; and the groups in which
    one eye stops before the other."""

    def __init__(self, records, w, h):
        self.rec, self.w, self.h = records, w, h
        self.rim = np.zeros((2, h, w), bool)
        self.stops = {}

    def __call__(self, eye, tile, ids, xs, ys, alpha, live):
        rec = self.rec[eye]
        t = M._power_terms(rec, ids, M.round_h(xs), M.round_h(ys))
        power, size = sum(t), sum(np.abs(x) for x in t)
        with np.errstate(over="ignore", invalid="ignore"):
            a = rec["opacity"][ids][:, None] * np.exp(-0.5 * power)
        hit = (live & (a >= RIM_ALPHA) & (np.abs(power - DF.R2_MAX) <= RIM_REACH * size)).any(0)
        inside = (xs < self.w) & (ys < self.h)
        self.rim[eye, ys[inside], xs[inside]] = hit[inside]
        self.stops[(tile, eye)] = live.sum(0).reshape(DF.TILE, DF.TILE)[::2, ::2]  # entries walked, per 2x2 group

    def uneven_groups(self, lists):
        """Groups where one eye's walk ends at least eight entries before the other's (and before the list's end)."""
        n = 0
        for tile, ids in lists:
            if (tile, 0) in self.stops:
                a, b = self.stops[(tile, 0)], self.stops[(tile, 1)]
                n += int(((np.abs(a - b) >= 8) & (np.minimum(a, b) < len(ids))).sum())
        return n


def measure_lists(view, w, h):
    """The frame's own records and lists through the model's blend, over the whole frame (clear value included).
    Stereo: less the rim pixels, at most MAX_PIXELS_LEFT_OUT of the frame."""
    if view["frame"] == "mono":
        m = DF.blend_mono(view["rec"], view["lists"], w, h)
        return _diffs(view, m, np.ones((h, w), bool)), None
    rim = Rim(view["eyes"], w, h)
    m = DF.blend_stereo(view["eyes"], view["lists"], w, h, on_tile=rim)
    share = float(rim.rim.sum()) / max(2 * int(m[0]["covered"].sum()), 1)
    print(f"lists: {share:.2%} of the drawn pixels on a rim")
    assert share <= MAX_PIXELS_LEFT_OUT, share
    return _diffs(view, m, ~rim.rim), rim


def measure_frame(pr, view, w, h):
    """The model alone: its visible set, its records quantised to the record format, its order, and every
    gaussian on every tile the model assigns it.  A pair in doubt (mono), the rectangle of a gaussian with an
    edge in doubt (stereo) and the visibility of a gaussian within eps of a cull are taken from the frame.  Left
    out: pixels where a gaussian at a rounding boundary of the record has an alpha of 1e-3 or more, and the
    stereo rim; at most MAX_PIXELS_LEFT_OUT of the drawn pixels."""
    out = T.left_out(pr)
    vis = np.where(out, view["mask"], pr["visible"])
    ids = np.nonzero(vis)[0]
    order = DF.depth_order(pr["depth"], ids, view["key_bits"])
    tc = view["tile_count"]
    frame_pairs = view["pairs"]
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs.reshape(-1).astype(float), ys.reshape(-1).astype(float)

    def touched_by(rec, flip):
        if not flip.size:
            return np.zeros((h, w), bool)
        return (M._alphas(rec, flip, fx, fy, 1.0) >= 1e-3).any(0).reshape(h, w)
    if view["frame"] == "mono":
        q, p = pr["record"], pr["pairs"]
        code = p["gaussian"] * tc + p["tile"]
        own = vis & ~pr["rect_doubt"] & ~out
        member = np.where(p["doubt"], np.isin(code, frame_pairs), p["passes"]) & own[p["gaussian"]]
        theirs = frame_pairs[(vis & ~own)[frame_pairs // tc]]
        lists = DF.lists_from_pairs(np.concatenate([p["gaussian"][member], theirs // tc]),
                                    np.concatenate([p["tile"][member], theirs % tc]), order)
        m = DF.blend_mono(q, lists, w, h)
        flip = np.nonzero(T.at_rounding_boundary(dict(pr, visible=vis), "global", w, h))[0]
        unsure = touched_by(q, flip)
        drawn = m["covered"]
    else:
        q = DF.quantise_stereo(dict(pr, eye_visible=pr["eye_visible"] & vis[None]))
        own = vis & ~pr["rect_doubt"] & ~out
        g, t = DF.rect_pairs(pr["rect"], np.nonzero(own)[0], w)
        theirs = frame_pairs[(vis & ~own)[frame_pairs // tc]]
        lists = DF.lists_from_pairs(np.concatenate([g, theirs // tc]), np.concatenate([t, theirs % tc]), order)
        rim = Rim(q, w, h)
        m = DF.blend_stereo(q, lists, w, h, on_tile=rim)
        unsure = rim.rim.copy()
        for e in range(2):
            eye = dict(pr["eyes"][e], depth=pr["center_depth"], visible=q[e]["visible"])
            unsure[e] |= touched_by(q[e], np.nonzero(T.at_rounding_boundary(eye, "global", w, h))[0])
        drawn = np.stack([m[0]["covered"], m[1]["covered"]])
    share = float((unsure & drawn).sum()) / max(int(drawn.sum()), 1)
    print(f"whole frame: {share:.2%} of the drawn pixels left out")
    assert share <= MAX_PIXELS_LEFT_OUT, share
    return _diffs(view, m, ~unsure)


DEEPEST_MAX = 3000  # the deepest list the dense constants were measured at is 2913 (stereo_dense_sh0_f32_128x96)


def regime(view):
    d = T.deepest(view)
    assert d <= DEEPEST_MAX, f"deepest list {d}: beyond the depths the dense constants were measured at"
    return "sparse" if d <= T.SPARSE_MAX else "dense"


def check_blend(which, fig, view):
    tol = BLEND_TOL[(view["frame"], which, regime(view))]
    print(f"{view['frame']} {which} ({regime(view)}, deepest {T.deepest(view)}): rgb {fig[0]:.3g} alpha {fig[1]:.3g} "
          f"depth {fig[2]:.3g}", "bounds", tol)
    assert fig[0] <= tol[0] and fig[1] <= tol[1] and fig[2] <= tol[2], (fig, tol)


def check_all(name, pr, view, frame=True):
    """Every check on one frame; tests/test_f64_df_gpu.py runs this on what the HIP path returns."""
    c = case_of(name)
    w, h = c["width"], c["height"]
    check_visibility(pr, view)
    check_records(pr, view, w, h)
    check_membership(pr, view, w)
    check_order(pr, view)
    check_blend("lists", measure_lists(view, w, h)[0], view)
    if frame:
        check_blend("frame", measure_frame(pr, view, w, h), view)


# ---- the tests ---------------------------------------------------------------------------------------------------
def test_scenes_hold_what_they_are_for(oracle):
    """Each scene's reason for being here, asserted on the model alone."""
    ps = projection_of("stereo_wide_sh2_f16_200x150")
    one_eye = int((ps["visible"] & (ps["eye_visible"][0] != ps["eye_visible"][1])).sum())
    assert one_eye >= MIN_ONE_EYE, one_eye
    # one eye of a group saturates well before the other
    c, v = case_of("stereo_dense_sh0_f32_128x96"), restatement_view("stereo_dense_sh0_f32_128x96")
    rim = measure_lists(v, c["width"], c["height"])[1]
    uneven = rim.uneven_groups(v["lists"])
    print("one-eye-only gaussians", one_eye, "groups with uneven walks", uneven)
    assert uneven >= 50, uneven
    # the opaque splat reaches the 0.99 clamp (record opacity 255) in both eyes and has its rim inside the frame
    ps = projection_of("stereo_opaque_splat_64x64")
    assert ps["eye_visible"][:, 0].all() and ps["opacity"][0] == 1.0
    assert np.abs(ps["eyes"][0]["mean"][0] - 23.0).max() < 1e-3 and 3.0 * ps["eyes"][0]["sigma"][0, 0] < 23.0
    # 16-bit keys: many gaussians share an fp16 depth whose float32 depths differ
    for name in ("stereo_plane_key16_128x64", "mono_plane_key16_128x64"):
        pr = projection_of(name)
        g = np.nonzero(pr["visible"])[0]
        k16, k32 = DF.depth_keys(pr["depth"][g], 16), DF.depth_keys(pr["depth"][g], 32)
        assert len(g) - len(np.unique(k16)) >= 200 and len(np.unique(k32)) == len(g)
        assert not np.array_equal(DF.depth_order(pr["depth"], g, 16), DF.depth_order(pr["depth"], g, 32))
    # low opacities: more than half of the rectangles' tiles pruned, and byte-1 opacities (a negative cutoff) among
    # the gaussians that pass the culls
    pr = projection_of("mono_low_opacity_200x150")
    p = pr["pairs"]
    assert p["passes"].mean() < 0.5, p["passes"].mean()
    byte1 = pr["culls_pass"] & (pr["record"]["opacity"] * 255.0 == 1.0)
    assert byte1.sum() >= 10 and np.all(p["cutoff"][byte1[p["gaussian"]]] < 0.0) and not pr["visible"][byte1].any()
    # the far plane inside the cloud culls a share of it, and nothing else would have
    pr = projection_of("mono_far_inside_200x150")
    m = pr["margins"]
    by_far = (m["far"] <= 0.0) & (np.min(np.stack([v for k, v in m.items() if k != "far"], 1), 1) > 0.0)
    assert by_far.mean() > 0.2, by_far.mean()
    # the transform scene scales by a length that no other column of the matrix shares (and no row: the nearest one
    # is 0.4% off, eight times the fp16 step of a conic entry)
    S = np.asarray(scene_transform(), np.float64).reshape(4, 4).T
    cols, rows = np.linalg.norm(S[:3, :3], axis=0), np.linalg.norm(S[:3, :3], axis=1)
    assert abs(cols[0] - 1.25) < 1e-6 and np.all(np.abs(cols[1:] - 1.25) > 0.05) and np.all(np.abs(rows - 1.25) > 0.004), \
        (cols, rows)


def test_min_quadratic_over_rect_against_a_grid():
    """Guards the guard: the closed form against a brute-force search over a fine grid of the rectangle."""
    rng = np.random.default_rng(3)
    for _ in range(40):
        th, s1, s2 = rng.uniform(0, np.pi), rng.uniform(1, 6), rng.uniform(0.5, 3)
        conic = M.conic_from_theta_sigmas(th, s1, s2)
        x0, y0 = rng.uniform(-30, 20, 2)
        got = DF.min_quadratic_over_rect(conic, x0, x0 + 16.0, y0, y0 + 16.0)
        xs, ys = np.meshgrid(np.linspace(x0, x0 + 16.0, 801), np.linspace(y0, y0 + 16.0, 801))
        brute = (conic[0] * xs * xs + 2 * conic[1] * xs * ys + conic[2] * ys * ys).min()
        assert got <= brute + 1e-12 and brute - got <= 2e-3 * max(brute, 1.0), (got, brute)


@pytest.mark.parametrize("name", ALL)
def test_visibility(oracle, name):
    check_visibility(projection_of(name), restatement_view(name))


@pytest.mark.parametrize("name", ALL)
def test_records(oracle, name):
    c = case_of(name)
    check_records(projection_of(name), restatement_view(name), c["width"], c["height"])


@pytest.mark.parametrize("name", ALL)
def test_tile_membership(oracle, name):
    check_membership(projection_of(name), restatement_view(name), case_of(name)["width"])


@pytest.mark.parametrize("name", ALL)
def test_order(oracle, name):
    check_order(projection_of(name), restatement_view(name))


@pytest.mark.parametrize("name", ALL)
def test_lists(oracle, name):
    c, v = case_of(name), restatement_view(name)
    check_blend("lists", measure_lists(v, c["width"], c["height"])[0], v)


@pytest.mark.parametrize("name", ALL)
def test_whole_frame(oracle, name):
    c, v = case_of(name), restatement_view(name)
    check_blend("frame", measure_frame(projection_of(name), v, c["width"], c["height"]), v)
