"""The float64 model extended to the two DepthFirst frames (TEST INFRASTRUCTURE).

tests/f64_model.py holds the mathematics (projection, covariance, harmonics, compositing); this file adds only
what DepthFirstShaders.metal, GaussianShared.h and DepthFirstStereoCopyEncoder.swift fix for the DepthFirst
frames and Global does not share (DESIGN.md 16 lists each): the screen mapping without the half-pixel shift,
the far-plane cull, two eyes projected in one pass with the ink cull, the centre depth and the colour decided
for the pair, the scene transform, the stereo record with its conic and its sentinel, the union tile rectangle,
the mono tile test against -2 ln(tau / opacity), the 32-bit and 16-bit depth orders, 16x16 tiles with 2x2
groups, the r^2 <= 9 cutoff of the stereo blend, alpha written as 1 - T, and the row flip of the copy pass.
It imports nothing from oracle/, loads no shared library and reads no file.
"""
from __future__ import annotations

import numpy as np

import f64_model as M

TILE = 16                    # both DepthFirst frames bin and blend 16x16 tiles
TAU = M.ALPHA_THRESHOLD      # the mono tile test keeps a tile whose largest alpha can reach this
R2_MAX = 9.0                 # the stereo blend writes alpha 0 beyond this quadratic form
MONO_RULES = dict(tile=(TILE, TILE), group=(2, 2), break_below=1.0 / 255.0, alpha_max=0.99, depth="blend")
STEREO_RULES = dict(MONO_RULES, r2_max=R2_MAX)
CLEAR = (0.0, 0.0, 0.0, 1.0)  # clearRenderTexturesKernel / clearStereoRenderTextureKernel; depth 0
SENTINEL_BELOW = -60000.0    # an eye whose meanX is below this is not visible (stored: half(-1e10) = -inf)


# ---------------------------------------------------------------------------------------------------
# projection
# ---------------------------------------------------------------------------------------------------
def project_eye(world, harm, sh, cam, w, h, color_space=0, scene_transform=None, sh_center=None, ink=True):
    """One eye: M.project with the DepthFirst conventions.  ink=False leaves the ink cull to the caller (the
    stereo frame decides it for the pair)."""
    pr = M.project(world, harm, sh, cam, w, h, color_space, renderer="depthfirst",
                   scene_transform=scene_transform, sh_center=sh_center)
    if not ink:
        pr["margins"].pop("ink")
        pr["margin"] = np.min(np.stack(list(pr["margins"].values()), 1), 1)
        pr["visible"] = pr["margin"] > 0.0
    return pr


def tile_rect(mean, extent, w, h):
    """[n, 4] (first column, last column, first row, last row) of the tiles the reference assigns to the box
    mean +- extent: the box is clamped to [0, size - 1], the first tile is floor(lo / 16), the last one
    ceil(hi / 16) - 1 (a box that ends exactly on a tile's first coordinate does not reach that tile)."""
    size = np.array([w, h], np.float64)
    tiles = np.ceil(size / TILE)
    with np.errstate(invalid="ignore"):
        lo = np.clip(np.nan_to_num(mean - extent), 0.0, size - 1.0)
        hi = np.clip(np.nan_to_num(mean + extent), 0.0, size - 1.0)
        first = np.maximum(np.floor(lo / TILE), 0.0)
        last = np.minimum(np.ceil(hi / TILE) - 1.0, tiles - 1.0)
    return np.stack([first[:, 0], last[:, 0], first[:, 1], last[:, 1]], 1).astype(np.int64)


def rect_area(rect):
    return np.maximum(rect[:, 1] - rect[:, 0] + 1, 0) * np.maximum(rect[:, 3] - rect[:, 2] + 1, 0)


def theta_reach(pr):
    """How far float32 may turn the major axis: the shader takes it from (b, lambda1 - a), and lambda1 - a
    loses mid^2 / root^2 of its precision under the root (the Global theta)."""
    a, b, d = pr["cov2d"].T
    with np.errstate(all="ignore"):
        mid = 0.5 * (a + d)
        root = np.sqrt(np.maximum(mid * mid - (a * d - b * b), 1e-300))
        return np.minimum(4.0 * 2.0 ** -24 * mid * mid / (root * np.maximum(np.abs(b), 1e-300)), M.PI / 2.0)


def rect_in_doubt(pr, w, h, eps_px):
    """Gaussians one of whose unclamped box edges lies within float32's reach of a tile boundary: eps_px for
    the mean and the eigenvalues, plus what the axis' uncertainty moves the extents by."""
    size = np.array([w, h], np.float64)
    with np.errstate(all="ignore"):
        e = M.EXTENT_SIGMAS * pr["sigma"]
        reach = eps_px + theta_reach(pr) * np.abs(e[:, 0] - e[:, 1])
        out = np.zeros(len(reach), bool)
        for edge in (pr["mean"] - pr["extent"], pr["mean"] + pr["extent"]):
            inside = (edge > 0.0) & (edge < size - 1.0)  # a clamped edge lands on the frame's own limit
            f = np.mod(edge, TILE)
            out |= (inside & (np.minimum(f, TILE - f) < reach[:, None])).any(1)
    return out


def project_stereo(world, harm, sh, left, right, w, h, color_space=0, scene_transform=None, eps=1e-5):
    """Both eyes and what the reference decides for the pair.  Returns eyes (two project_eye dicts),
    eye_visible [2, n], visible, center_depth, det (the ink cull's), rect [n, 4] (the union), color, opacity,
    margins, margin (distance to the nearest deciding cull, for the callers' |margin| < eps), repair."""
    mid = 0.5 * (np.asarray(left["position"], np.float64) + np.asarray(right["position"], np.float64))
    eyes = [project_eye(world, harm, sh, c, w, h, color_space, scene_transform, sh_center=mid, ink=False)
            for c in (left, right)]
    vl, vr = eyes[0]["visible"], eyes[1]["visible"]
    both, either = vl & vr, vl | vr
    with np.errstate(all="ignore"):
        center = np.where(both, 0.5 * (eyes[0]["depth"] + eyes[1]["depth"]),
                          np.where(vl, eyes[0]["depth"], eyes[1]["depth"]))
        det = np.where(both, np.maximum(eyes[0]["det"], eyes[1]["det"]), np.where(vl, eyes[0]["det"], eyes[1]["det"]))
        ink = M.ink_margin(eyes[0]["opacity"], np.maximum(det, 0.0), center, float(left["near"]), float(left["far"]))
    ink = np.where(np.isfinite(ink), ink, -np.inf)
    rl, rr = (tile_rect(e["mean"], e["extent"], w, h) for e in eyes)
    union = np.stack([np.minimum(rl[:, 0], rr[:, 0]), np.maximum(rl[:, 1], rr[:, 1]),
                      np.minimum(rl[:, 2], rr[:, 2]), np.maximum(rl[:, 3], rr[:, 3])], 1)
    rect = np.where(both[:, None], union, np.where(vl[:, None], rl, rr))
    visible = either & (ink > 0.0) & (rect_area(rect) > 0)
    ml, mr = eyes[0]["margin"], eyes[1]["margin"]
    margin = np.minimum(np.minimum(np.abs(ml), np.abs(mr)), np.where(either, np.abs(ink), np.inf))
    doubt = (rect_in_doubt(eyes[0], w, h, eps * max(w, h)) & vl) | (rect_in_doubt(eyes[1], w, h, eps * max(w, h)) & vr)
    return dict(eyes=eyes, eye_visible=np.stack([vl & visible, vr & visible]), visible=visible, center_depth=center,
                depth=center, det=det, rect=rect, rect_doubt=doubt & visible, color=eyes[0]["color"],
                opacity=eyes[0]["opacity"], margins=dict(left=ml, right=mr, ink=ink), margin=margin,
                repair=eyes[0]["repair"] | eyes[1]["repair"])


# ---------------------------------------------------------------------------------------------------
# mono tile membership
# ---------------------------------------------------------------------------------------------------
def min_quadratic_over_rect(conic, x0, x1, y0, y1):
    """The least value of A x^2 + 2 B x y + C y^2 over [x0, x1] x [y0, y1] (coordinates relative to the
    mean; A, C > 0 and A C > B^2, so the form is convex).  Zero when the origin lies inside; otherwise the
    minimum is on the boundary, and on an edge the form is a parabola in one variable whose vertex is clamped
    to the edge."""
    A, B, C = conic[..., 0], conic[..., 1], conic[..., 2]

    def on_vertical(x):  # minimise over y in [y0, y1] at fixed x
        y = np.clip(-B * x / C, y0, y1)
        return A * x * x + 2.0 * B * x * y + C * y * y

    def on_horizontal(y):
        x = np.clip(-B * y / A, x0, x1)
        return A * x * x + 2.0 * B * x * y + C * y * y
    edges = np.minimum(np.minimum(on_vertical(x0), on_vertical(x1)), np.minimum(on_horizontal(y0), on_horizontal(y1)))
    inside = (x0 <= 0.0) & (0.0 <= x1) & (y0 <= 0.0) & (0.0 <= y1)
    return np.where(inside, 0.0, edges)


def mono_pairs(pr, q, w, h):
    """Every (gaussian, tile) of the rectangles of the gaussians that pass the culls: gaussian [p], tile [p]
    (row-major), qmin [p] (least quadratic form of the quantised record q over the tile's extent
    [16 tx, 16 tx + 16] x [16 ty, 16 ty + 16]) and cutoff [p] = -2 ln(tau / opacity) of the quantised opacity
    (negative for the byte 1, whose opacity is below tau: no tile can pass)."""
    tiles_x = (w + TILE - 1) // TILE
    rect = tile_rect(pr["mean"], pr["extent"], w, h)
    g = np.nonzero(pr["visible"] & (rect_area(rect) > 0))[0]
    nx, ny = rect[g, 1] - rect[g, 0] + 1, rect[g, 3] - rect[g, 2] + 1
    cnt = nx * ny
    gi = np.repeat(np.arange(len(g)), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    tx, ty = rect[g[gi], 0] + k % nx[gi], rect[g[gi], 2] + k // nx[gi]
    gg = g[gi]
    x0, y0 = tx * float(TILE) - q["mean"][gg, 0], ty * float(TILE) - q["mean"][gg, 1]
    qmin = min_quadratic_over_rect(q["conic"][gg], x0, x0 + TILE, y0, y0 + TILE)
    with np.errstate(divide="ignore"):
        cutoff = -2.0 * np.log(TAU / q["opacity"][gg])
    return dict(gaussian=gg, tile=ty * tiles_x + tx, qmin=qmin, cutoff=cutoff, rect=rect)


def project_mono(world, harm, sh, cam, w, h, color_space=0, rel=0.0, eps=1e-5):
    """The mono frame's projection: project_eye with the ink cull, the quantised record, the tile test.  A pair
    is `sure` when its minimum is further than rel (relative) from the cutoff; a gaussian is visible when it
    passes the culls and a tile passes.  rect_doubt: gaussians whose rectangle has an edge within float32's reach
    of a tile boundary (eps of the frame's longer side), so that a row or column of tiles may or may not be tested."""
    pr = project_eye(world, harm, sh, cam, w, h, color_space)
    q = M.quantise_global(pr)
    pairs = mono_pairs(pr, q, w, h)
    passes = pairs["qmin"] <= pairs["cutoff"]
    pairs["passes"] = passes
    pairs["doubt"] = np.abs(pairs["qmin"] - pairs["cutoff"]) <= rel * np.abs(pairs["cutoff"])
    n = len(world)
    touched = np.bincount(pairs["gaussian"][passes], minlength=n)
    sure = np.bincount(pairs["gaussian"][passes & ~pairs["doubt"]], minlength=n)
    maybe = np.bincount(pairs["gaussian"][pairs["doubt"]], minlength=n)
    pr["culls_pass"] = pr["visible"]
    pr["rect_doubt"] = rect_in_doubt(pr, w, h, eps * max(w, h)) & pr["culls_pass"]
    pr["visible"] = pr["visible"] & (touched > 0)
    pr["tile_doubt"] = pr["culls_pass"] & (sure == 0) & (maybe > 0)  # visibility hangs on a pair in doubt
    pr["touched"], pr["pairs"], pr["record"] = touched, pairs, q
    return pr


# ---------------------------------------------------------------------------------------------------
# records and order
# ---------------------------------------------------------------------------------------------------
def from_stereo_records(rd) -> list:
    """StereoTiledRenderData (32 bytes) widened: one dict per eye (mean, conic as (A, B, C) with B = Cxy2 / 2,
    depth, visible through the sentinel) sharing colour, opacity and the centre depth."""
    color = np.stack([rd["colorR"], rd["colorG"], rd["colorB"]], 1).astype(np.float64) / 255.0
    opacity = rd["opacity"].astype(np.float64) / 255.0
    center = M.h2d(rd["centerDepth"])
    out = []
    for eye in ("left", "right"):
        mx = M.h2d(rd[eye + "MeanX"])
        with np.errstate(invalid="ignore"):
            vis = mx >= SENTINEL_BELOW
        conic = np.stack([M.h2d(rd[eye + "Cxx"]), 0.5 * M.h2d(rd[eye + "Cxy2"]), M.h2d(rd[eye + "Cyy"])], 1)
        mean = np.stack([mx, M.h2d(rd[eye + "MeanY"])], 1)
        out.append(dict(mean=np.where(vis[:, None], mean, 0.0), conic=conic, visible=vis, raw_mean=mean,
                        opacity=np.where(vis, opacity, 0.0), record_opacity=opacity, color=color,
                        depth=M.h2d(rd[eye + "Depth"]), center_depth=center))
    return out


def quantise_stereo(ps) -> list:
    """The model's stereo projection stored as the record stores it (fp16 means, conics and depths, truncating
    u8 colour and opacity), widened; an eye that is not visible blends nothing."""
    u8 = lambda v: np.floor(np.clip(np.nan_to_num(v) * 255.0, 0.0, 255.0)) / 255.0
    out = []
    for e, pr in enumerate(ps["eyes"]):
        vis = ps["eye_visible"][e]
        A, B, C = pr["conic"].T
        conic = np.stack([M.round_h(A), 0.5 * M.round_h(2.0 * B), M.round_h(C)], 1)
        out.append(dict(mean=np.where(vis[:, None], M.round_h(pr["mean"]), 0.0), conic=np.nan_to_num(conic), visible=vis,
                        opacity=np.where(vis, u8(ps["opacity"]), 0.0), color=u8(ps["color"]), depth=M.round_h(pr["depth"]),
                        center_depth=M.round_h(ps["center_depth"])))
    return out


def depth_keys(depth, key_bits=32):
    """The sort key of a positive depth as an integer: the float32's bits with the sign bit set, or with 16-bit
    keys the bits of its fp16 rounding with the sign bit flipped."""
    with np.errstate(invalid="ignore", over="ignore"):
        d32 = np.asarray(depth, np.float64).astype(np.float32)
        if key_bits == 16:
            return (d32.astype(np.float16).view(np.uint16).astype(np.int64) ^ 0x8000) & 0xFFFF
        bits = d32.view(np.uint32).astype(np.int64)
    return np.where(bits & 0x80000000, bits ^ 0xFFFFFFFF, bits ^ 0x80000000)


def depth_order(depth, ids, key_bits=32) -> np.ndarray:
    """ids ascending in (key, id)."""
    ids = np.asarray(ids)
    return ids[np.lexsort((ids, depth_keys(depth, key_bits)[ids]))]


# ---------------------------------------------------------------------------------------------------
# lists and frames
# ---------------------------------------------------------------------------------------------------
def lists_from_pairs(gaussian, tile, order):
    """(tile, ids in blend order) of every tile that holds a pair; order: all ids, front to back."""
    rank = np.empty(int(max(order.max(initial=-1), gaussian.max(initial=-1))) + 1, np.int64)
    rank[order] = np.arange(len(order))
    srt = np.lexsort((rank[gaussian], tile))
    t, g = tile[srt], gaussian[srt]
    cut = np.nonzero(np.diff(t))[0] + 1
    return [(int(tt[0]), gg) for tt, gg in zip(np.split(t, cut), np.split(g, cut))] if len(t) else []


def rect_pairs(rect, ids, w):
    """Every (gaussian, tile) of the rectangles rect[ids]."""
    tiles_x = (w + TILE - 1) // TILE
    r = rect[ids]
    nx, cnt = r[:, 1] - r[:, 0] + 1, rect_area(r)
    gi = np.repeat(np.arange(len(ids)), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return ids[gi], (r[gi, 2] + k // nx[gi]) * tiles_x + r[gi, 0] + k % nx[gi]


def blend_mono(records, lists, w, h, on_tile=None) -> dict:
    return M.blend_lists(records, lists, TILE, TILE, w, h, CLEAR, MONO_RULES, on_tile=on_tile)


def blend_stereo(eye_records, lists, w, h, on_tile=None) -> list:
    """One frame per eye.  An eye whose group is saturated skips entries and the walk ends when both are:
    since a skipped entry leaves the eye's transmittance where it is, each eye stops on its own, as a mono
    walk does.  A gaussian that is not visible in an eye has opacity 0 there."""
    return [M.blend_lists(rec, lists, TILE, TILE, w, h, CLEAR, STEREO_RULES,
                          on_tile=None if on_tile is None else (lambda *a, e=e: on_tile(e, *a)))
            for e, rec in enumerate(eye_records)]


def split_side_by_side(color, w):
    """The side-by-side target [h, 2 w, 4] as the two eyes' frames [2, h, w, 4]: the copy pass draws slice
    row 0 at the bottom, so rows come back in reverse."""
    return np.stack([color[::-1, e * w:(e + 1) * w] for e in range(2)])
