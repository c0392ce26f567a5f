"""A float64 model of gaussian splatting as the reference's shaders describe it (TEST INFRASTRUCTURE).

Second derivation of the frame, independent of oracle/gsm_oracle.c and of the HIP kernels: plain numpy,
float64 throughout, written from the mathematics (pinhole projection, the EWA Jacobian, the symmetric
2x2 eigenproblem, the real spherical harmonics, front-to-back compositing) and from the conventions the
reference's shader source fixes (pixel centres, the 0.3 dilation, the 1.3 tan(fov/2) clamp, SH signs and
layout, the cull thresholds, record formats, tile sizes, clear values, alpha cut-offs).  It imports
nothing from oracle/, loads no shared library and reads no file.

Where a closed form exists that the shaders do not use, the closed form is used here (the major axis is
atan2(2b, a - d) / 2, the conic is the matrix inverse, the quaternion goes through normalisation and the
textbook rotation matrix), so that an error of form in one derivation does not repeat in the other.

The repair branches of stabilizeCovariance2D are not modelled: with the 0.3 dilation the covariance is
positive definite and the function is the identity, except for an axis ratio above 256 or an extent above
twice the frame.  project() reports the gaussians that would enter those branches ("repair").
"""
from __future__ import annotations

import numpy as np

PI = np.pi

# What the reference's host code and shaders fix for every frame
ALPHA_THRESHOLD = 0.005      # TileBinningParams.alphaThreshold
TOTAL_INK_THRESHOLD = 2.0    # TileBinningParams.totalInkThreshold
MIN_SCALE = 0.0005           # kMinGaussianScale
MIN_RADIUS = 0.5             # kMinProjectedRadius
DILATION = 0.3               # low-pass term added to the 2-D covariance's diagonal
FOV_CLAMP = 1.3              # Jacobian's x/z, y/z are clamped to 1.3 tan(half fov)
MAX_AXIS_RATIO = 256.0       # stabilizeCovariance2D: repairs above this sigma ratio
EXTENT_SIGMAS = 3.0          # tile rectangle: the box around the 3 sigma oriented box

# What differs between the two tiled blends (globalRender / localRender16)
GLOBAL_RULES = dict(tile=(32, 16), group=(4, 2), break_below=1.0 / 255.0, alpha_max=0.99,
                    depth="blend")
LOCAL_RULES = dict(tile=(16, 16), group=(16, 16), break_below=0.004, alpha_max=0.99,
                   depth="first", depth_alpha=0.1)
GLOBAL_CLEAR = (0.0, 0.0, 0.0, 1.0)  # clearRenderTexturesKernel; depth 0
LOCAL_CLEAR = (0.0, 0.0, 0.0, 0.0)   # localClearTextures; depth 0


# ---------------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------------
def h2d(bits) -> np.ndarray:
    """fp16 bit patterns -> float64."""
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def round_h(x) -> np.ndarray:
    """float64 rounded to the nearest fp16 (ties to even), as float64."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def h_bits(x) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def h_ulp(x) -> np.ndarray:
    """The fp16 spacing at |x| (2^-24 in the subnormal range)."""
    ax = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(ax)) - 10)


def unpack_world(world):
    """(position [n,3], scale [n,3], quaternion xyzw [n,4], opacity [n]) in float64."""
    names = world.dtype.names
    pos = np.stack([world["px"], world["py"], world["pz"]], 1).astype(np.float64)
    if "rot" in names:
        scale = np.stack([world["sx"], world["sy"], world["sz"]], 1).astype(np.float64)
        quat = world["rot"].astype(np.float64)
        op = world["opacity"].astype(np.float64)
    else:
        scale = np.stack([h2d(world["sx"]), h2d(world["sy"]), h2d(world["sz"])], 1)
        quat = np.stack([h2d(world[k]) for k in ("rx", "ry", "rz", "rw")], 1)
        op = h2d(world["opacity"])
    return pos, scale, quat, op


def unpack_harmonics(harm, n, k):
    """[n, 3, k] float64: channel-major per gaussian (all of R, then G, then B)."""
    harm = np.asarray(harm)
    vals = h2d(harm) if harm.dtype == np.uint16 else harm.astype(np.float64)
    return vals.reshape(n, 3, k)


# ---------------------------------------------------------------------------------------------------
# spherical harmonics
# ---------------------------------------------------------------------------------------------------
# The closed-form real harmonics, listed as (l, m) with m = -l..l, are cos/sin(|m| phi) P_l^|m|(cos theta)
# with positive normalisation and NO Condon-Shortley phase.  The reference (and 3DGS before it) carries
# the phase: function (l, m) is the closed form times (-1)^m.
SH_LM = [(l, m) for l in range(4) for m in range(-l, l + 1)]
SH_SIGNS = np.array([(-1.0) ** (m % 2) for _, m in SH_LM])


def sh_basis(d) -> np.ndarray:
    """The 16 basis values [..., 16] at unit directions d [..., 3], in the reference's order and signs."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    s = np.sqrt
    k0 = s(1 / (4 * PI))
    k1 = s(3 / (4 * PI))
    k2a, k2b, k2c = s(15 / (4 * PI)), s(5 / (16 * PI)), s(15 / (16 * PI))
    k3a, k3b, k3c, k3d = s(35 / (32 * PI)), s(105 / (4 * PI)), s(21 / (32 * PI)), s(7 / (16 * PI))
    k3e = s(105 / (16 * PI))
    r2 = x * x + y * y + z * z  # 1 on the sphere; keeps the polynomials homogeneous
    out = np.stack([
        k0 * np.ones_like(x),
        -k1 * y, k1 * z, -k1 * x,
        k2a * x * y, -k2a * y * z, k2b * (3 * z * z - r2), -k2a * x * z, k2c * (x * x - y * y),
        -k3a * y * (3 * x * x - y * y), k3b * x * y * z, -k3c * y * (5 * z * z - r2),
        k3d * z * (5 * z * z - 3 * r2), -k3c * x * (5 * z * z - r2), k3e * z * (x * x - y * y),
        -k3a * x * (x * x - 3 * y * y)], -1)
    return out


def srgb_decode(c):
    c = np.clip(c, 0.0, 1.0)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


# ---------------------------------------------------------------------------------------------------
# projection
# ---------------------------------------------------------------------------------------------------
def _mat(flat):
    """A column-major flat 4x4 (as the camera dicts carry it) as a row-by-column matrix."""
    return np.asarray(flat, np.float64).reshape(4, 4).T


def rotation_from_quaternion(q):
    """Rotation matrices [n,3,3] of quaternions xyzw [n,4], normalised here (floor 1e-8 on the squared norm)."""
    nrm = np.sqrt(np.maximum((q * q).sum(1), 1e-8))
    v = q[:, :3] / nrm[:, None]
    r = q[:, 3] / nrm
    n = len(q)
    K = np.zeros((n, 3, 3))  # cross-product matrix of v
    K[:, 0, 1], K[:, 0, 2] = -v[:, 2], v[:, 1]
    K[:, 1, 0], K[:, 1, 2] = v[:, 2], -v[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -v[:, 1], v[:, 0]
    return np.eye(3)[None] + 2.0 * r[:, None, None] * K + 2.0 * (K @ K)  # Rodrigues, |q| = 1


def ink_margin(op, det, depth, near, far):
    """Signed margin of the ink cull: opacity * 2 pi sqrt(det) against the threshold times the depth factor
    (1 - saturate((0.02 far - depth) / (0.02 far - near))^2); no cull where the factor is zero."""
    with np.errstate(all="ignore"):
        ink = op * 2.0 * PI * np.sqrt(np.maximum(det, 1e-12))
        far_adj = far * 0.02
        depth_factor = 1.0 - np.clip((far_adj - depth) / (far_adj - near), 0.0, 1.0) ** 2
        return np.where(depth_factor * TOTAL_INK_THRESHOLD > 0,
                        ink / np.maximum(depth_factor * TOTAL_INK_THRESHOLD, 1e-300) - 1.0, 1.0)


def project(world, harm, sh_components, cam, w, h, color_space=0, renderer="global", scene_transform=None,
            sh_center=None, pose=False):
    """Every gaussian of the scene through the reference's projection, in float64.

    Returns a dict of arrays over all n gaussians (culled ones included; their later fields may hold
    non-finite values): view [n,3], depth (clip w), mean [n,2] (pixel centres at integers), cov3d, cov2d
    (a, b, d), sigma [n,2] (sigma1 >= sigma2), theta (major axis in [0, pi)), conic [n,3] (A, B, C of
    A dx^2 + 2 B dx dy + C dy^2), color [n,3], opacity, extent [n,2], margins {name: signed distance to the
    cull threshold, positive = kept}, margin (their minimum), visible, repair.
    renderer: "global" culls on the screen rectangle; "local" culls past the far plane and on an empty
    tile rectangle instead; "depthfirst" maps ndc to the screen without the half-pixel shift and culls past
    the far plane and on the screen rectangle (one eye of the DepthFirst frames).
    scene_transform (column-major flat 4x4, scene -> world) moves the positions and multiplies the scales by
    the length of its first column; its rotation does not turn the covariance and the SH direction is taken
    from the untransformed position (both the reference's choices).  sh_center: the point the SH direction
    is taken from, the camera position by default.
    pose=True takes scene_transform as the model matrix M of a composite's object and does what
    the mathematics does: the covariance becomes A Sigma A^T with A the upper 3x3 of M (for a similarity, the
    scales times its factor and the axes turned by its rotation), and the SH direction is that from the
    gaussian to the camera seen in the object's frame, A^-1 (camera - M p).  The scale cull stays on the
    scales as stored."""
    n = len(world)
    k = max(int(sh_components), 1)
    pos, scale, quat, op = unpack_world(world)
    scene_pos, model_scale = pos, scale
    if scene_transform is not None:
        S = _mat(scene_transform)
        pos = (np.concatenate([pos, np.ones((n, 1))], 1) @ S.T)[:, :3]
        scale = scale * np.linalg.norm(S[:3, 0])
    shift = 0.0 if renderer == "depthfirst" else 0.5
    V, P = _mat(cam["view"]), _mat(cam["proj"])
    near, far = float(cam["near"]), float(cam["far"])
    W, H = float(w), float(h)
    with np.errstate(all="ignore"):
        view4 = np.concatenate([pos, np.ones((n, 1))], 1) @ V.T
        clip = view4 @ P.T
        depth = clip[:, 3]
        ndc = clip[:, :2] / depth[:, None]
        # pixel centres sit at integers: ndc -1 is the left edge of pixel 0, i.e. -0.5
        # (the DepthFirst frames leave the shift out: ndc -1 is coordinate 0)
        mean = (ndc + 1.0) * 0.5 * np.array([W, H]) - shift

        R = rotation_from_quaternion(quat)
        if pose and scene_transform is not None:
            A = S[:3, :3]
            cov3d = A @ (R @ (model_scale[:, :, None] ** 2 * np.transpose(R, (0, 2, 1)))) @ A.T
        else:
            cov3d = R @ (scale[:, :, None] ** 2 * np.transpose(R, (0, 2, 1)))

        vx, vy, vz = view4[:, 0], view4[:, 1], view4[:, 2]
        az = np.maximum(np.abs(vz), 1e-4)
        sg = np.where(vz >= 0, 1.0, -1.0)
        tan_x, tan_y = 1.0 / abs(P[0, 0]), 1.0 / abs(P[1, 1])
        fx, fy = 0.5 * W * abs(P[0, 0]), 0.5 * H * abs(P[1, 1])
        tx = np.clip(vx / az, -FOV_CLAMP * tan_x, FOV_CLAMP * tan_x)
        ty = np.clip(vy / az, -FOV_CLAMP * tan_y, FOV_CLAMP * tan_y)
        J = np.zeros((n, 2, 3))  # d(pixel) / d(view position) of the pinhole map, at the clamped point
        J[:, 0, 0], J[:, 0, 2] = fx / az, -fx * tx * sg / az
        J[:, 1, 1], J[:, 1, 2] = fy / az, -fy * ty * sg / az
        T = J @ V[:3, :3]
        c2 = T @ cov3d @ np.transpose(T, (0, 2, 1))
        a, b, d = c2[:, 0, 0] + DILATION, 0.5 * (c2[:, 0, 1] + c2[:, 1, 0]), c2[:, 1, 1] + DILATION

        det = a * d - b * b
        mid = 0.5 * (a + d)
        root = np.sqrt(np.maximum(mid * mid - det, 0.0))
        lam1, lam2 = mid + root, mid - root
        sigma = np.sqrt(np.stack([lam1, lam2], 1))
        theta = np.mod(0.5 * np.arctan2(2.0 * b, a - d), PI)
        conic = np.stack([d, -b, a], 1) / det[:, None]

        # the reference's tile rectangle: the box around the oriented 3 sigma box
        ct, st = np.abs(np.cos(theta)), np.abs(np.sin(theta))
        e1, e2 = EXTENT_SIGMAS * sigma[:, 0], EXTENT_SIGMAS * sigma[:, 1]
        extent = np.stack([ct * e1 + st * e2, st * e1 + ct * e2], 1)

        max_extent = 2.0 * max(W, H) / 3.0
        repair = ~np.isfinite(a + b + d) | (lam1 > max_extent ** 2) | \
            (lam2 * MAX_AXIS_RATIO ** 2 < lam1) | (det < 1e-8)

        m = {}
        m["scale"] = model_scale.max(1) / MIN_SCALE - 1.0  # (the scale as stored, before a scene transform)
        m["near"] = depth / near - 1.0
        m["alpha"] = op / ALPHA_THRESHOLD - 1.0
        if renderer == "local":
            radius = 3.0 * np.ceil(sigma[:, 0])
        else:
            radius = 3.0 * sigma[:, 0]
        m["radius"] = radius / MIN_RADIUS - 1.0
        m["ink"] = ink_margin(op, det, depth, near, far)
        lo, hi = mean - extent, mean + extent
        if renderer == "depthfirst":
            m["far"] = 1.0 - depth / far
        if renderer in ("global", "depthfirst"):
            # kept while the rectangle reaches into [0, W] x [0, H]; in units of the frame's longer side
            m["screen"] = np.minimum(np.minimum(hi[:, 0], W - lo[:, 0]),
                                     np.minimum(hi[:, 1], H - lo[:, 1])) / max(W, H)
        else:
            m["far"] = 1.0 - depth / far
            # the tile rectangle of the clamped box is empty when the box ends at or left of / above pixel 0
            # (and, when the last pixel starts a tile, when it begins at or past the last pixel)
            s = np.minimum(hi[:, 0], hi[:, 1])
            if (w - 1) % LOCAL_RULES["tile"][0] == 0:
                s = np.minimum(s, (W - 1.0) - lo[:, 0])
            if (h - 1) % LOCAL_RULES["tile"][1] == 0:
                s = np.minimum(s, (H - 1.0) - lo[:, 1])
            m["screen"] = s / max(W, H)
        for key in m:
            m[key] = np.where(np.isfinite(m[key]), m[key], -np.inf)
        # only a gaussian that passes the culls ahead of the covariance stage can enter a repair branch
        reaches = (m["scale"] > 0) & (m["near"] > 0) & (m["alpha"] > 0) & (m.get("far", m["near"]) > 0)
        repair &= reaches
        # a gaussian is kept when it passes every test, so the minimum margin decides (a margin of exactly
        # zero passes some tests and fails others; callers leave |margin| < eps out)
        margin = np.min(np.stack(list(m.values()), 1), 1)
        visible = margin > 0.0

        center = cam["position"] if sh_center is None else sh_center
        if pose and scene_transform is not None and sh_center is None:
            dirs = (np.asarray(center, np.float64)[None] - pos) @ np.linalg.inv(S[:3, :3]).T
        else:
            dirs = np.asarray(center, np.float64)[None] - scene_pos
        dirs = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
        coef = unpack_harmonics(harm, n, k)
        if k == 1:
            color = coef[:, :, 0] * sh_basis(np.array([0.0, 0.0, 1.0]))[0]
        else:
            color = np.einsum("nck,nk->nc", coef[:, :, :min(k, 16)], sh_basis(dirs)[:, :min(k, 16)])
        color = np.maximum(color + 0.5, 0.0)
        if color_space == 1:
            color = srgb_decode(color)

    return dict(view=view4[:, :3], depth=depth, mean=mean, cov3d=cov3d, cov2d=np.stack([a, b, d], 1), det=det,
                sigma=sigma, theta=theta, conic=conic, color=color, opacity=op, extent=extent,
                margins=m, margin=margin, visible=visible, repair=repair)


# ---------------------------------------------------------------------------------------------------
# records: the implementation's packed formats, widened; and the model's values packed the same way
# ---------------------------------------------------------------------------------------------------
def conic_from_theta_sigmas(theta, s1, s2):
    """R(theta) diag(1/s1^2, 1/s2^2) R(theta)^T as (A, B, C); sigmas floored at 1e-4."""
    i1, i2 = 1.0 / np.maximum(s1, 1e-4) ** 2, 1.0 / np.maximum(s2, 1e-4) ** 2
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([c * c * i1 + s * s * i2, c * s * (i1 - i2), s * s * i1 + c * c * i2], -1)


def from_global_records(render_data) -> dict:
    """GaussianRenderData (16 bytes) widened to float64."""
    r = render_data
    s1, s2 = h2d(r["sigma1"]), h2d(r["sigma2"])
    theta = r["theta"].astype(np.float64) * (PI / 65535.0)
    return dict(mean=np.stack([h2d(r["meanX"]), h2d(r["meanY"])], 1),
                conic=conic_from_theta_sigmas(theta, s1, s2), sigma=np.stack([s1, s2], 1), theta=theta,
                opacity=r["opacity"].astype(np.float64) / 255.0,
                color=np.stack([r["colorR"], r["colorG"], r["colorB"]], 1).astype(np.float64) / 255.0,
                depth=h2d(r["depth"]))


def from_local_records(projected) -> dict:
    """ProjectedGaussian (32 bytes, fp16 fields) widened to float64."""
    p = projected
    return dict(mean=np.stack([h2d(p["posX"]), h2d(p["posY"])], 1),
                conic=np.stack([h2d(p["conicA"]), h2d(p["conicB"]), h2d(p["conicC"])], 1),
                opacity=h2d(p["opacity"]),
                color=np.stack([h2d(p["colorR"]), h2d(p["colorG"]), h2d(p["colorB"])], 1),
                depth=h2d(p["depth"]))


def quantise_global(pr) -> dict:
    """The model's projection stored as the Global record stores it (fp16 mean, sigmas and depth, theta in
    65535 steps of pi rounded to nearest, truncating u8 colour and opacity), widened again."""
    tq = np.floor(np.clip(pr["theta"] * (65535.0 / PI) + 0.5, 0.0, 65535.0))
    theta = tq * (PI / 65535.0)
    s = round_h(pr["sigma"])
    u8 = lambda v: np.floor(np.clip(np.nan_to_num(v) * 255.0, 0.0, 255.0)) / 255.0
    return dict(mean=round_h(pr["mean"]), conic=conic_from_theta_sigmas(theta, s[:, 0], s[:, 1]), sigma=s,
                theta=theta, opacity=u8(pr["opacity"]), color=u8(pr["color"]), depth=round_h(pr["depth"]))


def quantise_local(pr) -> dict:
    """The model's projection stored as the Local record stores it: every field rounded to fp16."""
    return dict(mean=round_h(pr["mean"]), conic=round_h(pr["conic"]), opacity=round_h(pr["opacity"]),
                color=round_h(pr["color"]), depth=round_h(pr["depth"]))


def depth_order(depth, ids=None) -> np.ndarray:
    """ids in the blend's global order: ascending (fp16(depth) bits ^ 0x8000, id)."""
    ids = np.arange(len(depth)) if ids is None else np.asarray(ids)
    key = (h_bits(depth[ids]).astype(np.int64) ^ 0x8000) & 0xFFFF
    return ids[np.lexsort((ids, key))]


# ---------------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------------
def _power_terms(rec, ids, px, py):
    """The three terms [k, p] of the quadratic form A dx^2 + 2 B dx dy + C dy^2 of gaussians ids at (px, py)."""
    dx = px[None, :] - rec["mean"][ids, 0][:, None]
    dy = py[None, :] - rec["mean"][ids, 1][:, None]
    A, B, C = (rec["conic"][ids, i][:, None] for i in range(3))
    return A * dx * dx, 2.0 * B * dx * dy, C * dy * dy


def _alphas(rec, ids, px, py, alpha_max, r2_max=None):
    """alpha [k, p] of gaussians ids at the pixels (px, py), exact exp; zero where the quadratic form
    exceeds r2_max, if one is given."""
    power = sum(_power_terms(rec, ids, px, py))
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = np.minimum(rec["opacity"][ids][:, None] * np.exp(-0.5 * power), alpha_max)
    return alpha if r2_max is None else np.where(power > r2_max, 0.0, alpha)


def _composite(rec, ids, alpha, live, rules):
    """Front-to-back sums over the entries that are `live` [k, p].  Returns rgb [p,3], alpha [p], depth [p]
    and, for rules['depth'] == 'first', the pixels whose depth hangs on an alpha within 2% of the cut."""
    a = np.where(live, alpha, 0.0)
    one_minus = 1.0 - a
    T_before = np.ones_like(a)
    np.cumprod(one_minus[:-1], axis=0, out=T_before[1:])
    wgt = a * T_before
    rgb = wgt.T @ rec["color"][ids]
    out_alpha = 1.0 - T_before[-1] * one_minus[-1] if len(ids) else np.zeros(alpha.shape[1])
    unsure = np.zeros(alpha.shape[1], bool)
    if rules["depth"] == "blend":
        dep = wgt.T @ rec["depth"][ids]
    else:
        cut = rules["depth_alpha"]

        def first(c):
            hit = a > c
            i = np.argmax(hit, axis=0)
            return np.where(hit.any(0), rec["depth"][ids][i], 0.0)
        dep = first(cut)
        unsure = (first(cut * 0.98) != dep) | (first(cut * 1.02) != dep)
    return rgb, out_alpha, dep, unsure


PICK_NONE = -1  # the model's "none" (the implementation's GSM_PICK_NONE is 0xFFFFFFFF)


def occluder_limits(occluder, xs, ys, w, h):
    """Z per pixel of (xs, ys): the occluder rounded once to fp16; +inf outside the frame (never read there)."""
    Z = np.full(len(xs), np.inf)
    if occluder is not None:
        inside = (xs < w) & (ys < h)
        Z[inside] = round_h(np.asarray(occluder, np.float64)[ys[inside], xs[inside]])
    return Z


def occlusion(Z, dep, how="sticky"):
    """(shut [k, p], closed_before [k, p]) of entries with fp16 depths dep [k] under limits Z [p].  An entry is
    shut at a pixel when it does not contribute there; closed_before is what the break test ahead of the entry
    sees.  how='sticky': a pixel closes at the first entry with Z < depth and stays closed (the contract's flag);
    how='entry': each entry is compared on its own, and the break test sees the previous entry's comparison (the
    kernel's form).  A NaN Z compares false: it occludes nothing."""
    with np.errstate(invalid="ignore"):
        behind = Z[None, :] < np.asarray(dep, np.float64)[:, None]
    shut = np.logical_or.accumulate(behind, axis=0) if how == "sticky" else behind
    before = np.zeros_like(shut)
    before[1:] = shut[:-1]
    return shut, before


def _pick(ids, wgt, query=None):
    """From the weights wgt [k, p] (alpha times the transmittance before the entry, zero where the entry is not
    live or is shut): the first entry of the largest weight per pixel (PICK_NONE where no weight is positive),
    that weight, the largest weight of any other entry, and -- for query [p], an id per pixel or PICK_NONE --
    the weight of the first occurrence of that id (-1 where the id is not in ids)."""
    k, p = wgt.shape
    cols = np.arange(p)
    first = np.argmax(wgt, axis=0)
    top = wgt[first, cols]
    rest = wgt.copy()
    rest[first, cols] = -1.0
    second = np.maximum(rest.max(0), 0.0) if k > 1 else np.zeros(p)
    pick = np.where(top > 0.0, np.asarray(ids)[first], PICK_NONE)
    out = dict(pick=pick, pick_weight=np.maximum(top, 0.0), pick_second=second)
    if query is not None:
        hit = np.asarray(ids)[:, None] == np.asarray(query)[None, :]
        at = np.argmax(hit, axis=0)
        out["query_in"], out["query_at"] = hit.any(0), at
        out["query_weight"] = np.where(out["query_in"], wgt[at, cols], -1.0)
    return out


def blend_lists(records, lists, tile_w, tile_h, w, h, clear, rules, on_tile=None, occluder=None, pick=False,
                pick_query=None, occlusion_form="sticky") -> dict:
    """Front-to-back compositing of each tile's list.  lists: iterable of (tile index, gaussian ids in blend
    order); tiles are numbered row-major over ceil(w / tile_w) columns.  A pixel group (rules['group'], in
    pixels) stops before the first entry at which the largest transmittance among its pixels is below
    rules['break_below'].  Pixels outside every listed tile hold `clear` (depth 0).  rules['r2_max'], if
    present, is the quadratic form beyond which alpha is zero.  on_tile(tile, ids, xs, ys, alpha, live) is
    called for every non-empty list with the [entries, pixels] arrays of that tile.
    Returns color [h,w,3], alpha [h,w], depth [h,w], covered [h,w] (inside a listed tile) and depth_unsure.
    occluder [h, w]: Z is the occluder rounded once to fp16; an entry contributes at a pixel only
    if not (Z < the entry's fp16 depth), by the sticky flag (occlusion_form 'entry': compared entry by entry);
    the break test sees a closed pixel's transmittance as 0.  Adds closed [h,w] (closed at the list's end) and
    closed_first [h,w] (closed by the first entry).
    pick: adds pick [h,w] (the first entry of the largest weight alpha * T_before among the live,
    unoccluded entries; PICK_NONE where no weight is positive), pick_weight, pick_second (the largest weight of
    any other entry) and, for pick_query [h,w] (ids or PICK_NONE), query_weight (that id's weight; -1 where it
    is not in the pixel's list) and query_open (it is a live, unoccluded entry of the list)."""
    tiles_x = (w + tile_w - 1) // tile_w
    color = np.empty((h, w, 3))
    color[:] = clear[:3]
    alpha = np.full((h, w), float(clear[3]))
    depth = np.zeros((h, w))
    covered = np.zeros((h, w), bool)
    unsure = np.zeros((h, w), bool)
    extra = {}
    if occluder is not None:
        extra.update(closed=np.zeros((h, w), bool), closed_first=np.zeros((h, w), bool))
    if pick:
        extra.update(pick=np.full((h, w), PICK_NONE, np.int64), pick_weight=np.zeros((h, w)),
                     pick_second=np.zeros((h, w)))
        if pick_query is not None:
            extra.update(query_weight=np.full((h, w), -1.0), query_open=np.zeros((h, w), bool))
    gw, gh = rules["group"]
    for tile, ids in lists:
        ids = np.asarray(ids, np.int64)
        x0, y0 = (tile % tiles_x) * tile_w, (tile // tiles_x) * tile_h
        ys, xs = np.mgrid[y0:y0 + tile_h, x0:x0 + tile_w]
        xs, ys = xs.reshape(-1), ys.reshape(-1)
        covered[y0:min(y0 + tile_h, h), x0:min(x0 + tile_w, w)] = True
        if len(ids) == 0:
            continue
        # the shaders form pixel coordinates in half precision
        a = _alphas(records, ids, round_h(xs), round_h(ys), rules["alpha_max"], rules.get("r2_max"))
        inside = (xs < w) & (ys < h)
        shut = None
        if occluder is not None:
            shut, closed_before = occlusion(occluder_limits(occluder, xs, ys, w, h), records["depth"][ids],
                                            occlusion_form)
            a = np.where(shut, 0.0, a)
        T_before = np.ones_like(a)
        np.cumprod(1.0 - a[:-1], axis=0, out=T_before[1:])
        T_seen = T_before if shut is None else np.where(closed_before, 0.0, T_before)
        group = ((ys - y0) // gh) * (tile_w // gw) + (xs - x0) // gw
        gmax = np.zeros((len(ids), group.max() + 1))
        for g in range(group.max() + 1):  # pixels outside the frame vote too, as the shader's lanes do
            gmax[:, g] = T_seen[:, group == g].max(1)
        live = (gmax >= rules["break_below"])[:, group]
        if shut is not None and occlusion_form != "sticky":
            live = np.logical_and.accumulate(live, axis=0)  # a walk that has stopped does not start again
        # T is non-increasing, so `live` is a prefix of the list; entries past it do not change T
        if on_tile is not None:
            on_tile(tile, ids, xs, ys, a, live)
        rgb, al, dep, uns = _composite(records, ids, a, live, rules)
        color[ys[inside], xs[inside]] = rgb[inside]
        alpha[ys[inside], xs[inside]] = al[inside]
        depth[ys[inside], xs[inside]] = dep[inside]
        unsure[ys[inside], xs[inside]] = uns[inside]
        if shut is not None:
            extra["closed"][ys[inside], xs[inside]] = shut[-1][inside]
            extra["closed_first"][ys[inside], xs[inside]] = shut[0][inside]
        if pick:
            wgt = np.where(live, a, 0.0) * T_before
            q = None if pick_query is None else np.where(inside, pick_query[np.minimum(ys, h - 1),
                                                                            np.minimum(xs, w - 1)], PICK_NONE)
            res = _pick(ids, wgt, q)
            for key in ("pick", "pick_weight", "pick_second"):
                extra[key][ys[inside], xs[inside]] = res[key][inside]
            if q is not None:
                extra["query_weight"][ys[inside], xs[inside]] = res["query_weight"][inside]
                ok = live if shut is None else live & ~shut
                extra["query_open"][ys[inside], xs[inside]] = (res["query_in"] & ok[res["query_at"],
                                                                                    np.arange(len(xs))])[inside]
    return dict(color=color, alpha=alpha, depth=depth, covered=covered, depth_unsure=unsure, **extra)


def blend_untiled(records, order, w, h, clear, rules=GLOBAL_RULES, rows=8, occluder=None, pick=False,
                  occlusion_form="sticky", surface_doubt=None) -> dict:
    """Every gaussian of `order` applied to every pixel, front to back in that order: no tiles, no
    rectangles, no saturation break.  `clear` fills the frame only when `order` is empty (a frame nothing
    was drawn into); compare drawn frames over the tiles that were active.
    occluder, pick, occlusion_form: as for blend_lists, every entry being live (closed, closed_first, pick,
    pick_weight, pick_second).  Every gaussian of the frame is an entry here, so 'closed' says little; of the
    entries whose alpha at the pixel is 1/255 or more, cut_any [h,w] says that one is shut, cut_first that the
    first is, and drawn_any that one is not.  surface_doubt = (depths [n], eps): adds at_surface [h,w], the
    pixels on which a gaussian of alpha >= 1e-3 has such a depth within eps (relative) of the pixel's Z."""
    order = np.asarray(order, np.int64)
    color = np.zeros((h, w, 3))
    alpha = np.zeros((h, w))
    depth = np.zeros((h, w))
    unsure = np.zeros((h, w), bool)
    extra = {}
    if occluder is not None:
        extra.update({k: np.zeros((h, w), bool) for k in ("closed", "closed_first", "at_surface", "cut_any",
                                                          "cut_first", "drawn_any")})
    if pick:
        extra.update(pick=np.full((h, w), PICK_NONE, np.int64), pick_weight=np.zeros((h, w)),
                     pick_second=np.zeros((h, w)))
    if len(order) == 0:
        color[:] = clear[:3]
        alpha[:] = clear[3]
        return dict(color=color, alpha=alpha, depth=depth, depth_unsure=unsure, **extra)
    for y0 in range(0, h, rows):
        ys, xs = np.mgrid[y0:min(y0 + rows, h), 0:w]
        shp = xs.shape
        xs, ys = xs.reshape(-1), ys.reshape(-1)
        a = _alphas(records, order, round_h(xs), round_h(ys), rules["alpha_max"])
        if occluder is not None:
            Z = occluder_limits(occluder, xs, ys, w, h)
            if surface_doubt is not None:
                d = np.asarray(surface_doubt[0], np.float64)[order][:, None]
                with np.errstate(invalid="ignore"):
                    near = (np.abs(d - Z[None, :]) <= surface_doubt[1] * np.abs(d)) & (a >= 1e-3)
                extra["at_surface"][y0:y0 + shp[0]] = near.any(0).reshape(shp)
            shut, _ = occlusion(Z, records["depth"][order], occlusion_form)
            seen = a >= 1.0 / 255.0
            first = np.argmax(seen, axis=0)
            extra["cut_any"][y0:y0 + shp[0]] = (seen & shut).any(0).reshape(shp)
            extra["drawn_any"][y0:y0 + shp[0]] = (seen & ~shut).any(0).reshape(shp)
            extra["cut_first"][y0:y0 + shp[0]] = (seen.any(0) & shut[first, np.arange(len(xs))]).reshape(shp)
            a = np.where(shut, 0.0, a)
            extra["closed"][y0:y0 + shp[0]] = shut[-1].reshape(shp)
            extra["closed_first"][y0:y0 + shp[0]] = shut[0].reshape(shp)
        rgb, al, dep, uns = _composite(records, order, a, np.ones(a.shape, bool), rules)
        color[y0:y0 + shp[0]] = rgb.reshape(shp + (3,))
        alpha[y0:y0 + shp[0]] = al.reshape(shp)
        depth[y0:y0 + shp[0]] = dep.reshape(shp)
        unsure[y0:y0 + shp[0]] = uns.reshape(shp)
        if pick:
            T_before = np.ones_like(a)
            np.cumprod(1.0 - a[:-1], axis=0, out=T_before[1:])
            res = _pick(order, a * T_before)
            for key in ("pick", "pick_weight", "pick_second"):
                extra[key][y0:y0 + shp[0]] = res[key].reshape(shp)
    return dict(color=color, alpha=alpha, depth=depth, depth_unsure=unsure, **extra)


def lists_from_headers(headers, sorted_values):
    """(tile, ids) of every tile with a nonzero count, from GaussianHeader {offset, count} and the sorted ids."""
    return [(t, np.asarray(sorted_values[o:o + c])) for t, (o, c) in enumerate(np.asarray(headers).tolist()) if c]


def lists_from_local(tile_counts, tile_lists, max_per_tile=2048):
    return [(t, np.asarray(tile_lists[t, :min(c, max_per_tile)])) for t, c in enumerate(np.asarray(tile_counts).tolist())
            if c]


# ---------------------------------------------------------------------------------------------------
# the composite of posed scenes
# ---------------------------------------------------------------------------------------------------
ITEM_BLOCK = 256  # object o's items start at 256 * B_o, B_o = the blocks of the objects before it


def item_layout(counts):
    """(first item of every object, items in all): B_o = sum over u < o of ceil(count_u / 256)."""
    blocks = [(int(c) + ITEM_BLOCK - 1) // ITEM_BLOCK for c in counts]
    base = ITEM_BLOCK * np.concatenate([[0], np.cumsum(blocks)]).astype(np.int64)
    return base[:-1], int(base[-1])


def project_composite(objects, sh_components, cam, w, h, color_space=0):
    """objects: [(world, harmonics, model matrix (column-major flat 4x4) or None)], all seen by the frame camera
    `cam`.  Each object is projected from its model matrix (project(..., scene_transform=M, pose=True)) and the
    projections are laid out by item.  Returns (projection over all items -- entries that belong to no gaussian
    are not visible and hold NaN --, visible [items], owner [items, 2] = (object, gaussian), -1 for no owner)."""
    counts = [len(o[0]) for o in objects]
    base, items = item_layout(counts)
    owner = np.full((items, 2), -1, np.int64)
    out = None
    for o, (world, harm, model) in enumerate(objects):
        if len(world) == 0:
            continue
        pr = project(world, harm, sh_components, cam, w, h, color_space, scene_transform=model,
                     pose=model is not None)
        if out is None:
            out = {}
            for k, v in pr.items():
                if k == "margins":
                    out[k] = {m: np.full(items, -np.inf) for m in v}
                else:
                    fill = False if v.dtype == bool else (-np.inf if k == "margin" else np.nan)
                    out[k] = np.full((items,) + v.shape[1:], fill, v.dtype)
        sl = slice(int(base[o]), int(base[o]) + len(world))
        for k, v in pr.items():
            if k == "margins":
                for m in v:
                    out[k][m][sl] = v[m]
            else:
                out[k][sl] = v
        owner[sl, 0], owner[sl, 1] = o, np.arange(len(world))
    return out, out["visible"].copy(), owner


# ---------------------------------------------------------------------------------------------------
# styles and the selects
# ---------------------------------------------------------------------------------------------------
# a style: (tint r, g, b, tint amount k, opacity scale s, hidden), all bytes
IDENTITY_STYLE = (0, 0, 0, 0, 255, 0)


def styles_of(states, styles, style_count=None):
    """[n, 6] int64: every gaussian's style; states at or above style_count take the identity."""
    table = np.asarray(list(styles), np.int64).reshape(-1, 6)
    count = len(table) if style_count is None else int(style_count)
    states = np.asarray(states, np.int64)
    out = np.tile(np.asarray(IDENTITY_STYLE, np.int64), (len(states), 1))
    known = states < count
    out[known] = table[states[known]]
    return out


def apply_styles(pr, states, styles, style_count=None):
    """A projection under a style table (rows of six bytes as IDENTITY_STYLE) and one state byte per entry.
    Hidden gaussians leave the visible set (margin 'style').  Each colour byte becomes
    (c (255 - k) + t k + 127) // 255 and the opacity byte (o s + 127) // 255, on the truncated bytes of
    quantise_global; 'color' and 'opacity' of the result hold byte / 255, 'styled_bytes' [n, 4] the bytes
    (r, g, b, opacity) themselves, 'plain_color' and 'plain_opacity' the values before the style.  A gaussian whose styled opacity byte is 0 stays visible ('no_tiles')."""
    st = styles_of(states, styles, style_count)
    hidden = st[:, 5] != 0
    byte = lambda v: np.floor(np.clip(np.nan_to_num(v) * 255.0, 0.0, 255.0)).astype(np.int64)
    c, o = byte(pr["color"]), byte(pr["opacity"])
    k = st[:, 3:4]
    c2 = (c * (255 - k) + st[:, 0:3] * k + 127) // 255
    o2 = (o * st[:, 4] + 127) // 255
    out = dict(pr)
    out["margins"] = dict(pr["margins"], style=np.where(hidden, -np.inf, np.inf))
    out["margin"] = np.where(hidden, -np.inf, pr["margin"])
    out["visible"] = pr["visible"] & ~hidden
    out["styled_bytes"] = np.concatenate([c2, o2[:, None]], 1)
    out["plain_color"], out["plain_opacity"] = pr["color"], pr["opacity"]
    out["color"], out["opacity"] = c2 / 255.0, o2 / 255.0
    out["no_tiles"] = out["visible"] & (o2 == 0)
    return out


def quantise_styled(spr) -> dict:
    """quantise_global of a styled projection: the colour and opacity bytes are already whole."""
    q = quantise_global(spr)
    q["color"], q["opacity"] = spr["styled_bytes"][:, :3] / 255.0, spr["styled_bytes"][:, 3] / 255.0
    return q


def _update(states, match, and_mask, xor_mask):
    out = np.asarray(states, np.uint8).copy()
    out[match] = ((out[match].astype(np.int64) & (and_mask & 0xFFFFFFFF)) ^ (xor_mask & 0xFFFFFFFF)) & 0xFF
    return out


def select_mask(pr, states, mask, w, h, and_mask, xor_mask, styles=None, style_count=None, eps=0.0):
    """gsm_global_select_mask on a model projection: a gaussian matches when it is visible, its current style is
    not hidden, its fp16 mean is finite and floor(mean + 0.5) names a pixel of the frame whose mask byte is
    nonzero.  Returns (new states, matches, in doubt [n]): in doubt is a visible gaussian whose mean lies within
    eps of a rounding boundary of its fp16 value or of a k + 0.5 (the pixel could be the neighbour)."""
    states = np.asarray(states, np.uint8)
    match = pr["visible"].copy()
    if styles is not None:
        match &= styles_of(states, styles, style_count)[:, 5] == 0
    with np.errstate(invalid="ignore", over="ignore"):
        m16 = round_h(pr["mean"])
        match &= np.isfinite(m16).all(1)
        px = np.floor(m16 + 0.5)
        inside = (px[:, 0] >= 0) & (px[:, 0] < w) & (px[:, 1] >= 0) & (px[:, 1] < h)
        match &= inside
        ix = np.where(match, px[:, 0], 0).astype(np.int64)
        iy = np.where(match, px[:, 1], 0).astype(np.int64)
        match &= np.asarray(mask)[iy, ix] != 0
        m = pr["mean"]
        f = np.mod(m + 0.5, 1.0)
        doubt = (np.abs(np.abs(m - m16) - 0.5 * h_ulp(m)) < eps) | (np.minimum(f, 1.0 - f) < eps)
        doubt = doubt.any(1) & np.isfinite(m).all(1)
    return _update(states, match, and_mask, xor_mask), int(match.sum()), doubt


def select_pick(items, counts, obj, states, gaussian_count, and_mask, xor_mask, mask=None):
    """gsm_global_select_pick from its rule: with object o's items at
    [256 B_o, 256 B_o + count_o), S is the set of ids item - 256 B_o of the pixels under the mask (None: every
    pixel) that lie below min(count_o, gaussian_count); every id of S is updated once.  The rule reads an image,
    not the scene, so nothing of it is in doubt: returns (new states, |S|, in doubt = all False)."""
    base, _ = item_layout(counts)
    items = np.asarray(items).astype(np.int64)
    hh, ww = items.shape
    under = np.ones((hh, ww), bool) if mask is None else np.asarray(mask)[:hh, :ww] != 0
    ids = items[under] - int(base[obj])
    ids = np.unique(ids[(ids >= 0) & (ids < min(int(counts[obj]), int(gaussian_count)))])
    match = np.zeros(len(states), bool)
    match[ids] = True
    return _update(states, match, and_mask, xor_mask), int(len(ids)), np.zeros(len(states), bool)
