"""A float64 model of the orthographic frame (TEST INFRASTRUCTURE).

Second derivation of the orthographic projection rule, independent of tests/ortho/ortho_ref.c and of the HIP
kernels: plain numpy, float64 throughout, written from the mathematics of a parallel projection.

* The mean is affine: pixel = S (P V x) with S the ndc -> pixel map, no division.
* The footprint is the image of the 3-D covariance under the map's (constant) linear part,
  J R S^2 R^T J^T + 0.3 I with J = d(pixel) / d(world) = S' P3 V3 -- formed here as ONE 2x3 matrix from whole-matrix
  products, not as the checker's J * W then T * C3 * T^T sequence over a diagonal J.
* Every ray is parallel.  The camera's axis in world space is the direction along which the picture does not
  change: the null vector of the 2x3 linear part (taken from its SVD, not read out of a row or a column of `view`).
  It is oriented toward the camera by the direction in which the depth decreases.
* Depth runs along the axis: the view-space z of the point, signed so that it grows away from the camera, the
  camera looking down +z when proj's z scale is positive (Metal's convention) and down -z otherwise.

Everything downstream of the projection -- the eigen-decomposition, the extents, the cull margins, the record
quantisation, the order and the blend -- is what tests/f64_model.py says for the perspective frame; its functions
are imported, and the part of M.project's text that follows the covariance is repeated here, with the orthographic
depth in the near and ink margins.  A composite's object is taken from its model matrix, as M.project(pose=True) does.
"""
from __future__ import annotations

import numpy as np

import f64_model as M

PI = M.PI


def camera_axis(V, P):
    """(toward [3], sign): the unit world-space direction from the scene toward the camera, and the sign of the
    view's z along which depth grows.  The axis is the null direction of the linear part of world -> ndc xy."""
    L = (P[:2, :3] @ V[:3, :3])
    axis = np.linalg.svd(L)[2][2]           # unit, L @ axis = 0 (an orthographic map of rank 2)
    sign = 1.0 if P[2, 2] >= 0 else -1.0    # depth = sign * view z
    grows = sign * (V[2, :3] @ axis)        # d(depth) / d(step along axis)
    return (-axis if grows > 0 else axis), sign


def project(world, harm, sh_components, cam, w, h, color_space=0, model=None):
    """Every gaussian through the orthographic projection, in float64: M.project's dictionary.  model: a
    composite object's model matrix (column-major flat, object -> world), `cam` being the frame's camera."""
    n = len(world)
    k = max(int(sh_components), 1)
    pos, scale, quat, op = M.unpack_world(world)
    A = np.eye(3)
    if model is not None:
        S = M._mat(model)
        A = S[:3, :3]
        pos = (np.concatenate([pos, np.ones((n, 1))], 1) @ S.T)[:, :3]
    V, P = M._mat(cam["view"]), M._mat(cam["proj"])
    near, far = float(cam["near"]), float(cam["far"])
    W, H = float(w), float(h)
    toward, sign = camera_axis(V, P)
    with np.errstate(all="ignore"):
        x4 = np.concatenate([pos, np.ones((n, 1))], 1)
        view4 = x4 @ V.T
        depth = sign * view4[:, 2]
        ndc = x4 @ (P @ V)[:2].T            # the first two rows of the affine map; its last row is (0 0 0 1)
        mean = (ndc + 1.0) * 0.5 * np.array([W, H]) - 0.5

        R = M.rotation_from_quaternion(quat)
        cov_obj = R @ (scale[:, :, None] ** 2 * np.transpose(R, (0, 2, 1)))
        J = 0.5 * np.array([[W], [H]]) * (P[:2, :3] @ V[:3, :3] @ A)   # d(pixel) / d(object position), constant
        c2 = J[None] @ cov_obj @ J.T[None]
        a, b, d = c2[:, 0, 0] + M.DILATION, 0.5 * (c2[:, 0, 1] + c2[:, 1, 0]), c2[:, 1, 1] + M.DILATION

        det = a * d - b * b
        mid = 0.5 * (a + d)
        root = np.sqrt(np.maximum(mid * mid - det, 0.0))
        lam1, lam2 = mid + root, mid - root
        sigma = np.sqrt(np.stack([lam1, lam2], 1))
        theta = np.mod(0.5 * np.arctan2(2.0 * b, a - d), PI)
        conic = np.stack([d, -b, a], 1) / det[:, None]
        ct, st = np.abs(np.cos(theta)), np.abs(np.sin(theta))
        e1, e2 = M.EXTENT_SIGMAS * sigma[:, 0], M.EXTENT_SIGMAS * sigma[:, 1]
        extent = np.stack([ct * e1 + st * e2, st * e1 + ct * e2], 1)
        max_extent = 2.0 * max(W, H) / 3.0
        repair = ~np.isfinite(a + b + d) | (lam1 > max_extent ** 2) | \
            (lam2 * M.MAX_AXIS_RATIO ** 2 < lam1) | (det < 1e-8)

        m = {}
        m["scale"] = scale.max(1) / M.MIN_SCALE - 1.0
        m["near"] = depth / near - 1.0
        m["alpha"] = op / M.ALPHA_THRESHOLD - 1.0
        m["radius"] = 3.0 * sigma[:, 0] / M.MIN_RADIUS - 1.0
        m["ink"] = M.ink_margin(op, det, depth, near, far)
        lo, hi = mean - extent, mean + extent
        m["screen"] = np.minimum(np.minimum(hi[:, 0], W - lo[:, 0]), np.minimum(hi[:, 1], H - lo[:, 1])) / max(W, H)
        for key in m:
            m[key] = np.where(np.isfinite(m[key]), m[key], -np.inf)
        repair &= (m["scale"] > 0) & (m["near"] > 0) & (m["alpha"] > 0)
        margin = np.min(np.stack(list(m.values()), 1), 1)
        visible = margin > 0.0

        # one direction for the whole object: the ray toward the camera, seen in the object's frame
        ray = np.linalg.inv(A) @ toward
        dirs = np.broadcast_to(ray / np.linalg.norm(ray), (n, 3))
        coef = M.unpack_harmonics(harm, n, k)
        if k == 1:
            color = coef[:, :, 0] * M.sh_basis(np.array([0.0, 0.0, 1.0]))[0]
        else:
            color = np.einsum("nck,nk->nc", coef[:, :, :min(k, 16)], M.sh_basis(dirs)[:, :min(k, 16)])
        color = np.maximum(color + 0.5, 0.0)
        if color_space == 1:
            color = M.srgb_decode(color)

    return dict(view=view4[:, :3], depth=depth, mean=mean, cov2d=np.stack([a, b, d], 1), det=det, sigma=sigma,
                theta=theta, conic=conic, color=color, opacity=op, extent=extent, margins=m, margin=margin,
                visible=visible, repair=repair)


def project_composite(objects, sh_components, cam, w, h, color_space=0):
    """M.project_composite under the orthographic rule: (projection by item, visible [items], owner [items, 2])."""
    counts = [len(o[0]) for o in objects]
    base, items = M.item_layout(counts)
    owner = np.full((items, 2), -1, np.int64)
    out = None
    for o, (world, harm, model) in enumerate(objects):
        if len(world) == 0:
            continue
        pr = project(world, harm, sh_components, cam, w, h, color_space, model=model)
        if out is None:
            out = {}
            for key, v in pr.items():
                if key == "margins":
                    out[key] = {name: np.full(items, -np.inf) for name in v}
                else:
                    fill = False if v.dtype == bool else (-np.inf if key == "margin" else np.nan)
                    out[key] = np.full((items,) + v.shape[1:], fill, v.dtype)
        sl = slice(int(base[o]), int(base[o]) + len(world))
        for key, v in pr.items():
            if key == "margins":
                for name in v:
                    out[key][name][sl] = v[name]
            else:
                out[key][sl] = v
        owner[sl, 0], owner[sl, 1] = o, np.arange(len(world))
    return out, out["visible"].copy(), owner
