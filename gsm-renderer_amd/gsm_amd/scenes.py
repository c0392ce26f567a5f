"""Synthetic Gaussian clouds and cameras for the benchmark configs.

Modelled on the reference's fixture generator generateVisibleGaussians
(Tests/RendererTests/TestUtils.swift:189-231: z ~ U[1.5, 9.5], x,y ~ U[-1,1]*0.6z,
opacity ~ U[0.5,1]) and camera makeProjectionMatrix/makeCameraParams
(TestUtils.swift:37-94: 60 deg fov, near 0.1, far 10, OpenCV +Z forward, identity
view).  The scale is changed for density: log-uniform scales tuned so a
frame has ~2.6 tile assignments per gaussian at every resolution (measured with the
oracle: scale_px 0.8/1.0/1.2/1.5 -> A/N 1.99/2.30/2.62/3.13), inside the reference's
4*N assignment capacity and its 16.78M radix-sort limit at 5M/4K.  Quaternions are random unit vectors, SH DC ~ U[0,1] and
higher bands ~ N(0, 0.1) clipped to +-0.3.  numpy PCG64, seeded.
"""
from __future__ import annotations

import math

import numpy as np

from .types import WORLD16, WORLD32


def projection_matrix(width: int, height: int, near: float = 0.1, far: float = 10.0,
                      fov_degrees: float = 60.0) -> np.ndarray:
    """makeProjectionMatrix, OpenCV convention (TestUtils.swift:37-71), column-major flat."""
    aspect = np.float32(width) / np.float32(height)
    fov = np.float32(fov_degrees) * np.float32(math.pi) / np.float32(180.0)
    f = np.float32(1.0) / np.float32(math.tan(float(fov) / 2.0))
    P = np.zeros(16, np.float32)
    P[0] = f / aspect
    P[5] = f
    P[10] = np.float32(far) / (np.float32(far) - np.float32(near))
    P[11] = 1.0
    P[14] = -(np.float32(far) * np.float32(near)) / (np.float32(far) - np.float32(near))
    return P


def make_camera(width: int, height: int, eye_offset_x: float = 0.0) -> dict:
    """makeCameraParams (TestUtils.swift:74-94); eye_offset_x shifts the camera for stereo."""
    P = projection_matrix(width, height)
    V = np.eye(4, dtype=np.float32).reshape(-1)  # column-major identity
    V[12] = -np.float32(eye_offset_x)            # translation column (view = T(-eye))
    aspect = width / height
    f = float(P[5])
    return {"view": V, "proj": P, "position": np.array([eye_offset_x, 0.0, 0.0], np.float32),
            "focal_x": width * f / (2 * aspect), "focal_y": height * f / 2, "near": 0.1, "far": 10.0}


def ortho_camera(width: int, height: int, half_height: float, near: float = 0.1, far: float = 10.0,
                 view=None) -> dict:
    """An orthographic camera for a frame with the orthographic flag (GlobalRenderer.render_frame(...,
    orthographic=True)), in make_camera's convention -- looking down +z, depth in [0, 1]: the view volume is
    2 * half_height world units high and aspect times as wide, p00 = 1 / (half_height * aspect), p11 = 1 /
    half_height, p10 = 1 / (far - near), p14 = -near / (far - near), p15 = 1 (column-major flat).  view: a
    column-major flat 4x4 (None: the identity).  An orthographic camera has no position: the field is zero and
    the frame ignores it; focal_x / focal_y are pixels per world unit."""
    aspect = np.float32(width) / np.float32(height)
    hh = np.float32(half_height)
    P = np.zeros(16, np.float32)
    P[0] = np.float32(1.0) / (hh * aspect)
    P[5] = np.float32(1.0) / hh
    P[10] = np.float32(1.0) / (np.float32(far) - np.float32(near))
    P[14] = -np.float32(near) / (np.float32(far) - np.float32(near))
    P[15] = 1.0
    V = np.eye(4, dtype=np.float32).reshape(-1) if view is None else \
        np.asarray(view, np.float32).reshape(-1).copy()
    return {"view": V, "proj": P, "position": np.zeros(3, np.float32),
            "focal_x": float(width * P[0] * np.float32(0.5)), "focal_y": float(height * P[5] * np.float32(0.5)),
            "near": float(near), "far": float(far)}


def orbit_camera(width: int, height: int, angle_deg: float, pivot_z: float = 5.5) -> dict:
    """make_camera's camera moved on a circle about the y axis through (0, 0, pivot_z), still looking
    at that point: angle 0 is make_camera itself.  Used for the moving-camera benchmark (bench.py
    --camera-path orbit), where every frame sees a slightly different view."""
    a = math.radians(angle_deg)
    c, s = np.float32(math.cos(a)), np.float32(math.sin(a))
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)        # camera-to-world rotation
    pos = np.array([0, 0, pivot_z], np.float32) + R @ np.array([0, 0, -pivot_z], np.float32)
    Rt = R.T
    t = -(Rt @ pos)
    V = np.eye(4, dtype=np.float32)
    V[:3, :3] = Rt
    V[:3, 3] = t
    cam = make_camera(width, height)
    cam["view"] = V.T.reshape(-1).astype(np.float32)  # column-major flat
    cam["position"] = pos.astype(np.float32)
    return cam


def object_camera(cam: dict, model) -> dict:
    """The camera `cam` as seen from the space of an object with model matrix `model` (4x4, column-major flat
    like scene_transform: object space -> world space), for GlobalRenderer.render_composite: view * M and
    M^-1 * position, computed in float64 and rounded once to float32; everything else of `cam` unchanged.
    Exact for a rotation, a translation and a uniform scale (the gaussians' scales stay in object space)."""
    M = np.asarray(model, np.float64).reshape(4, 4).T  # column-major flat -> the matrix
    out = dict(cam)
    out["proj"] = np.asarray(cam["proj"], np.float32).reshape(-1).copy()
    if np.array_equal(M, np.eye(4)):  # the camera's own words (a product's sums would turn a -0 into +0)
        out["view"] = np.asarray(cam["view"], np.float32).reshape(-1).copy()
        out["position"] = np.asarray(cam["position"], np.float32).reshape(-1).copy()
        return out
    V = np.asarray(cam["view"], np.float64).reshape(4, 4).T
    p = np.append(np.asarray(cam["position"], np.float64).reshape(3), 1.0)
    q = np.linalg.inv(M) @ p
    out["view"] = (V @ M).T.reshape(-1).astype(np.float32)
    out["position"] = (q[:3] / q[3]).astype(np.float32)
    return out


def pose_matrix(rotation, scale: float, translation) -> np.ndarray:
    """The model matrix of a rotation (3x3, rows by columns), a uniform scale and a translation: sixteen float64,
    column-major flat like `model` of object_camera and scene_transform, with scale * rotation in its upper 3x3 and
    the translation in its last column.  Transform.from_matrix takes it apart again."""
    M = np.eye(4)
    M[:3, :3] = float(scale) * np.asarray(rotation, np.float64).reshape(3, 3)
    M[:3, 3] = np.asarray(translation, np.float64).reshape(3)
    return M.T.reshape(16).copy()


def box_to_shape(center, half_extents, rotation=None) -> np.ndarray:
    """SelectQuery.to_shape of an oriented box (GlobalRenderer.select_where, SELECT_BOX; with SELECT_ELLIPSOID the
    ellipsoid inscribed in it): twelve float32, the row-major 3x4 that takes scene space to the box's unit cube.
    rotation: a 3x3 whose rows are the box axes (unit vectors; None: the scene's axes).  Row r is rotation[r] /
    half_extents[r], with -dot(rotation[r], center) / half_extents[r] in its fourth column; computed in float64
    and rounded once to float32."""
    c = np.asarray(center, np.float64).reshape(3)
    h = np.asarray(half_extents, np.float64).reshape(3)
    R = np.eye(3) if rotation is None else np.asarray(rotation, np.float64).reshape(3, 3)
    A = np.empty((3, 4), np.float64)
    A[:, :3] = R / h[:, None]
    A[:, 3] = -(R @ c) / h
    return A.astype(np.float32).reshape(12)


def sphere_to_shape(center, radius: float) -> np.ndarray:
    """SelectQuery.to_shape of a sphere (SELECT_ELLIPSOID): box_to_shape of its bounding cube."""
    return box_to_shape(center, (radius, radius, radius))


def _f16_bits(x: np.ndarray) -> np.ndarray:
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def gen_scene(count: int, width: int, height: int, sh_components: int, precision: int,
              seed: int = 42, scale_px: float = 1.2, spread: float = 0.6):
    """Returns (world structured array, harmonics array (float32 or fp16 bits), camera dict).

    precision: 0 -> PackedWorldGaussian + f32 SH, 1 -> PackedWorldGaussianHalf + f16 SH."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.5, 9.5, count).astype(np.float32)
    x = (rng.uniform(-1.0, 1.0, count) * spread * z).astype(np.float32)
    y = (rng.uniform(-1.0, 1.0, count) * spread * z).astype(np.float32)
    f_px = (height / 2.0) / math.tan(math.radians(30.0))
    s_med = scale_px * 5.5 / f_px
    s = (s_med * np.exp(rng.uniform(-1.0, 1.0, (count, 3)) * 0.6)).astype(np.float32)
    q = rng.normal(size=(count, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    op = rng.uniform(0.5, 1.0, count).astype(np.float32)
    k = max(int(sh_components), 1)
    harm = np.zeros((count, 3, k), np.float32)
    harm[:, :, 0] = rng.uniform(0.0, 1.0, (count, 3))
    if k > 1:
        harm[:, :, 1:] = np.clip(rng.normal(0.0, 0.1, (count, 3, k - 1)), -0.3, 0.3)
    harm = harm.reshape(-1)  # planar per gaussian: [R0..Rk-1, G0.., B0..]
    if precision == 0:
        w = np.zeros(count, WORLD32)
        w["px"], w["py"], w["pz"] = x, y, z
        w["opacity"] = op
        w["sx"], w["sy"], w["sz"] = s[:, 0], s[:, 1], s[:, 2]
        w["rot"] = q
        h = harm
    else:
        w = np.zeros(count, WORLD16)
        w["px"], w["py"], w["pz"] = x, y, z
        w["opacity"] = _f16_bits(op)
        w["sx"], w["sy"], w["sz"] = _f16_bits(s[:, 0]), _f16_bits(s[:, 1]), _f16_bits(s[:, 2])
        w["rx"], w["ry"], w["rz"], w["rw"] = (_f16_bits(q[:, i]) for i in range(4))
        h = _f16_bits(harm)
    return w, h, make_camera(width, height)


# Benchmark / parity configurations (BASELINE.json "configs")
CONFIGS = {
    "cfg1_50k_sh0_640x360_f32": dict(count=50_000, width=640, height=360, sh=1, precision=0),
    "cfg2_1m_sh3_1080p_f16": dict(count=1_000_000, width=1920, height=1080, sh=16, precision=1),
    "cfg3_5m_sh3_4k_f16": dict(count=5_000_000, width=3840, height=2160, sh=16, precision=1),
    # config 5: two eyes of 1440x1600 side by side (width = per eye), +-32 mm x offsets
    "cfg5_1m_sh2_stereo_2x1440x1600_f16": dict(count=1_000_000, width=1440, height=1600, sh=9, precision=1,
                                               stereo=0.032),
}
