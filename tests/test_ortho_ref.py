"""The orthographic frames' checker (tests/ortho/ortho_ref.c) on the CPU: the restatement against the
oracle, and every rule of the orthographic projection from the checker's own output."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def f16(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def world32(pos, scale=0.05, opacity=0.99, rot=(0, 0, 0, 1)):
    import oracle as O
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    w = np.zeros(len(pos), O.WORLD32)
    w["px"], w["py"], w["pz"] = pos[:, 0], pos[:, 1], pos[:, 2]
    w["opacity"] = opacity
    s = np.broadcast_to(np.asarray(scale, np.float32), (len(pos), 3))
    w["sx"], w["sy"], w["sz"] = s[:, 0], s[:, 1], s[:, 2]
    w["rot"] = np.asarray(rot, np.float32)
    return w


def dc(n, rgb=(0.5, 0.2, -0.1)):
    return np.tile(np.asarray(rgb, np.float32), n)


def test_flag_off_is_the_oracles_frame(oracle):
    """proj a perspective matrix, the flag off: every stage's bytes are oracle.render's (guards the restatement)."""
    import ortho_ref
    from gsm_amd import scenes
    for prec, sh, n, w, h in [(0, 16, 3001, 200, 120), (1, 4, 1500, 97, 45)]:
        world, harm, cam = scenes.gen_scene(n, w, h, sh, prec, seed=5)
        ref = oracle.render(world, harm, sh, cam, w, h, max_gaussians=n)
        got = ortho_ref.render(world, harm, sh, cam, w, h, orthographic=False, max_gaussians=n)
        for k in ("render_data", "bounds", "tile_counts", "sorted_keys", "sorted_values", "headers", "color", "depth"):
            assert np.array_equal(np.asarray(got[k]).view(np.uint8), np.asarray(ref[k]).view(np.uint8)), k
        assert got["total_assignments"] == ref["total_assignments"] > 0


def test_depth_orders_the_frame_and_sigma_flips_it(oracle):
    """Two opaque overlapping gaussians at different vp.z blend in d order; with proj[10] < 0 sigma = -1, d = -vp.z,
    and the two swap."""
    import ortho_ref
    from gsm_amd import scenes
    w, h = 64, 32
    harm = np.concatenate([dc(1, (2.0, -2.0, -2.0)), dc(1, (-2.0, -2.0, 2.0))])  # red, blue
    cam = scenes.ortho_camera(w, h, 1.0)
    near = world32([[0, 0, 2.0], [0, 0, 4.0]], scale=0.3)
    a = ortho_ref.render(near, harm, 1, cam, w, h)
    assert a["mask"].tolist() == [1, 1]
    assert f16(a["render_data"]["depth"]).tolist() == [2.0, 4.0]
    tile = a["sorted_keys"] >> 16
    first = {t: int(v) for t, v in zip(tile[::-1], a["sorted_values"][::-1])}  # the first entry of every tile
    assert set(first.values()) == {0}, "the nearer gaussian leads every tile"
    px = f16(a["color"][h // 2, w // 2])
    assert px[0] > 0.9 and px[2] < 0.05, "red in front"
    # sigma flips with proj[10]: the scene mirrored in z, d = -vp.z
    flip = dict(cam)
    flip["proj"] = cam["proj"].copy()
    flip["proj"][10] = -cam["proj"][10]
    far = world32([[0, 0, -2.0], [0, 0, -4.0]], scale=0.3)
    b = ortho_ref.render(far, harm, 1, flip, w, h)
    assert f16(b["render_data"]["depth"]).tolist() == [2.0, 4.0]
    assert np.array_equal(b["color"], a["color"]) and np.array_equal(b["sorted_values"], a["sorted_values"])
    # the same two under +sigma are behind the camera; under -sigma the first scene is
    assert ortho_ref.render(far, harm, 1, cam, w, h)["mask"].tolist() == [0, 0]
    assert ortho_ref.render(near, harm, 1, flip, w, h)["mask"].tolist() == [0, 0]
    # and swapping the two depths swaps the order
    swapped = world32([[0, 0, 4.0], [0, 0, 2.0]], scale=0.3)
    c = ortho_ref.render(swapped, harm, 1, cam, w, h)
    px = f16(c["color"][h // 2, w // 2])
    assert px[2] > 0.9 and px[0] < 0.05, "blue in front"


def test_translation_along_the_axis_changes_only_the_depth(oracle):
    """Positions and a step that are exact in float32 (multiples of 1/64, a step of 2): meanX, meanY, theta, sigma1,
    sigma2 and the colour are bit-identical, the depth moves by the step."""
    import ortho_ref
    from gsm_amd import scenes
    rng = np.random.default_rng(11)
    n, w, h, sh = 400, 200, 120, 16
    pos = np.stack([rng.integers(-96, 97, n) / 64.0, rng.integers(-64, 65, n) / 64.0, rng.integers(64, 256, n) / 64.0], 1)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    world = world32(pos, scale=rng.uniform(0.02, 0.2, (n, 3)), opacity=0.9, rot=q)
    harm = np.clip(rng.normal(0, 0.3, n * 3 * sh), -1, 1).astype(np.float32)
    cam = scenes.ortho_camera(w, h, 1.25)
    a = ortho_ref.render(world, harm, sh, cam, w, h)
    moved = world.copy()
    moved["pz"] += np.float32(2.0)
    b = ortho_ref.render(moved, harm, sh, cam, w, h)
    assert a["mask"].sum() > n // 2 and np.array_equal(a["mask"], b["mask"])
    vis = a["mask"] == 1
    for k in ("meanX", "meanY", "theta", "sigma1", "sigma2", "colorR", "colorG", "colorB", "opacity"):
        assert np.array_equal(a["render_data"][k][vis], b["render_data"][k][vis]), k
    assert np.array_equal(a["bounds"], b["bounds"]) and np.array_equal(a["tile_counts"], b["tile_counts"])
    da, db = f16(a["render_data"]["depth"][vis]), f16(b["render_data"]["depth"][vis])
    assert np.array_equal(db, np.float16(da + 2.0).astype(np.float64)) and (db > da).all()
    # the perspective rule does not have this property: the same move changes the means
    pcam = scenes.make_camera(w, h)
    pa = ortho_ref.render(world, harm, sh, pcam, w, h, orthographic=False)
    pb = ortho_ref.render(moved, harm, sh, pcam, w, h, orthographic=False)
    both = (pa["mask"] == 1) & (pb["mask"] == 1)
    assert (pa["render_data"]["meanX"][both] != pb["render_data"]["meanX"][both]).any()


def test_near_cull_is_on_d(oracle):
    """d = near is culled (the test is !(d > near)), the next float above it is kept; clip.w = 1 plays no part."""
    import ortho_ref
    from gsm_amd import scenes
    w, h = 64, 32
    near = np.float32(0.5)
    cam = scenes.ortho_camera(w, h, 1.0, near=float(near), far=10.0)
    zs = [np.nextafter(near, np.float32(0)), near, np.nextafter(near, np.float32(1)), np.float32(0.75)]
    r = ortho_ref.render(world32([[0, 0, z] for z in zs], scale=0.2), dc(4), 1, cam, w, h)
    assert r["mask"].tolist() == [0, 0, 1, 1]
    far_near = scenes.ortho_camera(w, h, 1.0, near=2.0, far=10.0)  # every gaussian has clip.w = 1 < near
    r = ortho_ref.render(world32([[0, 0, 1.5], [0, 0, 2.5]], scale=0.2), dc(2), 1, far_near, w, h)
    assert r["mask"].tolist() == [0, 1]


def test_colour_does_not_depend_on_the_camera_position(oracle):
    import ortho_ref
    from gsm_amd import scenes
    n, w, h, sh = 1500, 200, 120, 16
    world, harm, _ = scenes.gen_scene(n, w, h, sh, 0, seed=9)
    cam = scenes.ortho_camera(w, h, 3.0)
    a = ortho_ref.render(world, harm, sh, cam, w, h)
    moved = dict(cam)
    moved["position"] = np.array([3.0, -7.0, 11.0], np.float32)
    b = ortho_ref.render(world, harm, sh, moved, w, h)
    assert a["mask"].sum() > 200
    assert np.array_equal(a["render_data"], b["render_data"]) and np.array_equal(a["color"], b["color"])
    # the direction is the view's: a rotated view changes the colours of a degree-3 scene
    c, s = np.float32(np.cos(0.6)), np.float32(np.sin(0.6))
    V = np.eye(4, dtype=np.float32)
    V[0, 0], V[0, 2], V[2, 0], V[2, 2] = c, s, -s, c
    V[:3, 3] = (-V[:3, :3] @ np.array([0, 0, 5.5], np.float32)) + np.array([0, 0, 5.5], np.float32)
    rot = scenes.ortho_camera(w, h, 3.0, view=V.T.reshape(-1))
    r = ortho_ref.render(world, harm, sh, rot, w, h)
    both = (a["mask"] == 1) & (r["mask"] == 1)
    assert both.sum() > 100 and (a["render_data"]["colorR"][both] != r["render_data"]["colorR"][both]).any()
    # the perspective rule does depend on it
    pcam = scenes.make_camera(w, h)
    pmoved = dict(pcam)
    pmoved["position"] = moved["position"]
    pa = ortho_ref.render(world, harm, sh, pcam, w, h, orthographic=False)
    pb = ortho_ref.render(world, harm, sh, pmoved, w, h, orthographic=False)
    assert not np.array_equal(pa["render_data"], pb["render_data"])
    # degree 0 is unchanged by the rule: the DC colour
    a0 = ortho_ref.render(world, harm[:n * 3].copy(), 1, cam, w, h)
    vis = a0["mask"] == 1
    dc0 = np.float32(harm[:n * 3].reshape(n, 3)[:, 0]) * np.float32(0.28209479177387814)
    want = np.clip(np.maximum(dc0 + np.float32(0.5), 0) * np.float32(255.0), 0, 255).astype(np.uint8)
    assert np.array_equal(a0["render_data"]["colorR"][vis], want[vis])


def test_footprint_is_the_affine_image_of_the_covariance(oracle):
    """An isotropic gaussian of scale s under J = diag(jx, jy): sigmas sqrt(s^2 j^2 + 0.3), whatever its depth."""
    import ortho_ref
    from gsm_amd import scenes
    w, h = 200, 120
    cam = scenes.ortho_camera(w, h, 1.5)
    jx, jy = w * float(cam["proj"][0]) * 0.5, h * float(cam["proj"][5]) * 0.5
    r = ortho_ref.render(world32([[0.25, -0.5, 2.0], [0.25, -0.5, 8.0]], scale=0.1), dc(2), 1, cam, w, h)
    rd = r["render_data"]
    assert rd["sigma1"][0] == rd["sigma1"][1] and rd["meanX"][0] == rd["meanX"][1]
    s = np.sqrt(0.01 * jx * jy + 0.3)
    assert abs(f16(rd["sigma1"][0]) - s) < 2e-3 * s and abs(f16(rd["sigma2"][0]) - s) < 2e-3 * s
    assert abs(f16(rd["meanX"][0]) - ((0.25 * float(cam["proj"][0]) + 1) * w - 1) / 2) < 0.1
    assert abs(f16(rd["meanY"][0]) - ((-0.5 * float(cam["proj"][5]) + 1) * h - 1) / 2) < 0.1


def test_a_rect_of_more_than_32_tiles_takes_count_ranges_count(oracle):
    """A large gaussian: its rect exceeds 32 tiles and its tile count is the number of keys count_range / the scatter
    gave it -- fewer than the rect's tiles (the ellipse test ran), more than 32."""
    import ortho_ref
    from gsm_amd import scenes
    w, h = 640, 360
    cam = scenes.ortho_camera(w, h, 2.0)
    world = world32([[0.3, 0.1, 3.0], [-1.0, 0.5, 4.0]], scale=[[0.9, 0.15, 0.1], [0.05, 0.05, 0.05]],
                    rot=[[0, 0, 0.38268343, 0.92387953], [0, 0, 0, 1]])
    r = ortho_ref.render(world, dc(2), 1, cam, w, h, max_gaussians=4096)
    b = r["bounds"][0]
    rect = (b[1] - b[0] + 1) * (b[3] - b[2] + 1)
    assert rect > 32 and r["overflow"] == 0
    assert 32 < r["tile_counts"][0] < rect
    assert int((r["values"] == 0).sum()) == r["tile_counts"][0]
    assert r["total_assignments"] == int(r["tile_counts"].sum())


def test_object_camera_works_on_an_orthographic_camera(oracle):
    """A composite of one object under object_camera(cam, M) equals the single frame of the moved scene under cam,
    for a translation that is exact in float32."""
    import ortho_ref
    from gsm_amd import scenes
    n, w, h, sh = 600, 200, 120, 1
    world, harm, _ = scenes.gen_scene(n, w, h, sh, 0, seed=4)
    world["px"] = np.round(world["px"] * 64) / 64
    world["py"] = np.round(world["py"] * 64) / 64
    world["pz"] = np.round(world["pz"] * 64) / 64
    cam = scenes.ortho_camera(w, h, 3.0)
    M = np.eye(4)
    M[:3, 3] = [0.5, -0.25, 1.0]
    oc = scenes.object_camera(cam, M.T.reshape(-1))
    assert np.array_equal(oc["proj"], cam["proj"]) and oc["near"] == cam["near"]
    moved = world.copy()
    moved["px"] += np.float32(0.5)
    moved["py"] -= np.float32(0.25)
    moved["pz"] += np.float32(1.0)
    a = ortho_ref.render(world, harm, sh, oc, w, h)
    b = ortho_ref.render(moved, harm, sh, cam, w, h)
    assert a["mask"].sum() > 100
    assert np.array_equal(a["render_data"], b["render_data"]) and np.array_equal(a["color"], b["color"])


def test_ortho_camera_matrix():
    from gsm_amd import scenes
    cam = scenes.ortho_camera(200, 100, 2.0, near=0.5, far=8.5)
    P = cam["proj"]
    want = np.zeros(16, np.float32)
    want[0], want[5], want[10], want[14], want[15] = 1 / (2.0 * 2.0), 1 / 2.0, 1 / 8.0, -0.5 / 8.0, 1.0
    assert P.dtype == np.float32 and np.array_equal(P, want)
    assert np.array_equal(cam["view"], np.eye(4, dtype=np.float32).reshape(-1))
    assert cam["near"] == 0.5 and cam["far"] == 8.5 and P[11] == 0
