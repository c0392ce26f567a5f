"""gsm_global_transform without a GPU: the host helper gsm_global_transform_from_pose against a float64
derivation that shares no method with it, the convention of the whole transform against the float64 model's pose
branch (f64_model.project(..., scene_transform=M, pose=True)), and the numpy restatement on hand-made cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import extract_ref  # noqa: E402
import f64_model  # noqa: E402
import transform_ref as ref  # noqa: E402

F = np.float32
CSRC = os.path.join(ROOT, "gsm-renderer_amd", "csrc")
CHECK_SRC = os.path.join(HERE, "host", "transform_check_test.cpp")
ALL_KEEP = [0xFFFFFFFF] * 8
ERR_ARG = 14
EPS = 2.0 ** -23
SIZES = dict(matrix=12, quaternion=4, scale=1, sh1=9, sh2=25, sh3=49)


def axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def quarter(axis, turns):
    """an exact rotation by turns quarter turns about a coordinate axis: entries 0 and +-1"""
    return np.round(axis_angle(np.eye(3)[axis], turns * np.pi / 2))


def rotations():
    from test_select_where import ROT
    rng = np.random.default_rng(33)
    rs = {"identity": np.eye(3)}
    for k, name in enumerate("xyz"):
        rs["quarter turn about " + name] = quarter(k, 1)
    for k, name in enumerate("xyz"):
        rs["half turn about " + name] = quarter(k, 2)
    rs["ROT of test_select_where"] = np.asarray(ROT, np.float64)
    for i in range(4):
        q = rng.normal(size=4)
        rs["random %d" % i] = f64_model.rotation_from_quaternion(q[None])[0]
    # the helper takes floats: what it and the derivation see is the float32 value
    return {k: v.astype(F).astype(np.float64) for k, v in rs.items()}


GENERAL = axis_angle((0.3, -0.8, 0.5), 0.6).astype(F).astype(np.float64)


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    """the stand-alone program over the helper's header, built twice: plain, and with the address and
    undefined-behaviour sanitizers linked statically (no device, no Python in its process)"""
    d = tmp_path_factory.mktemp("transform_check")
    cxx = os.environ.get("CXX", "g++")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I" + CSRC]
    subprocess.run(base + ["-o", str(d / "plain"), CHECK_SRC], check=True)
    subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", str(d / "san"), CHECK_SRC], check=True)
    return d


def run_poses(exe, poses):
    """[(status, descriptor dict)] of poses [(R, s, t)] from the program"""
    text = "\n".join(" ".join(repr(float(v)) for v in list(np.asarray(R).reshape(9)) + [s] + list(t))
                     for R, s, t in poses)
    r = subprocess.run([str(exe), "poses"], input=text + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.strip().split("\n"):
        v = line.split()
        f = np.array([float(x) for x in v[1:]], np.float64).astype(F)
        assert len(f) == 100
        d, at = {}, 0
        for k in ref.NAMES:
            d[k] = f[at:at + SIZES[k]]
            at += SIZES[k]
        d["scale"] = F(d["scale"][0])
        out.append((int(v[0]), d))
    assert len(out) == len(poses)
    return out


def helper_desc(helper, R, s, t):
    (st, d), = run_poses(helper / "plain", [(R, s, t)])
    assert st == 0
    return d


# ---- 1. the helper ----
def test_refusal_rows_of_the_helper_and_the_entry(helper):
    """tests/host/transform_check_test.cpp with no argument: every refusal row of gsm_global_transform_from_pose,
    every row of gsm_global_transform's table in both precisions and their order, the exact identity -- once plain and
    once under the sanitizers."""
    for exe in ("plain", "san"):
        r = subprocess.run([str(helper / exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        assert "all checks passed" in r.stdout


def test_helper_against_the_float64_derivation(helper):
    """Every output for a dozen rotations against desc_f64, under both builds.  Entries of the quaternion and of D
    are at most 1 in magnitude, so a correct single rounding is within 2^-25; the bound of 2^-23 leaves a factor 4
    for the fit's own error.  The matrix is held to 2^-23 relative.  At a half turn w is 0 and q and -q are the same
    rotation: there the quaternion is compared up to that sign."""
    rs = rotations()
    assert len(rs) == 12
    s, t = 1.75, (0.5, -2.0, 3.25)
    poses = [(R, s, t) for R in rs.values()]
    plain = run_poses(helper / "plain", poses)
    san = run_poses(helper / "san", poses)
    worst = {}
    for (name, R), (st, d), (st2, d2) in zip(rs.items(), plain, san):
        assert st == 0 and st2 == 0, name
        want = ref.desc_f64(R, s, t)
        for k in ref.NAMES:
            assert np.array_equal(np.asarray(d[k]), np.asarray(d2[k])), (name, k)
            got = np.asarray(d[k], np.float64).reshape(-1)
            w = np.asarray(want[k], np.float64).reshape(-1)
            if k == "quaternion" and abs(w[3]) < 1e-6:
                w = w if np.abs(got - w).max() <= np.abs(got + w).max() else -w
            if k in ("matrix", "scale"):
                err = np.abs(got - w) / np.where(w == 0, 1.0, np.abs(w))
            else:
                err = np.abs(got - w)
                assert np.abs(got).max() <= 1.0
            worst[k] = max(worst.get(k, 0.0), float(err.max()))
            assert err.max() <= EPS, (name, k, float(err.max()))
        assert d["quaternion"][3] >= 0, name
        assert abs(float(np.linalg.norm(d["quaternion"].astype(np.float64))) - 1.0) <= EPS
    print("worst differences:", {k: "%.3g" % v for k, v in worst.items()})


def test_identity_and_quarter_turns_are_exact(helper):
    """The identity gives identity matrices exactly (so the transform by it changes no bit but a -0 sum), and a
    quarter turn gives matrices of 0 and +-1 up to the solve's rounding: rounded to float32 they are within 2^-23."""
    d = helper_desc(helper, np.eye(3), 1.0, (0, 0, 0))
    assert np.array_equal(d["matrix"].reshape(3, 4), np.eye(3, 4, dtype=F))
    assert d["quaternion"].tolist() == [0, 0, 0, 1] and d["scale"] == 1
    for k, n in (("sh1", 3), ("sh2", 5), ("sh3", 7)):
        assert np.array_equal(d[k].reshape(n, n), np.eye(n, dtype=F)), k
    d = helper_desc(helper, quarter(2, 1), 1.0, (0, 0, 0))
    for k in ("sh1", "sh2", "sh3"):
        assert np.abs(d[k] - np.round(d[k])).max() <= EPS and set(np.round(d[k]).tolist()) <= {-1.0, 0.0, 1.0}


def test_band_matrices_compose(helper):
    """D(R1 R2) = D(R1) D(R2).  The helper sees float32 entries of R1 R2: each is off by at most 2^-25, the nearest
    rotation by an angle of at most 3 * 2^-25 / sqrt(2), and a band-l matrix moves by at most l times that angle
    (its eigenvalues are exp(i m angle), |m| <= l): 6.4 * 2^-25 for band 3.  The product of two rounded 7x7 factors
    adds at most 14 * 2^-25 and the rounding of D(R1 R2) itself 2^-25: below 22 * 2^-25, held to 2^-20."""
    rs = list(rotations().values())
    pairs = [(rs[8], rs[9]), (rs[7], rs[10]), (rs[1], rs[11]), (rs[9], rs[8])]
    polar = lambda R: (lambda U, _, Vt: U @ Vt)(*np.linalg.svd(R))
    prods = [(polar(a) @ polar(b)).astype(F).astype(np.float64) for a, b in pairs]
    zero = (0.0, 0.0, 0.0)
    out = run_poses(helper / "plain", [(R, 1.0, zero) for ab in pairs for R in ab] + [(R, 1.0, zero) for R in prods])
    for i in range(len(pairs)):
        d1, d2, d12 = out[2 * i][1], out[2 * i + 1][1], out[2 * len(pairs) + i][1]
        for k, n in (("sh1", 3), ("sh2", 5), ("sh3", 7)):
            p = d1[k].astype(np.float64).reshape(n, n) @ d2[k].astype(np.float64).reshape(n, n)
            assert np.abs(p - d12[k].astype(np.float64).reshape(n, n)).max() <= 2.0 ** -20, (i, k)
        assert not np.allclose(d1["sh3"].reshape(7, 7) @ d2["sh3"].reshape(7, 7),
                               d2["sh3"].reshape(7, 7) @ d1["sh3"].reshape(7, 7), atol=1e-3), "the order matters"


def test_python_transform_reads_the_helper_back(gsm, helper):
    """gsm_amd.Transform.from_pose is the library's own entry: the same floats as the stand-alone program's, and
    from_matrix takes pose_matrix apart again; a matrix that is no similarity is refused."""
    from gsm_amd import scenes
    t = (0.25, -1.5, 2.0)
    d = helper_desc(helper, GENERAL, 1.0, t)
    T = gsm.Transform.from_pose(GENERAL, 1.0, t)
    for k in ref.NAMES:
        assert np.array_equal(np.asarray(getattr(T, k), F).reshape(-1), np.asarray(d[k], F).reshape(-1)), k
    T2 = gsm.Transform.from_matrix(scenes.pose_matrix(GENERAL, 1.0, t))
    for k in ref.NAMES:
        assert np.array_equal(np.asarray(getattr(T2, k)), np.asarray(getattr(T, k))), k
    T3 = gsm.Transform.from_matrix(scenes.pose_matrix(GENERAL, 2.5, t))
    assert abs(float(T3.scale) - 2.5) <= 2.5 * EPS and np.array_equal(T3.sh3, T.sh3)
    M = scenes.pose_matrix(GENERAL, 1.0, t)
    assert M.shape == (16,) and np.array_equal(M.reshape(4, 4).T[:3, 3], t)
    for bad in (np.diag([1.0, 2.0, 1.0, 1.0]), np.diag([1.0, 1.0, -1.0, 1.0])):
        with pytest.raises((gsm.RendererError, ValueError)):
            gsm.Transform.from_matrix(bad.T.reshape(16))
    shear = np.eye(4)
    shear[0, 1] = 0.1
    with pytest.raises((gsm.RendererError, ValueError)):
        gsm.Transform.from_matrix(shear.T.reshape(16))
    with pytest.raises(gsm.RendererError) as e:
        gsm.Transform.from_pose(GENERAL, 0.0, t)
    assert int(e.value.status) == ERR_ARG


# ---- 2. the convention, against the float64 model's pose branch ----
W, H, NG = 320, 180, 300
CENTRE = np.array([0.0, 0.0, 5.5])

# Measured here on the CPU (this test prints the figures): the largest difference between the model's projection of
# the transformed scene and its pose branch on the untransformed one, over the gaussians visible in both.  The two
# sides differ by the float32 rounding of the transformed fields alone.  Asserted with a margin of 8.
MEASURED = dict(mean=1.57e-5, depth=1.03e-7, conic=2.25e-7, color=3.76e-8, opacity=0.0)
MEASURED_S2 = dict(mean=1.83e-5, conic=4.22e-7)
MARGIN = 8.0


def differences(a, b, both):
    """the largest difference per field over the gaussians `both`: the mean in pixels, the depth relative, the conic
    relative to its largest entry, colour and opacity absolute"""
    out = {}
    out["mean"] = float(np.abs(a["mean"][both] - b["mean"][both]).max())
    out["depth"] = float((np.abs(a["depth"][both] - b["depth"][both]) / np.abs(b["depth"][both])).max())
    out["conic"] = float((np.abs(a["conic"][both] - b["conic"][both]) /
                          np.abs(b["conic"][both]).max(1, keepdims=True)).max())
    out["color"] = float(np.abs(a["color"][both] - b["color"][both]).max())
    out["opacity"] = float(np.abs(a["opacity"][both] - b["opacity"][both]).max())
    return out


def hamilton(p, q):
    """p (x) q for xyzw rows, float64"""
    px, py, pz, pw = (p[..., i] for i in range(4))
    qx, qy, qz, qw = (q[..., i] for i in range(4))
    return np.stack([pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx,
                     pw * qz + px * qy - py * qx + pz * qw, pw * qw - px * qx - py * qy - pz * qz], -1)


def test_transform_agrees_with_the_models_pose_branch(helper):
    """project(apply(scene)) against project(scene, scene_transform=M, pose=True) in mean, conic, depth, colour and
    opacity, at s = 1; each wrong convention -- D transposed, q (x) a for a (x) q, R^T in the matrix -- misses the
    bound by a factor of 100 or more in the field it concerns; then s = 2 on the conic and the mean."""
    from gsm_amd import scenes
    world, harm, cam = scenes.gen_scene(NG, W, H, 16, 0, seed=5)
    t = CENTRE - GENERAL @ CENTRE + np.array([0.2, -0.1, 0.3])   # a turn about the scene's centre, and a step
    t = t.astype(F).astype(np.float64)
    M = scenes.pose_matrix(GENERAL, 1.0, t)
    d = helper_desc(helper, GENERAL, 1.0, t)
    want = f64_model.project(world, harm, 16, cam, W, H, scene_transform=M, pose=True)

    def against(w2, h2, want=want):
        got = f64_model.project(w2, h2, 16, cam, W, H)
        both = got["visible"] & want["visible"]
        assert both.sum() >= NG // 2 and (got["visible"] == want["visible"]).mean() > 0.98
        return differences(got, want, both)

    w2, h2 = ref.apply(world, harm, 16, 0, 0, ALL_KEEP, d)
    diff = against(w2, h2)
    print("s = 1:", {k: "%.3g" % v for k, v in diff.items()})
    for k, v in diff.items():
        assert v <= MARGIN * MEASURED[k], (k, v)
    # wrong conventions
    wrong = dict(d, sh1=d["sh1"].reshape(3, 3).T.reshape(9).copy(), sh2=d["sh2"].reshape(5, 5).T.reshape(25).copy(),
                 sh3=d["sh3"].reshape(7, 7).T.reshape(49).copy())
    bad = against(*ref.apply(world, harm, 16, 0, 0, ALL_KEEP, wrong))
    print("D transposed:", "%.3g" % bad["color"])
    assert bad["color"] >= 100 * MARGIN * MEASURED["color"]
    w3 = w2.copy()
    w3["rot"] = hamilton(world["rot"].astype(np.float64), d["quaternion"].astype(np.float64)[None]).astype(F)
    bad = against(w3, h2)
    print("q (x) a:", "%.3g" % bad["conic"])
    assert bad["conic"] >= 100 * MARGIN * MEASURED["conic"]
    m = d["matrix"].reshape(3, 4).copy()
    m[:, :3] = m[:, :3].T
    got = f64_model.project(*ref.apply(world, harm, 16, 0, 0, ALL_KEEP, dict(d, matrix=m.reshape(12))), 16, cam, W, H)
    both = got["visible"] & want["visible"]
    bad = differences(got, want, both)
    print("R^T in the matrix:", "%.3g" % bad["mean"], "%.3g" % bad["depth"])
    assert bad["mean"] >= 100 * MARGIN * MEASURED["mean"] and bad["depth"] >= 100 * MARGIN * MEASURED["depth"]
    # s = 2: the scene twice as large about the camera, then the same step (it stays in view)
    t2 = np.array([0.2, -0.1, 0.3]).astype(F).astype(np.float64)
    R2 = axis_angle((0.3, -0.8, 0.5), 0.15).astype(F).astype(np.float64)
    M2 = scenes.pose_matrix(R2, 2.0, t2)
    d2 = helper_desc(helper, R2, 2.0, t2)
    want2 = f64_model.project(world, harm, 16, cam, W, H, scene_transform=M2, pose=True)
    got2 = f64_model.project(*ref.apply(world, harm, 16, 0, 0, ALL_KEEP, d2), 16, cam, W, H)
    alike = (got2["margins"]["scale"] > 0) == (want2["margins"]["scale"] > 0)
    both = got2["visible"] & want2["visible"] & alike
    assert both.sum() >= NG // 2
    diff2 = differences(got2, want2, both)
    print("s = 2:", {k: "%.3g" % diff2[k] for k in MEASURED_S2})
    for k in MEASURED_S2:
        assert diff2[k] <= MARGIN * MEASURED_S2[k], (k, diff2[k])


# ---- 3. hand-made cases of apply ----
@pytest.mark.parametrize("prec", [0, 1])
def test_apply_on_hand_made_cases(helper, prec):
    from gsm_amd import scenes
    n, sh = 6, 16
    world, harm, _ = scenes.gen_scene(n, 64, 64, sh, prec, seed=2)
    d = helper_desc(helper, GENERAL, 1.5, (1.0, 2.0, 3.0))
    state = np.array([0, 1, 0, 1, 1, 0], np.uint8)
    keep = extract_ref.keep_masked(1, 1)
    w2, h2 = ref.apply(world, harm, sh, prec, state, keep, d)
    rows, rows2 = np.asarray(harm).reshape(n, 3, sh), np.asarray(h2).reshape(n, 3, sh)
    out = state == 0
    # a gaussian out of the keep set keeps its bytes; the inputs are not written
    assert world[out].tobytes() == w2[out].tobytes() and rows[out].tobytes() == rows2[out].tobytes()
    assert all(world[i].tobytes() != w2[i].tobytes() and rows[i].tobytes() != rows2[i].tobytes()
               for i in np.nonzero(~out)[0])
    # band 0, the opacity and the pad words keep their bytes
    assert rows[:, :, 0].tobytes() == rows2[:, :, 0].tobytes()
    for k in ("opacity", "pad0") + (("pad1",) if prec else ()):
        assert world[k].tobytes() == w2[k].tobytes(), k
    # the position and the scales of one gaussian by hand
    m = d["matrix"].reshape(3, 4)
    p = np.array([world["px"][1], world["py"][1], world["pz"][1]], F)
    for r, k in enumerate(("px", "py", "pz")):
        assert w2[k][1] == F(F(F(F(m[r, 0] * p[0]) + F(m[r, 1] * p[1])) + F(m[r, 2] * p[2])) + m[r, 3])
    if prec:
        assert w2["sx"][1] == np.float16(F(np.uint16(world["sx"][1]).view(np.float16)) * F(1.5)).view(np.uint16)
    else:
        assert w2["sx"][1] == F(world["sx"][1] * F(1.5))
    # the whole scene by {NULL, default}: an int state
    w3, h3 = ref.apply(world, harm, sh, prec, 7, ALL_KEEP, d)
    assert w3[~out].tobytes() == w2[~out].tobytes() and all(world[i].tobytes() != w3[i].tobytes() for i in range(n))
    w4, _ = ref.apply(world, harm, sh, prec, 7, extract_ref.keep_masked(0xFF, 8), d)
    assert w4.tobytes() == world.tobytes()
    # sh_components 0 and 1 never read the harmonics: anything goes back as it came
    for k in (0, 1):
        sentinel = object()
        w5, h5 = ref.apply(world, sentinel, k, prec, 7, ALL_KEEP, d)
        assert h5 is sentinel and w5.tobytes() == w3.tobytes()
    # 4 and 9 components rotate bands 1 and 1-2 with the same matrices: the rows' leading coefficients agree with 16's
    for k in (4, 9):
        hk = np.ascontiguousarray(rows[:, :, :k]).reshape(-1)
        _, hk2 = ref.apply(world, hk, k, prec, 7, ALL_KEEP, d)
        assert np.asarray(hk2).reshape(n, 3, k).tobytes() == np.ascontiguousarray(
            np.asarray(h3).reshape(n, 3, sh)[:, :, :k]).tobytes()
