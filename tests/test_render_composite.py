"""gsm_global_render_composite: several posed scenes sorted and blended together into one Global
frame.  The contract: the frame is the Global frame of the concatenated objects, each projected under its own
camera.  The yardsticks are `render` of the concatenated buffers on a second handle (objects under one camera),
the oracle's frame of that concatenation, and the checker tests/compose/compose_ref.c (objects under different
cameras) -- never the composite itself.  Every target is pre-filled with a sentinel byte and followed by sentinel
rows that must keep it; all comparisons are of bytes.  Shapes are the smallest that reach each code path."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

ERR_COUNT, ERR_DIMS, ERR_SIZE, ERR_MISSING, ERR_ARG, ERR_UNSUPPORTED = 6, 7, 8, 13, 14, 15
FILL, GAP = 0xA5, 3  # the sentinel byte, and the sentinel rows after every target


# ---- helpers ----
def to_dev(torch, arr):
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def roundup256(n):
    return (n + 255) // 256 * 256


def diff(a, b):
    idx = np.nonzero(np.asarray(a).reshape(-1) != np.asarray(b).reshape(-1))[0]
    return f"{idx.size} bytes differ, first at {idx[:4].tolist()}"


class Scene:
    """A scene on the host and (with a torch module) on the device."""

    def __init__(self, torch, world, harm, sh):
        self.world_np, self.harm_np, self.sh = world, np.asarray(harm).reshape(-1), sh
        self.n = len(world)
        self.prec = 1 if world.dtype.itemsize == 32 else 0
        if torch is not None and self.n:
            self.world, self.harm = to_dev(torch, world), to_dev(torch, self.harm_np)
        else:
            self.world = self.harm = None

    def input(self, gsm):
        return gsm.GaussianInput(self.world, self.harm, self.n, self.sh)


def gen(torch, n, w, h, sh, prec, seed, **kw):
    from gsm_amd import scenes
    world, harm, _ = scenes.gen_scene(n, w, h, sh, prec, seed=seed, **kw)
    return Scene(torch, world, harm, sh)


def concat(torch, scs):
    return Scene(torch, np.concatenate([s.world_np for s in scs]), np.concatenate([s.harm_np for s in scs]),
                 scs[0].sh)


def items_of(scs):
    return max(sum(roundup256(s.n) for s in scs), 1)


def handle(gsm, max_gaussians, mw, mh, prec, fmt=0, color_space=0):
    return gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=max_gaussians, max_width=mw, max_height=mh,
                                                        precision=prec, color_format=fmt,
                                                        gaussian_color_space=color_space))


def target(torch, w, h, bpp=8):
    color = torch.full((h + GAP, w * bpp), FILL, dtype=torch.uint8, device="cuda")
    depth = torch.full((h + GAP, w * 2), FILL, dtype=torch.uint8, device="cuda")
    return color, depth


def readback(torch, color, depth, h):
    torch.cuda.synchronize()
    c, d = color.cpu().numpy(), depth.cpu().numpy()
    assert (c[h:] == FILL).all() and (d[h:] == FILL).all(), "sentinel rows were written"
    return c[:h], d[:h]


def objects_of(gsm, pairs):
    return [gsm.SceneObject(sc.input(gsm), gsm.CameraParams.from_dict(cam)) for sc, cam in pairs]


def composite(gsm, torch, r, pairs, w, h, bpp=8, depth=True):
    """One render_composite of [(scene, camera dict)] into fresh sentinel targets: (colour rows, depth rows)."""
    color, dep = target(torch, w, h, bpp)
    r.render_composite(color, dep if depth else None, objects_of(gsm, pairs), w, h)
    return readback(torch, color, dep, h)


def object_array(gsm, objs):
    """The gsm_global_object array of a SceneObject list, as the C entry takes it."""
    arr = (gsm._GlobalObject * max(len(objs), 1))()
    for g, o in zip(arr, objs):
        g.input = gsm._Input(gsm._ptr(o.input.gaussians), gsm._ptr(o.input.harmonics), int(o.input.gaussian_count),
                             int(o.input.sh_components))
        g.camera = gsm._camera_struct(o.camera)
    return arr


def raw_composite(gsm, r, arr, count, w, h, color, depth, bpp=8):
    """The bound C entry itself, with any array and object_count: its status."""
    return int(gsm._lib().gsm_global_render_composite(r._h, gsm._stream_handle(None), arr, count, w, h,
                                                      gsm._ptr(color), w * bpp, gsm._ptr(depth), w * 2))


def single(gsm, torch, r, sc, cam, w, h, bpp=8):
    color, dep = target(torch, w, h, bpp)
    r.render(color, dep, sc.input(gsm), gsm.CameraParams.from_dict(cam), w, h)
    return readback(torch, color, dep, h)


def frame_bytes(ref, h):
    return ref["color"].view(np.uint8).reshape(h, -1), ref["depth"].view(np.uint8).reshape(h, -1)


def checker_frame(pairs, w, h, max_gaussians, mw=None, mh=None, color_space=0):
    import compose_ref
    ref = compose_ref.render([(s.world_np, s.harm_np, cam) for s, cam in pairs], pairs[0][0].sh, w, h,
                             max_gaussians=max_gaussians, max_width=mw, max_height=mh, color_space=color_space)
    assert ref["status"] == 0
    return ref


def clear_bytes(h, w):
    """the clear value: colour (0, 0, 0, 1) in fp16, depth 0"""
    c = np.zeros((h, w, 4), np.uint16)
    c[..., 3] = 0x3C00
    return c.view(np.uint8).reshape(h, -1), np.zeros((h, w * 2), np.uint8)


def model(angle_deg, axis, t, s, pivot=(0.0, 0.0, 5.5)):
    """A similarity transform, 4x4 column-major flat: a rotation about `axis` through `pivot`, a uniform scale
    about the pivot, then a translation."""
    a = np.radians(angle_deg)
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    p = np.asarray(pivot, np.float64)
    M = np.eye(4)
    M[:3, :3] = s * R
    M[:3, 3] = p - s * R @ p + np.asarray(t, np.float64)
    return M.T.reshape(-1)


POSES = [model(9.0, (0, 1, 0), (0.3, -0.2, 0.4), 0.9), model(-14.0, (1, 1, 0), (-0.4, 0.1, -0.3), 1.15),
         model(21.0, (0, 0, 1), (0.1, 0.3, 0.2), 1.0), model(-6.0, (1, 0, 1), (-0.2, -0.3, 0.6), 0.8)]


def posed(scs, w, h):
    from gsm_amd import scenes
    cam = scenes.make_camera(w, h)
    return [(s, scenes.object_camera(cam, POSES[i % len(POSES)])) for i, s in enumerate(scs)]


def check_shared_camera(gsm, torch, oracle, scs, cam, w, h, mw=None, mh=None, with_oracle=True):
    """The composite of `scs` under one camera equals `render` of their concatenation on a second handle of the
    same size, and the oracle's frame of that concatenation; the assignment totals are equal."""
    mw, mh = mw or w, mh or h
    M, prec = items_of(scs), scs[0].prec
    rc = handle(gsm, M, mw, mh, prec)
    gc, gd = composite(gsm, torch, rc, [(s, cam) for s in scs], w, h)
    total = rc.debug_read_total_assignments()
    assert rc.counters()["overflow"] == 0
    assert rc.counters()["gaussian_count"] == sum(s.n for s in scs)
    rc.close()
    cat = concat(torch, scs)
    rs = handle(gsm, M, mw, mh, prec)
    sc_, sd_ = single(gsm, torch, rs, cat, cam, w, h)
    assert rs.counters()["overflow"] == 0, "the yardstick frame overflowed: no parity to check"
    assert total == rs.debug_read_total_assignments()
    rs.close()
    assert np.array_equal(gc, sc_), "colour vs render of the concatenation: " + diff(gc, sc_)
    assert np.array_equal(gd, sd_), "depth vs render of the concatenation: " + diff(gd, sd_)
    if with_oracle:
        ref = oracle.render(cat.world_np, cat.harm_np, cat.sh, cam, w, h, max_gaussians=M, max_width=mw,
                            max_height=mh)
        oc, od = frame_bytes(ref, h)
        assert np.array_equal(gc, oc), "colour vs oracle: " + diff(gc, oc)
        assert np.array_equal(gd, od), "depth vs oracle: " + diff(gd, od)
        assert total == ref["total_assignments"]
    return gc, gd, total


def check_against_checker(gsm, torch, pairs, w, h, kind=None, fmt=0, convert=None):
    """The composite of [(scene, its own camera)] equals the checker's frame: colour, depth, assignment total."""
    scs = [s for s, _ in pairs]
    M = items_of(scs)
    bpp = 8 if fmt == 0 else 4
    rc = handle(gsm, M, w, h, scs[0].prec, fmt=fmt)
    gc, gd = composite(gsm, torch, rc, pairs, w, h, bpp=bpp)
    total = rc.debug_read_total_assignments()
    assert rc.counters()["overflow"] == 0
    if kind is not None:
        assert rc.blend_kernel_kind() == kind
    rc.close()
    ref = checker_frame(pairs, w, h, M)
    oc, od = frame_bytes(ref, h)
    if convert is not None:
        oc = convert(ref["color"]).reshape(h, -1)
    assert total == ref["total_assignments"] and total > 0
    assert np.array_equal(gc, oc), "colour vs checker: " + diff(gc, oc)
    assert np.array_equal(gd, od), "depth vs checker: " + diff(gd, od)
    return ref


# ---- 1. declaration, export, binding and layout (no GPU) ----
def test_composite_entry_is_declared_exported_bound_and_laid_out(gsm):
    from gsm_amd import scenes
    src = open(os.path.join(ROOT, "include", "gsm_renderer.h")).read()
    assert re.search(r"gsm_status\s+gsm_global_render_composite\s*\(", src)
    assert re.search(r"\}\s*gsm_global_object\s*;", src)
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    assert gsm.abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    assert " T gsm_global_render_composite" in out
    assert "gsm_global_render_composite" in gsm._SIGNATURES
    assert callable(getattr(gsm.GlobalRenderer, "render_composite", None))
    assert {"input", "camera"} <= set(gsm.SceneObject.__dataclass_fields__)
    assert callable(getattr(scenes, "object_camera", None))
    m = re.search(r"static_assert\s*\(\s*sizeof\s*\(\s*gsm_global_object\s*\)\s*==\s*(\d+)", src)
    assert m, "the header pins sizeof(gsm_global_object)"
    assert C.sizeof(gsm._GlobalObject) == int(m.group(1))


# ---- 2. the checker against the oracle (no GPU) ----
def _same_frame(a, b):
    for k in ("color", "depth", "sorted_keys", "sorted_values", "keys", "values", "bounds", "tile_counts"):
        assert np.array_equal(a[k], b[k]), k
    assert a["total_assignments"] == b["total_assignments"] and a["overflow"] == b["overflow"]


@pytest.mark.parametrize("prec", [0, 1])
def test_checker_with_one_object_is_the_oracle(oracle, prec):
    from gsm_amd import scenes
    w, h = 97, 45
    sc = gen(None, 3000, w, h, 4, prec, 51)
    cam = scenes.orbit_camera(w, h, 7.0)
    ref = oracle.render(sc.world_np, sc.harm_np, 4, cam, w, h)
    got = checker_frame([(sc, cam)], w, h, sc.n)
    assert ref["total_assignments"] > 0
    _same_frame(got, ref)


@pytest.mark.parametrize("prec", [0, 1])
def test_checker_with_three_objects_under_one_camera_is_the_oracle_of_the_concatenation(oracle, prec):
    from gsm_amd import scenes
    w, h = 97, 45
    scs = [gen(None, n, w, h, 4, prec, 52 + i) for i, n in enumerate((1, 257, 5000))]
    cam = scenes.make_camera(w, h)
    cat = concat(None, scs)
    ref = oracle.render(cat.world_np, cat.harm_np, 4, cam, w, h)
    got = checker_frame([(s, cam) for s in scs], w, h, cat.n)
    assert got["first"] == [0, 1, 258] and ref["total_assignments"] > 0
    _same_frame(got, ref)


# ---- 3. object_camera (no GPU) ----
def test_object_camera_of_the_identity_is_the_camera(gsm):
    from gsm_amd import scenes
    cam = scenes.orbit_camera(97, 45, 11.0)
    got = scenes.object_camera(cam, np.eye(4).reshape(-1))
    for k in ("view", "proj", "position"):
        assert got[k].dtype == np.float32
        assert got[k].tobytes() == np.asarray(cam[k], np.float32).tobytes(), k
    for k in ("focal_x", "focal_y", "near", "far"):
        assert got[k] == cam[k]


def test_object_camera_of_a_similarity_matches_a_float64_restatement(gsm):
    """view * M by explicit float64 sums, M^-1 * position as R^T (position - t) / s.  Both sides are float64
    results rounded once to float32: the words are equal.  (A float32 product, a second rounding or a float32
    inverse differs from these in the last bits of some word.)"""
    from gsm_amd import scenes
    cam = scenes.orbit_camera(97, 45, -17.0)
    a, s, t = np.radians(33.0), 1.7, np.array([0.4, -1.1, 2.3])
    k = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    got = scenes.object_camera(cam, M.T.reshape(-1))
    V = np.asarray(cam["view"], np.float64).reshape(4, 4).T
    want_v = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            want_v[i, j] = sum(V[i, m] * M[m, j] for m in range(4))
    want_v = want_v.T.reshape(-1).astype(np.float32)
    want_p = (R.T @ (np.asarray(cam["position"], np.float64) - t) / s).astype(np.float32)
    assert got["view"].dtype == np.float32 and got["position"].dtype == np.float32
    assert got["view"].tobytes() == want_v.tobytes(), (got["view"], want_v)
    assert got["position"].tobytes() == want_p.tobytes(), (got["position"], want_p)
    assert got["proj"].tobytes() == np.asarray(cam["proj"], np.float32).tobytes()
    assert got["near"] == cam["near"] and got["far"] == cam["far"]


# ---- 4. shared camera: the composite is the frame of the concatenation ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("size", [(97, 45), (640, 360)])
def test_shared_camera_is_the_frame_of_the_concatenation(gsm, cuda, oracle, prec, size):
    """Counts 1, 257 and 5000: item bases 0, 256 and 768.  On a captured frame the sorted values, mapped from
    item to (object, id), are the oracle's."""
    from gsm_amd import scenes
    w, h = size
    counts = (1, 257, 5000)
    scs = [gen(cuda, n, w, h, 4, prec, 60 + i) for i, n in enumerate(counts)]
    cam = scenes.make_camera(w, h)
    _, _, total = check_shared_camera(gsm, cuda, oracle, scs, cam, w, h)
    assert total > 0
    # the captured frame: items -> concatenated ids
    M = items_of(scs)
    rc = handle(gsm, M, w, h, prec)
    rc.set_profiling(stage_events=False, capture=True)
    composite(gsm, cuda, rc, [(s, cam) for s in scs], w, h)
    vals = rc.copy_buffer(gsm.BufferId.SORTED_VALUES).astype(np.int64)
    keys = rc.copy_buffer(gsm.BufferId.SORTED_KEYS)
    rc.close()
    base = np.cumsum([0] + [roundup256(n) for n in counts])   # first item of every object
    first = np.cumsum([0] + list(counts))                     # first concatenated id
    obj = np.searchsorted(base[1:], vals, side="right")
    local = vals - base[obj]
    assert (local < np.asarray(counts)[obj]).all(), "a value names an item past its object's count"
    cat = concat(None, scs)
    ref = oracle.render(cat.world_np, cat.harm_np, 4, cam, w, h, max_gaussians=M)
    assert np.array_equal(keys, ref["sorted_keys"])
    assert np.array_equal(first[obj] + local, ref["sorted_values"].astype(np.int64))


# ---- 5. distinct poses ----
@pytest.mark.gpu
def test_distinct_poses_match_the_checker_and_each_object_its_own_render(gsm, cuda):
    w, h = 640, 360
    counts = (300, 257, 2000)
    scs = [gen(cuda, n, w, h, 4, 1, 70 + i) for i, n in enumerate(counts)]
    pairs = posed(scs, w, h)
    assert len({p[1]["view"].tobytes() for p in pairs}) == 3
    check_against_checker(gsm, cuda, pairs, w, h)
    M = items_of(scs)
    rc = handle(gsm, M, w, h, 1)
    rc.set_profiling(stage_events=False, capture=True)
    composite(gsm, cuda, rc, pairs, w, h)
    rd = rc.copy_buffer(gsm.BufferId.RENDER_DATA)
    bounds = rc.copy_buffer(gsm.BufferId.BOUNDS)
    rc.close()
    assert len(rd) == M and len(bounds) == M, "item-indexed arrays"
    at = 0
    for o, (sc, cam) in enumerate(pairs):
        rs = handle(gsm, M, w, h, 1)
        rs.set_profiling(stage_events=False, capture=True)
        single(gsm, cuda, rs, sc, cam, w, h)
        srd, sb = rs.copy_buffer(gsm.BufferId.RENDER_DATA), rs.copy_buffer(gsm.BufferId.BOUNDS)
        rs.close()
        assert np.array_equal(bounds[at:at + sc.n], sb[:sc.n]), f"object {o} bounds"
        # (render data: a culled gaussian's entry is unspecified after either call, include/gsm_renderer.h)
        vis = (sb[:sc.n, 0] <= sb[:sc.n, 1]) & (sb[:sc.n, 2] <= sb[:sc.n, 3])
        assert vis.any()
        assert rd[at:at + sc.n][vis].tobytes() == srd[:sc.n][vis].tobytes(), f"object {o} render data"
        at += roundup256(sc.n)


# ---- 6. tie order ----
@pytest.mark.gpu
def test_ties_keep_object_then_gaussian_order(gsm, cuda, oracle):
    """The same scene twice under one camera: every key ties across the two objects.  [A, B] and [B, A] each
    equal their own concatenation."""
    from gsm_amd import scenes
    w, h = 97, 45
    A, B = gen(cuda, 700, w, h, 1, 0, 80), gen(cuda, 300, w, h, 1, 0, 81)
    cam = scenes.make_camera(w, h)
    check_shared_camera(gsm, cuda, oracle, [A, A], cam, w, h)
    ab, _, _ = check_shared_camera(gsm, cuda, oracle, [A, B], cam, w, h)
    ba, _, _ = check_shared_camera(gsm, cuda, oracle, [B, A], cam, w, h)
    assert ab.shape == ba.shape


# ---- 7. edges ----
@pytest.mark.gpu
def test_single_object_is_render_byte_for_byte(gsm, cuda, oracle):
    from gsm_amd import scenes
    w, h = 97, 45
    check_shared_camera(gsm, cuda, oracle, [gen(cuda, 1000, w, h, 4, 1, 82)], scenes.orbit_camera(w, h, 5.0), w, h)


@pytest.mark.gpu
def test_empty_object_between_two_others(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    A, B = gen(cuda, 300, w, h, 1, 0, 83), gen(cuda, 500, w, h, 1, 0, 84)
    E = Scene(cuda, A.world_np[:0].copy(), A.harm_np[:0].copy(), 1)
    cam = scenes.make_camera(w, h)
    M = items_of([A, B])
    rc = handle(gsm, M, w, h, 0)
    gc, gd = composite(gsm, cuda, rc, [(A, cam), (E, cam), (B, cam)], w, h)
    assert rc.counters()["gaussian_count"] == 800
    rc.close()
    rs = handle(gsm, M, w, h, 0)
    sc_, sd_ = single(gsm, cuda, rs, concat(cuda, [A, B]), cam, w, h)
    rs.close()
    assert np.array_equal(gc, sc_) and np.array_equal(gd, sd_)


@pytest.mark.gpu
def test_object_wholly_behind_its_camera(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    A, B = gen(cuda, 300, w, h, 1, 0, 85), gen(cuda, 500, w, h, 1, 0, 86)
    cam = scenes.make_camera(w, h)
    away = dict(cam)
    V = np.eye(4, dtype=np.float32)
    V[0, 0] = V[2, 2] = -1.0  # half a turn about the y axis: every gaussian of B is behind it
    away["view"] = V.T.reshape(-1).astype(np.float32)
    M = items_of([A, B])
    rc = handle(gsm, M, w, h, 0)
    gc, gd = composite(gsm, cuda, rc, [(A, cam), (B, away)], w, h)
    total = rc.debug_read_total_assignments()
    rc.close()
    rs = handle(gsm, M, w, h, 0)
    sc_, sd_ = single(gsm, cuda, rs, A, cam, w, h)
    assert total == rs.debug_read_total_assignments() and total > 0
    rs.close()
    assert np.array_equal(gc, sc_) and np.array_equal(gd, sd_)


@pytest.mark.gpu
def test_every_count_zero_is_the_clear_value(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    A = gen(None, 4, w, h, 1, 0, 87)
    E = Scene(cuda, A.world_np[:0].copy(), A.harm_np[:0].copy(), 1)
    cam = scenes.make_camera(w, h)
    rc = handle(gsm, 256, w, h, 0)
    gc, gd = composite(gsm, cuda, rc, [(E, cam), (E, cam)], w, h)
    assert rc.debug_read_total_assignments() == 0 and rc.counters()["gaussian_count"] == 0
    rc.close()
    cc, cd = clear_bytes(h, w)
    assert np.array_equal(gc, cc) and np.array_equal(gd, cd)


@pytest.mark.gpu
def test_depth_null(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    scs = [gen(cuda, 300, w, h, 1, 0, 88), gen(cuda, 500, w, h, 1, 0, 89)]
    cam = scenes.make_camera(w, h)
    M = items_of(scs)
    rc = handle(gsm, M, w, h, 0)
    gc, gd = composite(gsm, cuda, rc, [(s, cam) for s in scs], w, h, depth=False)
    rc.close()
    rs = handle(gsm, M, w, h, 0)
    sc_, _ = single(gsm, cuda, rs, concat(cuda, scs), cam, w, h)
    rs.close()
    assert np.array_equal(gc, sc_)
    assert (gd == FILL).all(), "no depth target was passed"


@pytest.mark.gpu
def test_ragged_frame_smaller_than_the_handle(gsm, cuda, oracle):
    from gsm_amd import scenes
    w, h = 33, 17
    scs = [gen(cuda, 200, w, h, 1, 0, 90), gen(cuda, 300, w, h, 1, 0, 91)]
    check_shared_camera(gsm, cuda, oracle, scs, scenes.make_camera(w, h), w, h, mw=97, mh=45)


@pytest.mark.gpu
def test_screen_covering_gaussian_in_the_last_object(gsm, cuda, oracle):
    """Its rect is over 32 tiles: the scatter's own thread repeats the tile tests for it."""
    from gsm_amd import scenes
    w, h = 640, 360
    A = gen(cuda, 600, w, h, 1, 0, 92)
    big = gen(None, 1, w, h, 1, 0, 93).world_np.copy()
    big["px"], big["py"], big["pz"] = 0.0, 0.0, 4.0
    big["sx"] = big["sy"] = big["sz"] = 1.5
    big["opacity"] = 0.9
    B = Scene(cuda, big, np.full(3, 0.4, np.float32), 1)
    cam = scenes.make_camera(w, h)
    ref = oracle.render(B.world_np, B.harm_np, 1, cam, w, h)
    assert ref["tile_counts"][0] > 32, "the test's premise: a rect the masks do not hold"
    check_shared_camera(gsm, cuda, oracle, [A, B], cam, w, h)


# ---- 8. blend kinds ----
@pytest.mark.gpu
@pytest.mark.parametrize("size,kind", [((640, 360), 1), ((1920, 1080), 2), ((3840, 2160), 3)])
def test_blend_kinds_with_distinct_poses(gsm, cuda, size, kind):
    """20 000 gaussians in 4 objects: quadrant units, half-tile units and the pair walk, named by
    blend_kernel_kind() and checked against the checker."""
    w, h = size
    scs = [gen(cuda, n, w, h, 1, 1, 100 + i) for i, n in enumerate((5000, 4999, 5001, 5000))]
    check_against_checker(gsm, cuda, posed(scs, w, h), w, h, kind=kind)


# ---- 9. one 8-bit format ----
@pytest.mark.gpu
def test_bgra8_unorm_srgb(gsm, cuda, oracle):
    w, h = 97, 45
    scs = [gen(cuda, n, w, h, 4, 1, 110 + i) for i, n in enumerate((300, 700))]
    check_against_checker(gsm, cuda, posed(scs, w, h), w, h, fmt=5,
                          convert=lambda c: oracle.convert_color(c, 5))


# ---- 10. the handle's other entries are undisturbed ----
@pytest.mark.gpu
def test_other_entries_of_the_handle_are_undisturbed(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    A, B = gen(cuda, 2000, w, h, 1, 0, 120), gen(cuda, 1000, w, h, 1, 0, 121)
    cams = [scenes.orbit_camera(w, h, a) for a in (0.0, 8.0)]
    pairs = posed([A, B], w, h)
    M = 2 * roundup256(A.n)

    def mk():
        return handle(gsm, M, w, 2 * h, 0)  # (tile space for two views)

    def views(r):
        color = cuda.full((2, h, w * 8), FILL, dtype=cuda.uint8, device="cuda")
        depth = cuda.full((2, h, w * 2), FILL, dtype=cuda.uint8, device="cuda")
        r.render_views(color, depth, A.input(gsm), [gsm.CameraParams.from_dict(c) for c in cams], w, h)
        cuda.cuda.synchronize()
        return color.cpu().numpy(), depth.cpu().numpy()

    def batch(r):
        tg = [target(cuda, w, h) for _ in range(2)]
        r.render_batch([gsm.BatchView(s.input(gsm), gsm.CameraParams.from_dict(c), w, h, t[0], t[1])
                        for s, c, t in zip((A, B), cams, tg)])
        return [readback(cuda, t[0], t[1], h) for t in tg]

    fresh = {}
    for name, fn in (("render", lambda r: single(gsm, cuda, r, A, cams[1], w, h)), ("views", views),
                     ("batch", batch), ("composite", lambda r: composite(gsm, cuda, r, pairs, w, h))):
        r = mk()
        fresh[name] = fn(r)
        r.close()
    ref = checker_frame(pairs, w, h, M, mh=2 * h)
    assert np.array_equal(fresh["composite"][0], frame_bytes(ref, h)[0]), "the yardstick is the checker's frame"

    def same(a, b):
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(a, b)

    r = mk()
    assert same(single(gsm, cuda, r, A, cams[1], w, h), fresh["render"])
    assert same(composite(gsm, cuda, r, pairs, w, h), fresh["composite"])
    assert same(single(gsm, cuda, r, A, cams[1], w, h), fresh["render"]), "render after a composite"
    assert same(views(r), fresh["views"]), "render_views after a composite"
    got = batch(r)
    assert same(got, fresh["batch"]), "render_batch after a composite"
    assert same(composite(gsm, cuda, r, pairs, w, h), fresh["composite"]), "a composite after them"
    r.close()


# ---- 11. the call consumes its array ----
@pytest.mark.gpu
def test_the_call_consumes_its_array(gsm, cuda):
    from gsm_amd import scenes
    w, h = 640, 360
    scs = [gen(cuda, 5000, w, h, 4, 1, 130), gen(cuda, 3000, w, h, 4, 1, 131)]
    pairs = posed(scs, w, h)
    M = items_of(scs)
    rc = handle(gsm, M, w, h, 1)
    color, dep = target(cuda, w, h)
    arr = object_array(gsm, objects_of(gsm, pairs))
    assert raw_composite(gsm, rc, arr, len(pairs), w, h, color, dep) == 0
    C.memset(arr, 0xFF, C.sizeof(arr))  # (before the sync: the frame may still be in flight)
    gc, gd = readback(cuda, color, dep, h)
    rc.close()
    oc, od = frame_bytes(checker_frame(pairs, w, h, M), h)
    assert np.array_equal(gc, oc) and np.array_equal(gd, od)


# ---- 12. errors ----
@pytest.mark.gpu
def test_errors_and_their_order(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45  # 4 x 3 tiles
    A, B = gen(cuda, 300, w, h, 1, 0, 140), gen(cuda, 500, w, h, 1, 0, 141)
    B4 = Scene(cuda, B.world_np, np.zeros(B.n * 12, np.float32), 4)
    cam = gsm.CameraParams.from_dict(scenes.make_camera(w, h))
    r = handle(gsm, 1024, w, h, 0)  # 512 + 512 items
    color, depth = target(cuda, w, h)

    def obj(sc, count=None, gaussians=True, harmonics=True):
        return gsm.SceneObject(gsm.GaussianInput(sc.world if gaussians else None, sc.harm if harmonics else None,
                                                 sc.n if count is None else count, sc.sh), cam)

    def status(objs, width=w, height=h, color_t=color, depth_t=depth, **kw):
        try:
            r.render_composite(color_t, depth_t, objs, width, height, **kw)
        except gsm.RendererError as e:
            return int(e.status)
        return 0

    ok = [obj(A), obj(B)]
    # counts
    assert raw_composite(gsm, r, object_array(gsm, ok), 0, w, h, color, depth) == ERR_COUNT
    assert raw_composite(gsm, r, object_array(gsm, ok), 65536, w, h, color, depth) == ERR_COUNT
    assert status([obj(A), obj(B, count=1025)]) == ERR_COUNT            # a count over max_gaussians
    assert status([obj(A), obj(B), obj(A, count=1)]) == ERR_COUNT       # 512 + 512 + 256 items > 1024
    # dimensions
    assert status(ok, width=0) == ERR_DIMS and status(ok, height=0) == ERR_DIMS
    assert status(ok, width=w + 1) == ERR_DIMS and status(ok, height=h + 1) == ERR_DIMS
    # missing buffers
    assert status(None) == ERR_MISSING
    assert raw_composite(gsm, r, None, 70000, 0, h, color, depth) == ERR_MISSING  # first of all
    assert status(ok, color_t=None) == ERR_MISSING
    assert status([obj(A), obj(B, gaussians=False)]) == ERR_MISSING
    assert status([obj(A, harmonics=False), obj(B)]) == ERR_MISSING
    # sizes
    assert status(ok, color_pitch=w * 8 - 4) == ERR_SIZE
    assert status(ok, depth_pitch=w * 2 - 2) == ERR_SIZE
    assert status(ok, depth_pitch=w * 2 + 1) == ERR_SIZE
    assert status(ok, color_t=int(color.data_ptr()) + 2) == ERR_SIZE
    # sh_components
    assert status([obj(A), obj(B4)]) == ERR_ARG
    # tile rows
    r.set_tile_rows(1, 2)
    assert status(ok) == ERR_UNSUPPORTED
    # two rows failing at once: the earlier row decides
    assert status([obj(A), obj(B4)]) == ERR_ARG                                        # sh before tile rows
    assert status([obj(A), obj(B4)], color_pitch=w * 8 - 4) == ERR_SIZE                # size before sh
    assert status(ok, color_t=None, depth_pitch=w * 2 + 1) == ERR_MISSING              # missing before size
    assert status(ok, color_t=None, width=w + 1) == ERR_DIMS                           # dimensions before missing
    assert status([obj(A), obj(B, count=1025)], width=0) == ERR_COUNT                  # count before dimensions
    r.set_tile_rows(0, 0)
    cuda.cuda.synchronize()
    assert (color.cpu().numpy() == FILL).all() and (depth.cpu().numpy() == FILL).all(), "a refused call wrote"
    assert status([obj(A), obj(B, count=0, gaussians=False, harmonics=False)]) == 0  # (NULL with a count of 0)
    assert status(ok) == 0
    cuda.cuda.synchronize()
    assert not (color.cpu().numpy()[:h] == FILL).all(), "an accepted call renders"
    r.close()


# ---- 13. shared capacity ----
@pytest.mark.gpu
def test_shared_capacity_overflow_and_the_next_frame(gsm, cuda, oracle):
    from gsm_amd import scenes
    w, h = 640, 360
    fat = [gen(cuda, 1024, w, h, 1, 0, 150 + i, scale_px=12.0) for i in range(2)]
    thin = [gen(cuda, 1024, w, h, 1, 0, 152 + i) for i in range(2)]
    cam = scenes.make_camera(w, h)
    M = 2048
    ref = checker_frame([(s, cam) for s in fat], w, h, M)
    assert ref["overflow"] == 1, "the test's premise: the objects together exceed 4 * max_gaussians assignments"
    r = handle(gsm, M, w, h, 0)
    composite(gsm, cuda, r, [(s, cam) for s in fat], w, h)  # (GSM_OK; no bytes compared)
    c = r.counters()
    assert c["overflow"] == 1 and c["total_assignments"] == 4 * M
    gc, gd = composite(gsm, cuda, r, [(s, cam) for s in thin], w, h)
    assert r.counters()["overflow"] == 0
    r.close()
    cat = concat(cuda, thin)
    rs = handle(gsm, M, w, h, 0)
    sc_, sd_ = single(gsm, cuda, rs, cat, cam, w, h)
    rs.close()
    assert np.array_equal(gc, sc_), diff(gc, sc_)
    assert np.array_equal(gd, sd_), diff(gd, sd_)
