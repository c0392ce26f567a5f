"""gsm_global_select_where and gsm_global_state_bounds against their restatement in numpy
(tests/select_where_ref.py): every state byte with its guard bytes, the matched count and the eight words of the
bounds, for equality.  Then the loop the entries exist for (select in a box -> bounds -> extract -> bounds of the
extract -> its frame), every refusal row in order, graph replay, and the same through the C ABI alone
(tests/c/select_where_sequence.c)."""
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

import extract_ref  # noqa: E402
import select_where_ref as ref  # noqa: E402

ERR_COUNT, ERR_SIZE, ERR_MISSING, ERR_ARG = 6, 8, 13, 14
GUARD, GFILL, MFILL, BFILL = 37, 0xC3, 0x7FFFFFFF, 0x5A5A5A5A
COUNTS = [1, 255, 256, 257, 1000]
N = 3000
F = np.float32
INF = float("inf")
CSRC = os.path.join(ROOT, "gsm-renderer_amd", "csrc")
CHECK_SRC = os.path.join(HERE, "host", "select_check_test.cpp")
SEQ_BIN = os.path.join(HERE, "c", "select_where_sequence")
ALL_KEEP = [0xFFFFFFFF] * 8

# the shapes of the tests: an axis-aligned box and a sphere whose faces are exact in float32, and a rotated,
# anisotropic box
CENTER, HALF, RADIUS = (0.25, -0.5, 5.0), (1.0, 0.5, 2.0), 2.0
_a = np.radians(30.0)
ROT = np.array([[np.cos(_a), np.sin(_a), 0.0], [-np.sin(_a), np.cos(_a), 0.0], [0.0, 0.0, 1.0]])
ROT = ROT @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.4), np.sin(0.4)], [0.0, -np.sin(0.4), np.cos(0.4)]])
ROT = ROT @ np.array([[np.cos(0.7), 0.0, -np.sin(0.7)], [0.0, 1.0, 0.0], [np.sin(0.7), 0.0, np.cos(0.7)]])
RCENTER, RHALF = (0.3, -0.2, 5.5), (0.7, 1.3, 2.1)


def shapes():
    from gsm_amd import scenes
    return {"box": (ref.BOX, scenes.box_to_shape(CENTER, HALF)),
            "sphere": (ref.ELLIPSOID, scenes.sphere_to_shape(CENTER, RADIUS)),
            "rotated box": (ref.BOX, scenes.box_to_shape(RCENTER, RHALF, ROT)),
            "rotated ellipsoid": (ref.ELLIPSOID, scenes.box_to_shape(RCENTER, RHALF, ROT))}


def setf(world, name, idx, value):
    """world[name][idx] = value, as fp16 bits where the field is fp16"""
    if world[name].dtype == np.uint16:
        world[name][idx] = np.asarray(value, np.float16).view(np.uint16)
    else:
        world[name][idx] = value


def edge_scene(prec, n=N, seed=7):
    """gen_scene, then from record 0 on: NaN and infinite coordinates, NaN opacity, NaN scales (one, two, all three),
    positions exactly on the faces of the box and at radius 1 of the sphere with the neighbouring floats on both
    sides, and the centre.  The first record has a NaN coordinate, so a scene of one gaussian is that case."""
    from gsm_amd import scenes
    world, _, _ = scenes.gen_scene(n, 64, 64, 1, prec, seed=seed)
    nan = float("nan")
    world["px"][0] = nan
    world["py"][1] = INF
    world["pz"][2] = -INF
    world["px"][3], world["py"][3], world["pz"][3] = CENTER
    setf(world, "opacity", 3, nan)
    world["px"][4], world["py"][4], world["pz"][4] = CENTER
    setf(world, "sx", 4, nan)
    world["px"][5], world["py"][5], world["pz"][5] = CENTER
    for k in ("sx", "sy", "sz"):
        setf(world, k, 5, nan)
    world["px"][6], world["py"][6], world["pz"][6] = CENTER
    setf(world, "sy", 6, nan)
    setf(world, "sz", 6, nan)
    i = 7
    c = np.asarray(CENTER, F)
    for axis in range(3):
        for ext in (HALF[axis], RADIUS):          # the box's faces, the sphere's poles
            for sign in (-1.0, 1.0):
                face = F(c[axis] + F(sign * ext))
                for p in (face, np.nextafter(face, F(-INF)), np.nextafter(face, F(INF))):
                    q = c.copy()
                    q[axis] = p
                    world["px"][i], world["py"][i], world["pz"][i] = q
                    i += 1
    assert i <= min(n, 255), "the special records lie in the first block"
    return world


def classes_present(world):
    """the premise of the contract test, asserted on the input"""
    S = shapes()
    px, py, pz, o, sx, sy, sz = ref.attributes(world)
    one, above, below = F(1), F(1.000001), F(0.999999)   # (a few units in the last place on either side of 1)
    q = np.abs(np.stack(ref.shape_q(S["box"][1], px, py, pz)))
    for axis in range(3):
        with np.errstate(invalid="ignore"):
            others = np.delete(q, axis, axis=0).max(axis=0) < 1
            on, out, in_ = q[axis] == one, (q[axis] > one) & (q[axis] < above), (q[axis] < one) & (q[axis] > below)
        assert (others & on).any() and (others & out).any() and (others & in_).any(), f"box axis {axis}"
    v = ref.shape_q(S["sphere"][1], px, py, pz)
    with np.errstate(all="ignore"):
        s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        assert (s == one).any() and ((s > one) & (s < above)).any() and ((s < one) & (s > below)).any()
    assert np.isnan(px).any() and np.isinf(py).any() and np.isinf(pz).any() and np.isnan(o).any()
    nans = np.isnan(sx).astype(int) + np.isnan(sy) + np.isnan(sz)
    assert (nans == 1).any() and (nans == 2).any() and (nans == 3).any()
    A = S["rotated box"][1].reshape(3, 4)
    assert (A[:, :3] != 0).all(), "the rotated box has no zero entry"
    inside = ref.matches(world, ref.query(ref.BOX, 0, A), np.zeros(len(world), np.uint8))
    assert 0 < inside.sum() < len(world)


def py_query(gsm, q):
    return gsm.SelectQuery(q["shape"], q["flags"], tuple(float(v) for v in q["to_shape"]), float(q["opacity"][0]),
                           float(q["opacity"][1]), float(q["scale"][0]), float(q["scale"][1]), q["test"][0],
                           q["test"][1])


def to_dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def run_where(gsm, torch, r, dworld, n, q, state, a, x, hidden=None, shift=0):
    """(the new state bytes, matched) from the GPU.  The state array starts `shift` bytes past an aligned address;
    the bytes before it, the GUARD bytes past the count and the word after `matched` must keep their values."""
    buf = torch.from_numpy(np.concatenate([np.full(shift, GFILL, np.uint8), state[:n],
                                           np.full(GUARD, GFILL, np.uint8)])).cuda()
    matched = torch.full((2,), MFILL, dtype=torch.int32, device="cuda")
    styles = None if hidden is None else [gsm.Style(hidden=bool(h)) for h in hidden]
    r.select_where(gsm.GaussianInput(dworld, None, n, 0), py_query(gsm, q), buf[shift:], a, x, styles=styles,
                   matched=matched)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:shift] == GFILL).all() and (out[shift + n:] == GFILL).all(), "bytes outside the count were written"
    m = matched.tolist()
    assert m[1] == MFILL
    return out[shift:shift + n], m[0]


def check_where(gsm, torch, r, world, dworld, n, q, state, a, x, hidden=None, shift=0, what=""):
    want, nwant = ref.select_where(world[:n], q, state[:n], a, x, hidden)
    got, ngot = run_where(gsm, torch, r, dworld, n, q, state, a, x, hidden, shift)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} states differ, first {bad[:5].tolist()}"
    assert ngot == nwant, what
    return want, nwant


def run_bounds(gsm, torch, r, dworld, n, state, keep):
    """the eight words of the bounds from the GPU; the words past them keep their sentinel.  state: a uint8 array,
    an int, or a device tensor"""
    out = torch.full((8 + 3,), BFILL, dtype=torch.int32, device="cuda")
    dstate = torch.from_numpy(state).cuda() if isinstance(state, np.ndarray) else state
    r.state_bounds(gsm.GaussianInput(dworld, None, n, 0), dstate, keep, out)
    torch.cuda.synchronize()
    w = out.cpu().numpy().view(np.uint32)
    assert (w[8:] == BFILL).all(), "words past the bounds were written"
    return w[:8]


def handle(gsm, n, prec):
    from test_render_pick import handle as h
    return h(gsm, n, 64, 64, prec)


# ---- CPU: declaration, layout, defaults, refusals without a device, the reference on hand-made cases ----
def test_entries_are_declared_exported_and_bound(gsm):
    src = open(os.path.join(ROOT, "include", "gsm_renderer.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    for name, ret in (("gsm_global_select_where", "gsm_status"), ("gsm_global_state_bounds", "gsm_status"),
                      ("gsm_global_select_query_default", "void")):
        assert re.search(r"%s\s+%s\s*\(" % (ret, name), src), name
        assert f" T {name}\n" in out, name
        assert name in gsm._SIGNATURES, name
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    for name in ("select_where", "state_bounds"):
        assert callable(getattr(gsm.GlobalRenderer, name, None)), name
    from gsm_amd import scenes
    assert callable(scenes.box_to_shape) and callable(scenes.sphere_to_shape)
    q = gsm.SelectQuery()
    assert (q.shape, q.flags, q.test_mask, q.test_value) == (0, 0, 0, 0)
    assert (gsm.SELECT_ALL, gsm.SELECT_BOX, gsm.SELECT_ELLIPSOID, gsm.SELECT_OUTSIDE) == (0, 1, 2, 1)
    for name, v in (("GSM_SELECT_ALL", 0), ("GSM_SELECT_BOX", 1), ("GSM_SELECT_ELLIPSOID", 2), ("GSM_SELECT_OUTSIDE", 1)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, v), src), name


def test_structs_are_80_and_32_bytes(gsm, tmp_path):
    fields = [("gsm_global_select_query", f) for f in ("shape", "flags", "to_shape", "opacity_min", "opacity_max",
                                                       "scale_min", "scale_max", "test_mask", "test_value")]
    fields += [("gsm_global_bounds", f) for f in ("min", "max", "count", "skipped")]
    offs = ", ".join(f"offsetof({t}, {f})" for t, f in fields)
    prog = tmp_path / "size.c"
    prog.write_text('#include "gsm_renderer.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){size_t v[] = {sizeof(gsm_global_select_query), sizeof(gsm_global_bounds), %s};\n'
                    'for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);return 0;}\n' % offs)
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Q, B = gsm._SelectQuery, gsm._Bounds
    want = [80, 32] + [getattr(Q if t.endswith("query") else B, f).offset for t, f in fields]
    assert got == want
    assert C.sizeof(Q) == 80 and C.sizeof(B) == 32


def test_query_default_gives_the_stated_defaults(gsm):
    q = gsm.select_query_default()
    assert q == gsm.SelectQuery()
    assert (q.shape, q.flags) == (gsm.SELECT_ALL, 0) and q.to_shape == ref.IDENTITY
    assert (q.opacity_min, q.opacity_max, q.scale_min, q.scale_max) == (-INF, INF, -INF, INF)
    assert (q.test_mask, q.test_value) == (0, 0)
    gsm._lib().gsm_global_select_query_default(None)   # (a NULL query: nothing to fill)


def test_null_handle_is_refused(gsm):
    L = gsm._lib()
    inp, st, q = gsm._Input(None, None, 0, 0), gsm._State(None, 0, 0), gsm._SelectQuery()
    keep = (C.c_uint32 * 8)()
    assert L.gsm_global_select_where(None, None, C.byref(inp), C.byref(q), None, None, 0, 0, 0, None) == ERR_ARG
    assert L.gsm_global_select_where(None, None, None, None, None, None, 0, 0, 0, 2) == ERR_ARG
    assert L.gsm_global_state_bounds(None, None, C.byref(inp), C.byref(st), keep, 16) == ERR_ARG
    assert L.gsm_global_state_bounds(None, None, None, None, None, None) == ERR_ARG


def test_every_refusal_row_on_the_cpu(tmp_path):
    """tests/host/select_check_test.cpp: the checks' header alone, every row of both tables and their order and the
    query's defaults -- a stand-alone program built with the address and undefined-behaviour sanitizers and run
    here, with no device and no Python in its process."""
    exe = tmp_path / "select_check_test"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", "-I" + CSRC, "-o", str(exe), CHECK_SRC], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout


def test_c_source_uses_only_declared_entry_points():
    src = open(os.path.join(HERE, "c", "select_where_sequence.c")).read()
    hdrs = open(os.path.join(ROOT, "include", "gsm_renderer.h")).read()
    names = set(re.findall(r"\b(gsm_\w+)\(", src))
    assert {"gsm_global_select_where", "gsm_global_state_bounds", "gsm_global_select_query_default",
            "gsm_global_extract", "gsm_global_render", "gsm_global_keep_masked"} <= names
    for name in names:
        assert re.search(rf"\b{name}\(", hdrs), name


def test_shape_helpers():
    from gsm_amd import scenes
    A = scenes.box_to_shape(CENTER, HALF)
    assert A.dtype == np.float32 and A.shape == (12,)
    assert A.tolist() == [1, 0, 0, -0.25, 0, 2, 0, 1, 0, 0, 0.5, -2.5]
    assert scenes.sphere_to_shape(CENTER, RADIUS).tolist() == [0.5, 0, 0, -0.125, 0, 0.5, 0, 0.25, 0, 0, 0.5, -2.5]
    R = scenes.box_to_shape(RCENTER, RHALF, ROT).astype(np.float64).reshape(3, 4)
    for r in range(3):   # the centre maps to 0 and the end of axis r to the unit vector r
        assert np.allclose(R[:, :3] @ np.asarray(RCENTER) + R[:, 3], 0, atol=1e-6)
        assert np.allclose(R[:, :3] @ (np.asarray(RCENTER) + RHALF[r] * ROT[r]) + R[:, 3], np.eye(3)[r], atol=1e-6)


@pytest.mark.parametrize("prec", [0, 1])
def test_reference_on_hand_made_cases(prec):
    from gsm_amd.types import WORLD16, WORLD32
    nan = float("nan")
    w = np.zeros(6, WORLD16 if prec else WORLD32)
    pos = [(1.0, 0.0, 0.0),                         # on a face of the unit box, at radius 1 of the unit ball
           (float(np.nextafter(F(1), F(2))), 0, 0),  # the next float outside
           (nan, 0.0, 0.0),                         # a NaN coordinate
           (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)]
    for i, p in enumerate(pos):
        w["px"][i], w["py"][i], w["pz"][i] = p
        setf(w, "opacity", i, 0.5)
        for k in ("sx", "sy", "sz"):
            setf(w, k, i, 0.25)
    setf(w, "opacity", 3, nan)                      # NaN opacity
    for k in ("sx", "sy", "sz"):
        setf(w, k, 4, nan)                          # all three scales NaN
    setf(w, "sx", 5, nan)                           # one scale NaN: the largest is still 0.25
    st = np.zeros(6, np.uint8)
    for shape in (ref.BOX, ref.ELLIPSOID):
        assert ref.matches(w, ref.query(shape), st).tolist() == [True, False, False, True, True, True]
        assert ref.matches(w, ref.query(shape, ref.OUTSIDE), st).tolist() == [False, True, False, False, False, False]
    # the (-inf, +inf) ranges are not applied: NaN attributes match; any other range is false for them
    assert ref.matches(w, ref.query(), st).all()
    assert ref.matches(w, ref.query(opacity=(-INF, 3e38)), st).tolist() == [True, True, True, False, True, True]
    assert ref.matches(w, ref.query(opacity=(0.5, 0.5)), st).tolist() == [True, True, True, False, True, True]
    assert ref.matches(w, ref.query(scale=(-3e38, INF)), st).tolist() == [True, True, True, True, False, True]
    assert ref.matches(w, ref.query(scale=(0.25, 0.25)), st).tolist() == [True, True, True, True, False, True]
    assert not ref.matches(w, ref.query(scale=(0.26, INF)), st).any()
    # the state test, the hidden rule, the update
    st = np.array([0, 1, 2, 3, 4, 5, 99], np.uint8)   # (one byte past the count)
    assert ref.matches(w, ref.query(test=(1, 1)), st).tolist() == [False, True, False, True, False, True]
    assert ref.matches(w, ref.query(test=(1, 3)), st).tolist() == [False] * 6
    assert ref.matches(w, ref.query(), st, hidden=[0, 1, 0, 1]).tolist() == [True, False, True, False, True, True]
    out, m = ref.select_where(w, ref.query(test=(1, 1)), st, ~0x40, 0x40)
    assert out.tolist() == [0, 0x41, 2, 0x43, 4, 0x45, 99] and m == 3
    # the bounds: -0 counts as +0, non-finite positions are skipped, an empty set
    w["px"][:] = [-0.0, 0.0, nan, -2.0, 3.0, INF]
    b = ref.state_bounds(w, 7, extract_ref.keep_bits(ALL_KEEP))
    assert b[:6].view(F).tolist() == [-2, 0, 0, 3, 0, 0] and b[6:].tolist() == [4, 2]
    b = ref.state_bounds(w[:2], 7, extract_ref.keep_bits(ALL_KEEP))
    assert b.tolist() == [0, 0, 0, 0, 0, 0, 2, 0], "one bit pattern for a zero"
    b = ref.state_bounds(w, 7, extract_ref.keep_bits([0] * 8))
    assert b[:6].view(F).tolist() == [INF] * 3 + [-INF] * 3 and b[6:].tolist() == [0, 0]


# ---- 1. the shapes against the reference ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_select_where_matches_the_reference(gsm, cuda, prec):
    """Every shape with and without OUTSIDE, and no shape, over the edge scene at the full count; then counts 1, 255,
    256, 257 and 1000 with the state array 0 to 3 bytes past an aligned address."""
    world = edge_scene(prec)
    classes_present(world)
    dworld = to_dev(cuda, world)
    rng = np.random.default_rng(prec)
    state = rng.integers(0, 256, N).astype(np.uint8)
    r = handle(gsm, N, prec)
    cases = [("all", ref.query())]
    for name, (shape, A) in shapes().items():
        cases += [(name, ref.query(shape, 0, A)), (name + " outside", ref.query(shape, ref.OUTSIDE, A))]
    for name, q in cases:
        _, m = check_where(gsm, cuda, r, world, dworld, N, q, state, 0, 0x9C, what=name)
        if name == "all":
            assert m == N
        else:
            assert 0 < m < N, name
    shift = 0
    for n in COUNTS:
        for name, q in cases:
            shift = (shift + 1) % 4
            check_where(gsm, cuda, r, world, dworld, n, q, state, 0xFF, 0x02, shift=shift, what=f"{name} n {n}")
    # an inside and its outside part the gaussians without a NaN in q
    q_in, q_out = cases[1][1], cases[2][1]
    a = ref.matches(world, q_in, state)
    b = ref.matches(world, q_out, state)
    assert not (a & b).any() and (~(a | b)).sum() == 3, "the three records with a NaN or infinite coordinate"
    r.close()


# ---- 2. the attribute ranges ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_attribute_ranges(gsm, cuda, prec):
    """Each range alone and both together; bounds equal to a record's own value (inclusive on both sides); a range
    of (-inf, +inf) beside a NaN attribute matches it, any other range does not; a reversed range matches nothing."""
    world = edge_scene(prec)
    dworld = to_dev(cuda, world)
    px, py, pz, o, sx, sy, sz = ref.attributes(world)
    with np.errstate(invalid="ignore"):
        big = np.fmax(np.fmax(sx, sy), sz)
    o50, s50 = float(o[50]), float(big[50])
    olo, ohi = float(np.nanpercentile(o, 30)), float(np.nanpercentile(o, 70))
    slo = float(np.nanpercentile(big, 60))
    state = np.zeros(N, np.uint8)
    r = handle(gsm, N, prec)
    cases = {"opacity": ref.query(opacity=(olo, ohi)), "floaters": ref.query(opacity=(-INF, olo)),
             "needles": ref.query(scale=(slo, INF)), "never drawn": ref.query(scale=(-INF, 0.0005)),
             "both": ref.query(opacity=(olo, INF), scale=(-INF, slo)),
             "opacity at a record's value": ref.query(opacity=(o50, o50)),
             "scale at a record's value": ref.query(scale=(s50, s50)),
             "opacity upper bound 3e38": ref.query(opacity=(-INF, 3e38)),
             "scale lower bound -3e38": ref.query(scale=(-3e38, INF)),
             "not applied": ref.query(), "reversed": ref.query(opacity=(ohi, olo)),
             "in a box": ref.query(ref.BOX, 0, shapes()["rotated box"][1], opacity=(olo, INF), scale=(-INF, slo))}
    got = {}
    for name, q in cases.items():
        want, got[name] = check_where(gsm, cuda, r, world, dworld, N, q, state, 0, 1, what=name)
        if name == "opacity at a record's value":
            assert want[50] == 1
        if name == "scale at a record's value":
            assert want[50] == 1
    assert 0 < got["opacity"] < N and 0 < got["floaters"] < N and 0 < got["needles"] < N and 0 < got["both"] < N
    assert got["never drawn"] == 0 and got["reversed"] == 0 and 0 < got["in a box"] < got["both"]
    assert got["opacity at a record's value"] >= 1 and got["scale at a record's value"] >= 1
    assert got["not applied"] == N
    assert got["opacity upper bound 3e38"] == N - 1, "the record with a NaN opacity"
    assert got["scale lower bound -3e38"] == N - 1, "the record whose three scales are NaN"
    # a record the frame never draws is selectable: give some a scale below the projection's cull
    for k in ("sx", "sy", "sz"):
        setf(world, k, slice(100, 110), 0.0003)
    _, m = check_where(gsm, cuda, r, world, to_dev(cuda, world), N, cases["never drawn"], state, 0, 1)
    assert m == 10
    r.close()


# ---- 3. the state test and the hidden rule ----
@pytest.mark.gpu
def test_state_test_and_hidden_styles(gsm, cuda):
    """Refine within the selection: a second select tests the selection bit, so only selected gaussians can match.
    A hidden state is not selectable with the style table and selectable without it; states at or past the table
    take the identity."""
    prec = 1
    world = edge_scene(prec)
    dworld = to_dev(cuda, world)
    r = handle(gsm, N, prec)
    S = shapes()
    state0 = np.zeros(N, np.uint8)
    sel, m1 = check_where(gsm, cuda, r, world, dworld, N, ref.query(ref.ELLIPSOID, 0, S["sphere"][1]), state0, ~1, 1)
    q2 = ref.query(ref.BOX, ref.OUTSIDE, S["rotated box"][1], test=(1, 1))
    refined, m2 = check_where(gsm, cuda, r, world, dworld, N, q2, sel, ~1, 0, what="refine")
    assert 0 < m2 < m1 and (refined & 1).sum() == m1 - m2 and not (refined[sel == 0] & 1).any()
    # a test value with a bit outside the mask matches nothing; only the low byte of either counts
    _, m = check_where(gsm, cuda, r, world, dworld, N, ref.query(test=(1, 3)), sel, 0, 0x55)
    assert m == 0
    _, m = check_where(gsm, cuda, r, world, dworld, N, ref.query(test=(0x101, 0x301)), sel, 0, 0x55)
    assert m == m1
    rng = np.random.default_rng(3)
    st = rng.integers(0, 8, N).astype(np.uint8)
    hidden = [0, 0, 1, 0, 0, 1]     # states 2 and 5 hidden; 6 and 7 past the table
    for h in (hidden, None):
        want, m = check_where(gsm, cuda, r, world, dworld, N, ref.query(), st, 0, 0x77, hidden=h, what=f"hidden {h}")
        gone = (st == 2) | (st == 5)
        if h is None:
            assert m == N and (want == 0x77).all()
        else:
            assert m == N - gone.sum() and np.array_equal(want[gone], st[gone]) and (want[~gone] == 0x77).all()
    r.close()


# ---- 4. the update idioms ----
OPS = {"set": (~0x40, 0x40), "clear": (~0x01, 0), "toggle": (0xFF, 0x02), "assign": (0, 0x9C)}


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(OPS))
def test_update_idioms(gsm, cuda, op):
    prec = 0
    world = edge_scene(prec)
    dworld = to_dev(cuda, world)
    state = np.random.default_rng(4).integers(0, 256, N).astype(np.uint8)
    r = handle(gsm, N, prec)
    a, x = OPS[op]
    q = ref.query(ref.BOX, 0, shapes()["rotated box"][1])
    want, m = check_where(gsm, cuda, r, world, dworld, N, q, state, a, x, what=op)
    hit = ref.matches(world, q, state)
    assert 0 < m == hit.sum() and np.array_equal(want[~hit], state[~hit])
    if op == "set":
        assert (want[hit] & 0x40).all() and np.array_equal(want[hit] | 0x40, state[hit] | 0x40)
    elif op == "clear":
        assert not (want[hit] & 1).any()
    elif op == "toggle":
        assert np.array_equal(want[hit], state[hit] ^ 2)
    else:
        assert (want[hit] == 0x9C).all()
    r.close()


# ---- 5. no shape, no range, no test, no styles ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_select_all_matches_every_gaussian(gsm, cuda, prec):
    world = edge_scene(prec)
    dworld = to_dev(cuda, world)
    state = np.random.default_rng(5).integers(0, 256, N).astype(np.uint8)
    r = handle(gsm, N, prec)
    for n in COUNTS + [N]:
        got, m = run_where(gsm, cuda, r, dworld, n, ref.query(), state, 0, 0x11, shift=n % 4)
        assert m == n and (got == 0x11).all()   # (run_where asserts that the bytes past the count are untouched)
    # matched NULL, and a count of 0: *matched = 0 and nothing else
    buf = cuda.full((N,), 7, dtype=cuda.uint8, device="cuda")
    r.select_where(gsm.GaussianInput(dworld, None, N, 0), gsm.SelectQuery(), buf, 0, 0x11)
    matched = cuda.full((2,), MFILL, dtype=cuda.int32, device="cuda")
    r.select_where(gsm.GaussianInput(None, None, 0, 0), gsm.SelectQuery(), None, 0, 0x22, matched=matched)
    cuda.cuda.synchronize()
    assert (buf == 0x11).all().item() and matched.tolist() == [0, MFILL]
    r.close()


# ---- 6. the bounds ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_state_bounds_matches_the_reference(gsm, cuda, prec):
    """The whole scene ({NULL, s}), a keep set from keep_masked, an empty keep set, non-finite positions, -0.0 as the
    extreme, and the counts 1, 255, 256, 257, 1000 and 3000."""
    world = edge_scene(prec)
    dworld = to_dev(cuda, world)
    state = np.random.default_rng(6).integers(0, 256, N).astype(np.uint8)
    r = handle(gsm, N, prec)
    empty = np.concatenate([np.full(3, np.inf, F), np.full(3, -np.inf, F)]).view(np.uint32).tolist() + [0, 0]
    for n in COUNTS + [N]:
        w = world[:n]
        got = run_bounds(gsm, cuda, r, dworld, n, 0x21, ALL_KEEP)
        want = ref.state_bounds(w, 0x21, extract_ref.keep_bits(ALL_KEEP))
        assert got.tolist() == want.tolist(), f"whole scene, n {n}"
        assert got[6] + got[7] == n and got[7] == min(n, 3), "the three non-finite positions are skipped"
        for mask, value in ((1, 1), (0xFF, 0x9C), (0x80, 0)):
            keep = gsm.keep_masked(mask, value)
            got = run_bounds(gsm, cuda, r, dworld, n, state, keep)
            want = ref.state_bounds(w, state, extract_ref.keep_bits(keep))
            assert got.tolist() == want.tolist(), f"keep_masked({mask}, {value}), n {n}"
            assert got[6] + got[7] == ((state[:n] & mask) == value).sum()
        assert run_bounds(gsm, cuda, r, dworld, n, state, [0] * 8).tolist() == empty
        assert run_bounds(gsm, cuda, r, dworld, n, 0x21, gsm.keep_masked(0xFF, 0x20)).tolist() == empty
    assert run_bounds(gsm, cuda, r, None, 0, 0, ALL_KEEP).tolist() == empty, "a count of 0"
    # -0.0 as the extreme: all x at or below -0.0, all y at or above it; the result holds +0 in both
    w = world.copy()
    w["px"] = -np.abs(w["px"])
    w["py"] = np.abs(w["py"])
    w["px"][[3, 700]] = -0.0
    w["py"][[4, 900]] = -0.0
    w["pz"][:] = -0.0
    keep = gsm.keep_masked(0, 0)
    got = run_bounds(gsm, cuda, r, to_dev(cuda, w), N, 0, keep)
    assert got.tolist() == ref.state_bounds(w, 0, extract_ref.keep_bits(keep)).tolist()
    assert got[3] == 0 and got[1] == 0 and got[2] == 0 and got[5] == 0, "a -0 extreme is stored as +0"
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65_536, 65_537])
def test_state_bounds_second_round_of_the_final_reduce(gsm, cuda, n):
    """The final reduce walks the partials 256 a round: 65 536 gaussians are 256 partials, one round; 65 537 are 257,
    the smallest count whose last partial is a thread's second.  The extremes sit in the last gaussian."""
    prec = 1
    from gsm_amd import scenes
    world, _, _ = scenes.gen_scene(n, 64, 64, 1, prec, seed=9)
    world["px"][n - 1], world["py"][n - 1], world["pz"][n - 1] = -100.0, 200.0, -300.0
    state = np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
    state[n - 1] = 1
    r = handle(gsm, n, prec)
    dworld = to_dev(cuda, world)
    for st, keep in ((0, ALL_KEEP), (state, gsm.keep_masked(1, 1)), (state, gsm.keep_masked(1, 0))):
        got = run_bounds(gsm, cuda, r, dworld, n, st, keep)
        assert got.tolist() == ref.state_bounds(world, st, extract_ref.keep_bits(keep)).tolist()
    got = run_bounds(gsm, cuda, r, dworld, n, state, gsm.keep_masked(1, 1))
    assert got[:6].view(F)[[0, 4, 2]].tolist() == [-100.0, 200.0, -300.0]
    r.close()


# ---- 7. the loop the entries exist for ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_select_bounds_extract_render_on_one_handle(gsm, cuda, prec):
    """select_where with a box -> state_bounds of the selection, inside the box's own AABB -> extract with
    keep_masked -> state_bounds of the extracted scene with a full keep set, equal word for word -> render of the
    extracted scene equals render_styled of the full scene with the complement hidden, byte for byte."""
    import style_ref
    from gsm_amd import scenes
    from test_extract import Outputs
    from test_render_pick import Targets, gen
    from test_render_pick import handle as frame_handle
    from test_render_styled import styled
    n, w, h, sh = 3000, 200, 120, 4
    sc = gen(cuda, n, w, h, sh, prec, 31)
    cam = scenes.make_camera(w, h)
    A = scenes.box_to_shape(RCENTER, RHALF, ROT)
    r = frame_handle(gsm, n, w, h, prec)
    dstate = cuda.zeros(n, dtype=cuda.uint8, device="cuda")
    matched = cuda.full((1,), MFILL, dtype=cuda.int32, device="cuda")
    q = ref.query(ref.BOX, 0, A)
    r.select_where(sc.input(gsm), py_query(gsm, q), dstate, ~1, 1, matched=matched)
    keep = gsm.keep_masked(1, 1)
    b1 = run_bounds(gsm, cuda, r, sc.world, n, dstate, keep)
    want_state, m = ref.select_where(sc.world_np, q, np.zeros(n, np.uint8), ~1, 1)
    assert np.array_equal(dstate.cpu().numpy(), want_state) and matched.item() == m and 0 < m < n
    assert b1.tolist() == ref.state_bounds(sc.world_np, want_state, extract_ref.keep_bits(keep)).tolist()
    assert b1[6] == m and b1[7] == 0
    signs = 2.0 * np.array(list(np.ndindex(2, 2, 2))) - 1.0
    corners = np.asarray(RCENTER) + (signs * np.asarray(RHALF)) @ ROT   # (ROT's rows are the box axes)
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    mn, mx = b1[:3].view(F).astype(np.float64), b1[3:6].view(F).astype(np.float64)
    assert (mn >= lo).all() and (mx <= hi).all() and (mn <= mx).all(), "the bounds lie inside the box's own AABB"
    o = Outputs(cuda, prec, sh, n)
    o.refill()
    r.extract(sc.input(gsm), dstate, keep, o.g, o.hview, o.s, o.i, kept=o.kept)
    cuda.cuda.synchronize()
    K = int(o.kept[0].item())
    assert K == m
    b2 = run_bounds(gsm, cuda, r, o.g, K, 0, ALL_KEEP)
    assert b2.tolist() == b1.tolist(), "the bounds of the extracted scene equal the selection's word for word"
    table = style_ref.style_table([(0, 0, 0, 0, 255, 1), (0, 0, 0, 0, 255, 0)])   # the complement (state 0) hidden
    c, d, _ = styled(gsm, cuda, r, [(sc, cam)], w, h, [dstate], table)
    t = Targets(cuda, w, h)
    r.render(t.color, t.depth, gsm.GaussianInput(o.g, o.hview, K, sh), gsm.CameraParams.from_dict(cam), w, h)
    c2, d2, _ = t.read(with_pick=False)
    r.close()
    assert np.array_equal(c2, c), "colour"
    assert np.array_equal(d2, d), "depth"
    assert (c2 != 0).any()


# ---- 8. refusals ----
@pytest.mark.gpu
def test_refusals_in_order_enqueue_nothing(gsm, cuda):
    n, prec = 300, 1
    world = edge_scene(prec, 512)
    dworld = to_dev(cuda, world)
    r = handle(gsm, 512, prec)
    state = cuda.full((n + GUARD,), 9, dtype=cuda.uint8, device="cuda")
    matched = cuda.full((2,), MFILL, dtype=cuda.int32, device="cuda")
    bounds = cuda.full((10,), BFILL, dtype=cuda.int32, device="cuda")
    box = shapes()["box"][1]
    good_q = dict(shape=ref.BOX, flags=0, to_shape=tuple(float(v) for v in box))
    good_styles = [gsm.Style()]
    nan = float("nan")

    def ptr(t, off=0):
        return int(t.data_ptr()) + off

    def status(count=n, g=dworld, st=state, mt=matched, styles=None, style_count=None, **q):
        query = None if q.get("null_query") else gsm.SelectQuery(**dict(good_q, **q))
        try:
            r.select_where(gsm.GaussianInput(g, None, count, 0), query, st, 0, 1, styles=styles, matched=mt,
                           style_count=style_count)
        except gsm.RendererError as e:
            return int(e.status)
        return 0

    L = gsm._lib()
    sq = gsm._select_query_struct(gsm.SelectQuery(**good_q))
    assert status(count=513) == ERR_COUNT
    # (the binding always passes an input: a NULL one through ctypes)
    assert L.gsm_global_select_where(r._h, None, None, C.byref(sq), ptr(state), None, 0, 0, 1, ptr(matched)) == ERR_MISSING
    assert status(null_query=True) == ERR_MISSING
    assert status(g=None) == ERR_MISSING and status(st=None) == ERR_MISSING
    for off in (1, 2, 3):
        assert status(mt=ptr(matched, off)) == ERR_SIZE
    assert status(shape=3) == ERR_ARG and status(flags=2) == ERR_ARG and status(flags=3) == ERR_ARG
    assert status(shape=ref.ALL, flags=ref.OUTSIDE) == ERR_ARG
    for k in ("opacity_min", "opacity_max", "scale_min", "scale_max"):
        assert status(**{k: nan}) == ERR_ARG, k
    for i in (0, 5, 11):
        for bad in (nan, INF, -INF):
            A = list(good_q["to_shape"])
            A[i] = bad
            assert status(to_shape=tuple(A)) == ERR_ARG
            assert status(shape=ref.ELLIPSOID, to_shape=tuple(A)) == ERR_ARG
    assert status(style_count=3) == ERR_ARG
    assert status(styles=good_styles, style_count=0) == ERR_ARG and status(styles=good_styles, style_count=257) == ERR_ARG
    # the order: count, missing, size, argument
    assert L.gsm_global_select_where(r._h, None, C.byref(gsm._Input(ptr(dworld), None, 513, 0)), None, ptr(state), None,
                                     0, 0, 1, ptr(matched)) == ERR_COUNT
    assert status(count=513, g=None) == ERR_COUNT
    assert status(st=None, mt=ptr(matched, 2)) == ERR_MISSING
    assert status(null_query=True, mt=ptr(matched, 2)) == ERR_MISSING
    assert status(mt=ptr(matched, 2), shape=3) == ERR_SIZE and status(mt=ptr(matched, 2), style_count=3) == ERR_SIZE

    def bstatus(count=n, g=dworld, st=state, keep=ALL_KEEP, b=bounds):
        try:
            r.state_bounds(gsm.GaussianInput(g, None, count, 0), st, keep, b)
        except gsm.RendererError as e:
            return int(e.status)
        return 0

    assert bstatus(count=513) == ERR_COUNT
    kw = (C.c_uint32 * 8)(*ALL_KEEP)
    sstruct = gsm._State(ptr(state), 0, 0)
    assert L.gsm_global_state_bounds(r._h, None, None, C.byref(sstruct), kw, ptr(bounds)) == ERR_MISSING
    assert bstatus(st=None) == ERR_MISSING and bstatus(keep=None) == ERR_MISSING and bstatus(b=None) == ERR_MISSING
    assert bstatus(g=None) == ERR_MISSING
    for off in (1, 2, 3):
        assert bstatus(b=ptr(bounds, off)) == ERR_SIZE
    assert bstatus(st=256) == ERR_ARG
    # the order
    assert L.gsm_global_state_bounds(r._h, None, C.byref(gsm._Input(ptr(dworld), None, 513, 0)), None, kw,
                                     ptr(bounds)) == ERR_COUNT
    assert bstatus(g=None, b=None) == ERR_MISSING and bstatus(g=None, b=ptr(bounds, 2)) == ERR_MISSING
    assert bstatus(b=ptr(bounds, 2), st=256) == ERR_SIZE
    cuda.cuda.synchronize()
    assert (state == 9).all().item() and matched.tolist() == [MFILL, MFILL], "a refused select wrote"
    assert (bounds.cpu().numpy().view(np.uint32) == BFILL).all(), "a refused state_bounds wrote"
    # what the rows leave alone
    assert status() == 0 and status(mt=None) == 0 and status(shape=ref.ALL, to_shape=(nan,) * 12) == 0
    assert status(opacity_min=INF) == 0 and status(styles=good_styles) == 0
    assert status(count=0, g=None, st=None) == 0
    assert bstatus() == 0 and bstatus(count=0, g=None) == 0 and bstatus(st=255) == 0 and bstatus(b=ptr(bounds, 4)) == 0
    cuda.cuda.synchronize()
    assert (state[n:] == 9).all().item() and matched.tolist() == [0, MFILL]
    r.close()


# ---- 9. capture ----
@pytest.mark.gpu
def test_captured_select_and_bounds_follow_the_replays_state(gsm, cuda):
    """One select_where (with a style table) and one state_bounds in a graph, a linear chain on one stream, replayed
    twice after the state bytes changed: the new bytes, matched and the bounds follow the replay's state bytes and
    are overwritten, not accumulated; the query, the table and the keep set are the captured ones."""
    n, prec = 2500, 0
    world = edge_scene(prec)[:n]
    dworld = to_dev(cuda, world)
    r = handle(gsm, n, prec)
    q = ref.query(ref.ELLIPSOID, 0, shapes()["rotated ellipsoid"][1], test=(0x80, 0))
    hidden = [0, 0, 1]
    keep = gsm.keep_masked(0x40, 0x40)
    dstate = cuda.zeros(n, dtype=cuda.uint8, device="cuda")
    matched = cuda.full((2,), MFILL, dtype=cuda.int32, device="cuda")
    bounds = cuda.full((10,), BFILL, dtype=cuda.int32, device="cuda")
    inp = gsm.GaussianInput(dworld, None, n, 0)
    styles = [gsm.Style(hidden=bool(h)) for h in hidden]
    # (the handle's first calls allocate the style table and the partials: before the capture)
    r.select_where(inp, py_query(gsm, q), dstate, 0xFF, 0, styles=styles, matched=matched)
    r.state_bounds(inp, dstate, keep, bounds)
    cuda.cuda.synchronize()
    s = cuda.cuda.Stream()
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        r.select_where(inp, py_query(gsm, q), dstate, ~0x40, 0x40, styles=styles, matched=matched, stream=s)
        r.state_bounds(inp, dstate, keep, bounds, stream=s)
    cuda.cuda.synchronize()
    # a later call with another table and query on the handle must not change what the graph replays
    r.select_where(inp, gsm.SelectQuery(), cuda.zeros(n, dtype=cuda.uint8, device="cuda"), 0, 1,
                   styles=[gsm.Style(hidden=True)] * 8)
    counts = []
    for seed in (1, 2, 2):
        state = np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)
        dstate.copy_(cuda.from_numpy(state).cuda())
        cuda.cuda.synchronize()
        g.replay()
        cuda.cuda.synchronize()
        want, m = ref.select_where(world, q, state, ~0x40, 0x40, hidden)
        assert 0 < m < n
        assert np.array_equal(dstate.cpu().numpy(), want)
        assert matched.tolist() == [m, MFILL], "matched is overwritten, not added to"
        b = bounds.cpu().numpy().view(np.uint32)
        assert b[:8].tolist() == ref.state_bounds(world, want, extract_ref.keep_bits(keep)).tolist()
        assert (b[8:] == BFILL).all()
        counts.append(m)
    assert counts[0] != counts[1] and counts[1] == counts[2]
    r.close()


# ---- 10. through the C ABI alone ----
@pytest.mark.gpu
def test_select_where_sequence_through_the_c_abi(tmp_path, oracle):
    """tests/c/select_where_sequence.c: select_where, state_bounds, extract, state_bounds of the extract, render -- no
    Python and no torch in that process.  The state bytes and both bounds are compared here with the reference and
    the frame with the oracle."""
    from gsm_amd import scenes
    assert os.path.exists(SEQ_BIN), "tests/c/select_where_sequence not built (__graft_entry__.build)"
    n, W, H, sh = 3000, 320, 180, 4
    world, harm, cam = scenes.gen_scene(n, W, H, sh, 1, seed=12)
    A = scenes.box_to_shape(RCENTER, RHALF, ROT)
    omin = float(F(0.6))
    (tmp_path / "w.bin").write_bytes(world.tobytes())
    (tmp_path / "h.bin").write_bytes(harm.tobytes())
    (tmp_path / "b.bin").write_bytes(A.tobytes())
    cf = np.concatenate([cam["view"], cam["proj"], cam["position"],
                         np.array([cam["focal_x"], cam["focal_y"], cam["near"], cam["far"]], np.float32)])
    (tmp_path / "c.bin").write_bytes(cf.astype(np.float32).tobytes())
    p = subprocess.run([SEQ_BIN, str(tmp_path / "w.bin"), str(tmp_path / "h.bin"), str(n), str(sh), str(W), str(H),
                        str(tmp_path / "c.bin"), str(tmp_path / "b.bin"), repr(omin), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr + p.stdout
    m = re.search(r"matched (\d+) kept (\d+) count (\d+) skipped (\d+)", p.stdout)
    assert m, p.stdout
    matched, kept, count, skipped = (int(x) for x in m.groups())
    q = ref.query(ref.BOX, 0, A, opacity=(omin, INF))
    want, nwant = ref.select_where(world, q, np.full(n, 0x40, np.uint8), ~1, 1)
    assert 0 < nwant < n and matched == nwant and kept == nwant and (count, skipped) == (nwant, 0)
    assert np.array_equal(np.frombuffer((tmp_path / "out.state").read_bytes(), np.uint8), want)
    b = np.frombuffer((tmp_path / "out.bounds").read_bytes(), np.uint32)
    wb = ref.state_bounds(world, want, extract_ref.keep_bits(extract_ref.keep_masked(1, 1)))
    assert b[:8].tolist() == wb.tolist() and b[8:].tolist() == wb.tolist()
    ids = np.frombuffer((tmp_path / "out.ids").read_bytes(), np.uint32)
    assert np.array_equal(ids, np.nonzero(want & 1)[0])
    fr = oracle.render(world[ids], np.asarray(harm).reshape(n, -1)[ids].reshape(-1), sh, cam, W, H, max_gaussians=n)
    got = np.frombuffer((tmp_path / "out.color").read_bytes(), np.uint16).reshape(H, W, 4)
    assert np.array_equal(got, fr["color"])
