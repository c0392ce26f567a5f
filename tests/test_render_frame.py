"""gsm_global_render_frame and gsm_global_select_pick (include/gsm_renderer.h) against the checker
(tests/frame/frame_ref.c): the occluded pick walk in every instance, the identities with the existing entries, the
composite, handle reuse and graph replay, the select, and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_render_pick import (FILL, NONE, Targets, cus, far_scene, gen, handle, handle_size_for_tiles,  # noqa: E402
                              to_dev)
from test_render_occluded import ramp_occluder, random_occluder, visible_depths  # noqa: E402

ERR_COUNT, ERR_DIMS, ERR_SIZE, ERR_RENDER_FAILED, ERR_MISSING, ERR_ARG, ERR_UNSUPPORTED = 6, 7, 8, 11, 13, 14, 15


# ---- helpers ----
def dev_f32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def run_frame(gsm, torch, r, objects, w, h, pick=True, occ=None, states=None, styles=None, pad=2, stream=None):
    """One render_frame into fresh sentinel targets: (colour, depth, pick or None); the padding is checked."""
    t = Targets(torch, w, h, pad)
    r.render_frame(t.color, t.depth, objects, w, h, pick=t.pick if pick else None,
                   occluder=None if occ is None else dev_f32(torch, occ), states=states, styles=styles,
                   pick_pitch=t.pick_pitch, stream=stream)
    c, d, p = t.read(with_pick=pick)
    return (c, d, p) if pick else (c, d, None)


def ref_frame(objs, sh, w, h, styles=None, M=None, mw=None, mh=None):
    import frame_ref
    n = sum(len(o[0]) for o in objs)
    fr = frame_ref.frame(objs, sh, w, h, styles=styles, max_gaussians=M or max(n, 1), max_width=mw or w,
                         max_height=mh or h)
    assert fr.overflow == 0
    return fr


def assert_frame(got, res, h, w, what=""):
    gc, gd, gp = got
    oc, od = res["color"].view(np.uint8).reshape(h, -1), res["depth"].view(np.uint8).reshape(h, -1)
    bad = np.argwhere(gc.reshape(h, w, 8) != oc.reshape(h, w, 8))
    assert len(bad) == 0, f"{what}: {len(bad)} colour bytes differ, first (y, x, byte) {bad[:4].tolist()}"
    assert np.array_equal(gd, od), f"{what}: depth differs"
    if gp is not None:
        bad = np.argwhere(gp != res["items"])
        assert len(bad) == 0, f"{what}: {len(bad)} picks differ, first (y, x) {bad[:4].tolist()}"


def occluder_depths(fr, res):
    return visible_depths({"sorted_values": fr.sorted_values, "records": res["records"]})


def single(gsm, sc, cam):
    return (sc.input(gsm), gsm.CameraParams.from_dict(cam))


def check_occluded_pick(gsm, torch, sc, cam, w, h, make_occ, mw=None, mh=None, M=None, kind=None, pad=2):
    """render_frame with an occluder and a pick target against the checker; the occluder comes from the checker's
    own depths.  Returns (checker frame results: occluded, free; the occluder)."""
    mw, mh, M = mw or w, mh or h, M or max(sc.n, 1)
    with ref_frame([(sc.world_np, sc.harm_np, cam)], sc.sh, w, h, M=M, mw=mw, mh=mh) as fr:
        free = fr.walk(None)
        occ = make_occ(occluder_depths(fr, free))
        res = fr.walk(occ)
        active = fr.active_pixels()
    r = handle(gsm, M, mw, mh, sc.prec)
    got = run_frame(gsm, torch, r, single(gsm, sc, cam), w, h, occ=occ, pad=pad)
    assert r.counters()["overflow"] == 0
    if kind is not None:
        assert r.blend_kernel_kind() == kind
    r.close()
    assert_frame(got, res, h, w, "occluder + pick")
    return res, free, occ, active


def assert_not_vacuous(res, free, active):
    """From the checker alone: the occluder changes picks, closes pixels before their first contribution, and leaves
    opened and closed pixels side by side in the active tiles."""
    assert (res["pick"] != free["pick"]).any(), "the occluder changes no pick"
    assert (active & res["closed"] & (res["pick"] == NONE) & (free["pick"] != NONE)).any(), \
        "no pixel of an active tile lost its pick to the occluder"
    assert (active & res["closed"]).any() and (active & ~res["closed"]).any()


# ---- 0. declaration, export, binding (no GPU) ----
def test_frame_entries_are_declared_exported_and_bound(gsm, tmp_path):
    import ctypes as C
    import re
    root = os.path.dirname(HERE)
    src = open(os.path.join(root, "include", "gsm_renderer.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    for name in ("gsm_global_render_frame", "gsm_global_select_pick"):
        assert re.search(r"gsm_status\s+%s\s*\(" % name, src), name
        assert f" T {name}\n" in out, name
        assert name in gsm._SIGNATURES
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    for name in ("render_frame", "select_pick"):
        assert callable(getattr(gsm.GlobalRenderer, name, None)), name
    prog = tmp_path / "size.c"
    prog.write_text('#include "gsm_renderer.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(gsm_global_frame), offsetof(gsm_global_frame, color),'
                    ' offsetof(gsm_global_frame, states), offsetof(gsm_global_frame, flags));return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(prog), "-o", str(tmp_path / "size")], check=True)
    sizes = [int(x) for x in subprocess.run([str(tmp_path / "size")], capture_output=True, text=True,
                                            check=True).stdout.split()]
    F = gsm._GlobalFrame
    assert sizes == [C.sizeof(F), F.color.offset, F.states.offset, F.flags.offset] and sizes[0] == gsm.GLOBAL_FRAME_BYTES
    assert len(gsm._SIGNATURES["gsm_global_select_pick"][0]) == 14
    # the header no longer says that the pick entries have no occluder and the occluded entries no styles
    assert "the pick entries, the DepthFirst" not in src and "the occluded entries, the DepthFirst" not in src


def test_c_program_uses_only_declared_entry_points():
    import re
    src = open(os.path.join(HERE, "c", "frame_sequence.c")).read()
    hdr = open(os.path.join(HERE, "..", "include", "gsm_renderer.h")).read()
    names = set(re.findall(r"\b(gsm_\w+)\(", src))
    assert {"gsm_global_render_frame", "gsm_global_select_pick"} <= names
    for name in names:
        assert re.search(rf"\b{name}\(", hdr), name


# ---- 1. checker parity ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec,sh", [(1, 16), (0, 1)])
@pytest.mark.parametrize("w,h,pad", [(320, 180, 2), (203, 77, 2)])
def test_render_frame_with_occluder_and_pick_matches_the_checker(gsm, cuda, prec, sh, w, h, pad):
    """320x180: aligned targets (8-byte pick stores and occluder loads).  203x77: an odd width, the occluder's pitch
    and the pick's are no multiple of 8 (4-byte accesses)."""
    from gsm_amd import scenes
    sc = gen(cuda, 4096, w, h, sh, prec, 3)
    res, free, occ, active = check_occluded_pick(gsm, cuda, sc, scenes.make_camera(w, h), w, h,
                                                 lambda deps: random_occluder(deps, w, h, 7), pad=pad)
    assert_not_vacuous(res, free, active)


# ---- 2. the rule that motivates the feature ----
@pytest.mark.gpu
def test_no_pick_lies_behind_a_constant_surface(gsm, cuda):
    from gsm_amd import scenes
    w, h = 320, 180
    sc = gen(cuda, 4096, w, h, 1, 0, 3)
    cam = scenes.make_camera(w, h)
    with ref_frame([(sc.world_np, sc.harm_np, cam)], sc.sh, w, h) as fr:
        deps = occluder_depths(fr, fr.walk(None))
    Z = np.float32(deps[int(0.4 * len(deps))])
    zh = np.float32(np.float16(Z))
    r = handle(gsm, sc.n, w, h, sc.prec)
    r.set_profiling(stage_events=False, capture=True)
    _, _, gp = run_frame(gsm, cuda, r, single(gsm, sc, cam), w, h, occ=np.full((h, w), Z, np.float32))
    dep = r.copy_buffer(gsm.BufferId.RENDER_DATA)["depth"].view(np.float16).astype(np.float32)
    _, _, fp = run_frame(gsm, cuda, r, single(gsm, sc, cam), w, h)
    r.close()
    assert (gp != NONE).any() and (dep[gp[gp != NONE]] <= zh).all(), "a pick behind the surface"
    assert (dep[fp[fp != NONE]] > zh).any(), "the test's premise: the un-occluded pick frame picks behind the surface"


# ---- 3. every instance ----
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["quadrant-8", "quadrant-12", "quadrant-16", "half-8", "half-12", "half-16"])
def test_both_unit_shapes_and_every_wave_count(gsm, cuda, monkeypatch, case):
    """The host's rule (gsm_blend.hip): quadrant units while T <= 8 C, half-tile units beyond; 16 waves from 96 C
    units, 12 from 24 C, else 8; quadrant units reach 16 waves by the handle's GSM_BLEND_WAVES=16 override."""
    from gsm_amd import scenes
    C_ = cus(cuda)
    w, h = 320, 180
    shape, waves = case.split("-")
    if shape == "quadrant":
        kind = 1
        tiles = {"8": 120, "12": 6 * C_, "16": 120}[waves]
        if waves == "16":
            monkeypatch.setenv("GSM_BLEND_WAVES", "16")
    else:
        kind = 2
        tiles = {"8": 8 * C_ + 1, "12": 12 * C_, "16": 48 * C_}[waves]
    mw, mh = (w, h) if tiles == 120 else handle_size_for_tiles(tiles)
    T = ((mw + 31) // 32) * ((mh + 15) // 16)
    assert (T <= 8 * C_) == (kind == 1) and T <= 65536
    sc = gen(cuda, 4096, w, h, 1, 0, 4)
    res, free, occ, active = check_occluded_pick(gsm, cuda, sc, scenes.make_camera(w, h), w, h,
                                                 lambda deps: random_occluder(deps, w, h, 11), mw=mw, mh=mh, kind=kind)
    assert_not_vacuous(res, free, active)


# ---- 4. the exact rewalk ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
def test_units_walked_again_exactly_keep_the_cut_and_the_pick(gsm, cuda, kind):
    w, h = 320, 180
    sc, cam, far = far_scene(cuda, 0)
    mw, mh = (w, h) if kind == 1 else handle_size_for_tiles(8 * cus(cuda) + 1)

    def make(deps):
        occ = random_occluder(deps[np.isfinite(deps)], w, h, 5)
        occ[:, : w // 2] = np.inf  # the far records stay visible on the left half
        return occ
    res, free, occ, active = check_occluded_pick(gsm, cuda, sc, cam, w, h, make, mw=mw, mh=mh, M=4 * sc.n, kind=kind)
    listed = np.unique(fr_listed(res, sc, cam, w, h, mw, mh))
    assert ((res["records"][listed, 9] & 0x7C00) == 0x7C00).any(), "the test's premise: a listed record of inf depth"
    assert np.isin(res["pick"], far).any(), "the test's premise: an inf-depth record is picked"
    assert (res["pick"] != free["pick"]).any() and res["closed"].any()


def fr_listed(res, sc, cam, w, h, mw, mh):
    with ref_frame([(sc.world_np, sc.harm_np, cam)], sc.sh, w, h, M=4 * sc.n, mw=mw, mh=mh) as fr:
        return fr.sorted_values[fr.sorted_values >= 0]


# ---- 5. long walks ----
LONG = dict(n=8192, w=64, h=32, spread=0.5, scale_px=1.2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("prec", [0, 1])
def test_long_walks_are_cut_in_every_batch_position(gsm, cuda, kind, prec):
    """Opacities of [0.02, 0.05] on 8192 small gaussians over 64x32: lists of hundreds of entries, the four-batch
    pipeline turns over more than once; a ramp occluder cuts the walks at every depth, so at every list position."""
    from gsm_amd import scenes
    w, h = LONG["w"], LONG["h"]
    sc = gen(cuda, LONG["n"], w, h, 1, prec, 21, opacity=(0.02, 0.05), spread=LONG["spread"],
             scale_px=LONG["scale_px"])
    mw, mh = (64, 32) if kind == 1 else handle_size_for_tiles(8 * cus(cuda) + 1)
    res, free, occ, active = check_occluded_pick(gsm, cuda, sc, scenes.make_camera(w, h), w, h,
                                                 lambda deps: ramp_occluder(deps, w, h), mw=mw, mh=mh, M=4 * sc.n,
                                                 kind=kind)
    assert (res["pick"] != free["pick"]).any() and res["closed"].any() and not res["closed"].all()


# ---- 6. identities ----
@pytest.mark.gpu
def test_every_null_option_combination_equals_the_existing_entry(gsm, cuda):
    from gsm_amd import scenes
    w, h = 203, 77
    sc = gen(cuda, 4096, w, h, 4, 1, 3)
    cam = scenes.make_camera(w, h)
    camp = gsm.CameraParams.from_dict(cam)
    inp = sc.input(gsm)
    rng = np.random.default_rng(1)
    state = cuda.from_numpy(rng.integers(0, 3, sc.n).astype(np.uint8)).cuda()
    styles = [gsm.Style(), gsm.Style((255, 40, 0), 200, 255, False), gsm.Style((0, 0, 0), 0, 255, True)]
    r = handle(gsm, sc.n, w, h, sc.prec)

    def old(call, pick):
        t = Targets(cuda, w, h)
        call(t)
        c, d, p = t.read(with_pick=pick)
        return (c, d, p) if pick else (c, d, None)

    def same(a, b, what):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
        assert (a[2] is None) == (b[2] is None) and (a[2] is None or np.array_equal(a[2], b[2])), what

    one = (inp, camp)
    objs = [gsm.SceneObject(inp, camp)]
    plain = old(lambda t: r.render(t.color, t.depth, inp, camp, w, h), False)
    same(run_frame(gsm, cuda, r, one, w, h, pick=False), plain, "plain")
    # the surface: the median of the plain frame's own nonzero depths, nothing occluded on the left third
    dimg = plain[1].view(np.float16).astype(np.float32)
    occ = np.full((h, w), np.median(dimg[np.isfinite(dimg) & (dimg > 0)]), np.float32)
    occ[:, : w // 3] = np.inf
    occ_t = dev_f32(cuda, occ)
    pickf = old(lambda t: r.render_pick(t.color, t.depth, t.pick, inp, camp, w, h, pick_pitch=t.pick_pitch), True)
    same(run_frame(gsm, cuda, r, one, w, h), pickf, "pick")
    same(run_frame(gsm, cuda, r, one, w, h, pick=False, occ=occ),
         old(lambda t: r.render_occluded(t.color, t.depth, occ_t, inp, camp, w, h), False), "occluded")
    same(run_frame(gsm, cuda, r, one, w, h, pick=False, states=state, styles=styles),
         old(lambda t: r.render_styled(t.color, t.depth, None, inp, camp, w, h, state, styles), False), "styled")
    same(run_frame(gsm, cuda, r, one, w, h, states=state, styles=styles),
         old(lambda t: r.render_styled(t.color, t.depth, t.pick, inp, camp, w, h, state, styles,
                                       pick_pitch=t.pick_pitch), True), "styled pick")
    # one object: the composite entries give the single entries' bytes through this entry too
    same(run_frame(gsm, cuda, r, objs, w, h, pick=False, occ=occ),
         old(lambda t: r.render_composite_occluded(t.color, t.depth, occ_t, objs, w, h), False), "one-object composite")
    # an all-inf occluder: the pick frame's three targets; an identity table: the unstyled frame
    same(run_frame(gsm, cuda, r, one, w, h, occ=np.full((h, w), np.inf, np.float32)), pickf, "all-inf occluder")
    both = run_frame(gsm, cuda, r, one, w, h, occ=occ)
    same(run_frame(gsm, cuda, r, one, w, h, occ=occ, states=0, styles=[gsm.Style()]), both, "identity styles")
    # the combined frame's colour and depth are the occluded entry's, its pick is not the pick frame's
    occf = old(lambda t: r.render_occluded(t.color, t.depth, occ_t, inp, camp, w, h), False)
    assert np.array_equal(both[0], occf[0]) and np.array_equal(both[1], occf[1])
    assert not np.array_equal(both[2], pickf[2])
    r.close()


# ---- 7. composite ----
def three_objects(gsm, torch, w, h, prec=1, sh=4):
    from gsm_amd import scenes
    scs = [gen(torch, n, w, h, sh, prec, seed=11 + i) for i, n in enumerate((600, 611, 593))]
    cams = [scenes.orbit_camera(w, h, a) for a in (0.0, 20.0, -14.0)]
    rng = np.random.default_rng(5)
    states = [rng.integers(0, 4, 600).astype(np.uint8), 1, rng.integers(0, 4, 593).astype(np.uint8)]
    styles = [(0, 0, 0, 0, 255, 0), (255, 40, 0, 200, 255, 0), (0, 0, 0, 0, 90, 0), (0, 0, 0, 0, 255, 1)]
    return scs, cams, states, styles


def gsm_styles(gsm, styles):
    return [gsm.Style(tuple(s[:3]), s[3], s[4], bool(s[5])) for s in styles]


def dev_states(torch, states):
    return [s if np.isscalar(s) else torch.from_numpy(s.copy()).cuda() for s in states]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_composite_with_styles_occluder_and_pick_matches_the_checker(gsm, cuda, prec):
    import frame_ref
    w, h = 203, 77
    scs, cams, states, styles = three_objects(gsm, cuda, w, h, prec)
    objs_ref = [(s.world_np, s.harm_np, c, st) for s, c, st in zip(scs, cams, states)]
    M = 4096
    with ref_frame(objs_ref, 4, w, h, styles=frame_ref.style_table(styles), M=M) as fr:
        free = fr.walk(None)
        occ = random_occluder(occluder_depths(fr, free), w, h, 9)
        res = fr.walk(occ)
        active = fr.active_pixels()
        first, counts = fr.first, fr.counts
    assert_not_vacuous(res, free, active)
    objects = [gsm.SceneObject(s.input(gsm), gsm.CameraParams.from_dict(c)) for s, c in zip(scs, cams)]
    r = handle(gsm, M, w, h, prec)
    got = run_frame(gsm, cuda, r, objects, w, h, occ=occ, states=dev_states(cuda, states), styles=gsm_styles(gsm, styles))
    assert_frame(got, res, h, w, "composite")
    obj, gid = r.pick_owner(got[2])
    r.close()
    hit = res["pick"] != NONE
    want_obj = np.searchsorted(np.asarray(first), res["pick"][hit], side="right") - 1
    assert hit.any() and len(np.unique(want_obj)) == 3
    assert np.array_equal(obj[hit], want_obj) and np.array_equal(gid[hit], res["pick"][hit] - np.asarray(first)[want_obj])
    assert (obj[~hit] == NONE).all() and (gid[~hit] == NONE).all()


# ---- 8. handle reuse and graph replay ----
@pytest.mark.gpu
def test_all_eight_option_combinations_share_a_handle_and_replay(gsm, cuda):
    w, h = 96, 48
    scs, cams, states, styles = three_objects(gsm, cuda, w, h)
    objects = [gsm.SceneObject(s.input(gsm), gsm.CameraParams.from_dict(c)) for s, c in zip(scs, cams)]
    dstates, dstyles = dev_states(cuda, states), gsm_styles(gsm, styles)
    occ = np.full((h, w), 5.0, np.float32)
    occ[:, : w // 3] = np.inf
    occ[h // 2:, w // 2:] = 2.5
    combos = [(p, o, s) for p in (False, True) for o in (False, True) for s in (False, True)]

    def frame(r, combo):
        p, o, s = combo
        return run_frame(gsm, cuda, r, objects, w, h, pick=p, occ=occ if o else None,
                         states=dstates if s else None, styles=dstyles if s else None)

    fresh = []
    for combo in combos:
        r = handle(gsm, 4096, 192, 48, 1)
        fresh.append((frame(r, combo), r.counters()))
        r.close()
    r = handle(gsm, 4096, 192, 48, 1)
    for rnd in range(2):
        for combo, (want, counters) in zip(combos, fresh):
            got = frame(r, combo)
            for k, (a, b) in enumerate(zip(got, want)):
                assert (a is None and b is None) or np.array_equal(a, b), f"round {rnd + 1}, {combo}: output {k}"
            assert r.counters() == counters, (rnd, combo)
    full = fresh[7][0]
    assert not np.array_equal(full[0], fresh[4][0][0]) and not np.array_equal(full[2], fresh[4][0][2])
    # one captured combined frame, replayed into refilled targets
    t = Targets(cuda, w, h)
    occ_t = dev_f32(cuda, occ)
    s = cuda.cuda.Stream()
    with cuda.cuda.stream(s):
        r.render_frame(t.color, t.depth, objects, w, h, pick=t.pick, occluder=occ_t, states=dstates, styles=dstyles,
                       pick_pitch=t.pick_pitch)  # (a warm call: the lazy allocations are done)
        cuda.cuda.synchronize()
        g = cuda.cuda.CUDAGraph()
        with cuda.cuda.graph(g, stream=s):
            r.render_frame(t.color, t.depth, objects, w, h, pick=t.pick, occluder=occ_t, states=dstates,
                           styles=dstyles, pick_pitch=t.pick_pitch)
    for _ in range(2):
        t.refill()
        g.replay()
        got = t.read()
        for k in range(3):
            assert np.array_equal(got[k], full[k]), f"replay: output {k}"
    r.close()


# ---- 9. select_pick ----
@pytest.mark.gpu
def test_select_pick_selects_what_the_occluded_pick_frame_shows(gsm, cuda):
    import frame_ref
    w, h = 203, 77
    scs, cams, states, styles = three_objects(gsm, cuda, w, h)
    objs_ref = [(s.world_np, s.harm_np, c) for s, c in zip(scs, cams)]
    M = 4096
    with ref_frame(objs_ref, 4, w, h, M=M) as fr:
        occ = random_occluder(occluder_depths(fr, fr.walk(None)), w, h, 9)
        res = fr.walk(occ)
        counts = fr.counts
    bases = [0, 768, 1536]
    objects = [gsm.SceneObject(s.input(gsm), gsm.CameraParams.from_dict(c)) for s, c in zip(scs, cams)]
    r = handle(gsm, M, w, h, 1)
    t = Targets(cuda, w, h)
    r.render_frame(t.color, t.depth, objects, w, h, pick=t.pick, occluder=dev_f32(cuda, occ), pick_pitch=t.pick_pitch)
    _, _, gp = t.read()
    assert np.array_equal(gp, res["items"])
    brush = np.zeros((h, w + 5), np.uint8)
    brush[10:60, 40:170] = 7
    brush_t = cuda.from_numpy(brush).cuda()
    matched = cuda.full((1,), 12345, dtype=cuda.int32, device="cuda")
    GUARD = 16
    for o in (0, 2):
        n = counts[o]
        rng = np.random.default_rng(o)
        host = rng.integers(0, 256, n + GUARD).astype(np.uint8)
        dev = cuda.from_numpy(host.copy()).cuda()
        for what, am, xm, mask, cnt in (("set", ~4, 4, None, n), ("clear", ~1, 0, brush, n), ("toggle", 0xFF, 2, None, n),
                                        ("assign", 0, 77, brush, n - 100), ("toggle", 0xFF, 2, brush, n)):
            want, m = frame_ref.select_pick(gp, mask, bases[o], n, host[:n], cnt, am, xm)
            r.select_pick(t.pick, w, h, o, dev, cnt, am, xm, mask=None if mask is None else brush_t, matched=matched,
                          pick_pitch=t.pick_pitch, mask_pitch=w + 5)
            cuda.cuda.synchronize()
            got = dev.cpu().numpy()
            assert int(matched.item()) == m and m > 0, (o, what)
            assert np.array_equal(got[:n], want), (o, what)
            assert np.array_equal(got[n:], host[n:]), "bytes past gaussian_count were written"
            host[:n] = want
        before = host.copy()
        for _ in range(2):  # toggling twice restores the bytes
            r.select_pick(t.pick, w, h, o, dev, n, 0xFF, 0x80, pick_pitch=t.pick_pitch)
        cuda.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), before)
    # a count of 0 writes 0
    r.select_pick(t.pick, w, h, 1, None, 0, 0, 1, matched=matched, pick_pitch=t.pick_pitch)
    cuda.cuda.synchronize()
    assert int(matched.item()) == 0
    # the selection highlighted: a styled frame over the selected state, against the checker
    sel = np.zeros(counts[0], np.uint8)
    dsel = cuda.from_numpy(sel.copy()).cuda()
    r.render_frame(t.color, t.depth, objects, w, h, pick=t.pick, occluder=dev_f32(cuda, occ), pick_pitch=t.pick_pitch)
    r.select_pick(t.pick, w, h, 0, dsel, counts[0], 0, 1, pick_pitch=t.pick_pitch)
    cuda.cuda.synchronize()
    sel, m = frame_ref.select_pick(gp, None, 0, counts[0], sel, counts[0], 0, 1)
    assert np.array_equal(dsel.cpu().numpy(), sel) and 0 < m < counts[0]
    hl = [(0, 0, 0, 0, 255, 0), (255, 255, 0, 220, 255, 0)]
    with ref_frame([objs_ref[0] + (sel,), objs_ref[1] + (0,), objs_ref[2] + (0,)], 4, w, h,
                   styles=frame_ref.style_table(hl), M=M) as fr:
        want = fr.walk(occ)
    got = run_frame(gsm, cuda, r, objects, w, h, occ=occ, states=[dsel, 0, 0], styles=gsm_styles(gsm, hl))
    assert_frame(got, want, h, w, "highlighted selection")
    assert not np.array_equal(want["color"], res["color"])
    r.close()


# ---- 10. the C program ----
@pytest.mark.gpu
def test_c_program_renders_and_selects_through_the_c_abi(tmp_path):
    import frame_ref
    sys.path.insert(0, os.path.join(HERE, "..", "gsm-renderer_amd"))
    from gsm_amd import scenes
    exe = os.path.join(HERE, "c", "frame_sequence")
    assert os.path.exists(exe), "tests/c/frame_sequence not built (__graft_entry__.build)"
    n, W, H, sh = 4096, 203, 77, 1
    world, harm, cam = scenes.gen_scene(n, W, H, sh, 0, seed=3)
    with ref_frame([(world, np.asarray(harm).reshape(-1), cam)], sh, W, H) as fr:
        deps = occluder_depths(fr, fr.walk(None))
        Z = float(deps[int(0.4 * len(deps))])
        res = fr.walk(np.full((H, W), Z, np.float32))
    (tmp_path / "w.bin").write_bytes(world.tobytes())
    (tmp_path / "h.bin").write_bytes(np.asarray(harm).tobytes())
    cf = np.concatenate([cam["view"], cam["proj"], cam["position"],
                         np.array([cam["focal_x"], cam["focal_y"], cam["near"], cam["far"]], np.float32)])
    (tmp_path / "c.bin").write_bytes(cf.astype(np.float32).tobytes())
    out = tmp_path / "out.bin"
    p = subprocess.run([exe, str(tmp_path / "w.bin"), str(tmp_path / "h.bin"), str(n), str(sh), str(W), str(H),
                        str(tmp_path / "c.bin"), repr(Z), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr + p.stdout
    raw = out.read_bytes()
    px = W * H
    color = np.frombuffer(raw[:px * 8], np.uint16).reshape(H, W, 4)
    pick = np.frombuffer(raw[px * 8:px * 12], np.uint32).reshape(H, W)
    state = np.frombuffer(raw[px * 12:px * 12 + n], np.uint8)
    matched = int(np.frombuffer(raw[px * 12 + n:], np.uint32)[0])
    assert np.array_equal(color, res["color"]) and np.array_equal(pick, res["items"])
    want, m = frame_ref.select_pick(pick, None, 0, n, np.zeros(n, np.uint8), n, 0xFF, 1)
    assert np.array_equal(state, want) and matched == m > 0


# ---- 11. refusals ----
@pytest.mark.gpu
def test_refusals_enqueue_nothing(gsm, cuda):
    """Every row of both check tables, in precedence order: a call that fails two rows reports the earlier one."""
    from gsm_amd import scenes
    w, h = 96, 48
    sc = gen(cuda, 600, w, h, 4, 1, 11)
    sc2 = gen(cuda, 300, w, h, 1, 1, 12)
    camp = gsm.CameraParams.from_dict(scenes.make_camera(w, h))
    inp = sc.input(gsm)
    one = (inp, camp)
    two = [gsm.SceneObject(inp, camp), gsm.SceneObject(inp, camp)]
    mixed = [gsm.SceneObject(inp, camp), gsm.SceneObject(sc2.input(gsm), camp)]
    big = gsm.GaussianInput(sc.world, sc.harm, 5000, 4)
    r = handle(gsm, 2048, w, h, 1)
    t = Targets(cuda, w, h)
    occ_t = dev_f32(cuda, np.full((h, w), 3.0, np.float32))
    st = [gsm.Style()]

    def refused(status, objects, **kw):
        a = dict(pick=t.pick, occluder=occ_t, pick_pitch=t.pick_pitch, width=w, height=h)
        a.update(kw)
        width, height = a.pop("width"), a.pop("height")
        color = a.pop("color", t.color)
        with pytest.raises(gsm.RendererError) as e:
            r.render_frame(color, t.depth, objects, width, height, **a)
        assert e.value.status == status, (status, kw)
        assert t.untouched(), kw

    # frame NULL / flags, before everything else (with a count that would fail too)
    refused(ERR_ARG, (big, camp), null_frame=True)
    refused(ERR_ARG, (big, camp), flags=1)
    # the single and the composite entries' rows, in order
    refused(ERR_COUNT, (big, camp), width=w + 1)
    refused(ERR_COUNT, [], width=w + 1)
    refused(ERR_COUNT, [gsm.SceneObject(big, camp), gsm.SceneObject(inp, camp)], width=0)
    refused(ERR_DIMS, one, width=w + 1, color=None)
    refused(ERR_DIMS, two, height=0, color=None)
    refused(ERR_MISSING, one, color=None, pick_pitch=4)
    refused(ERR_MISSING, None, pick_pitch=4)
    refused(ERR_MISSING, two, color=None, occluder_pitch=4)
    refused(ERR_SIZE, one, pick_pitch=4 * w - 4, states=0)
    refused(ERR_SIZE, one, occluder_pitch=4 * w - 4, states=0)
    refused(ERR_SIZE, two, occluder_pitch=4 * w + 2, styles=st)
    refused(ERR_SIZE, mixed, pick_pitch=4 * w + 2)
    refused(ERR_ARG, mixed)                       # objects that differ in sh_components
    refused(ERR_ARG, one, styles=st)              # styles without states
    refused(ERR_ARG, one, states=0)               # states without styles
    refused(ERR_ARG, two, states=[0, 0])
    refused(ERR_ARG, two, states=[0, 300], styles=st)
    refused(ERR_ARG, one, states=0, styles=st, style_count=257)
    r.set_tile_rows(0, 1)
    refused(ERR_ARG, one, styles=st)              # the styled row comes before the tile rows
    refused(ERR_UNSUPPORTED, one)
    refused(ERR_UNSUPPORTED, one, pick=None, occluder=None, states=0, styles=st)
    refused(ERR_UNSUPPORTED, two, pick=None, occluder=None)
    r.set_tile_rows(0, 0)

    # select_pick: the last frame was not a pick frame
    state = cuda.full((600,), FILL, dtype=cuda.uint8, device="cuda")
    matched = cuda.full((1,), 0x5A5A, dtype=cuda.int32, device="cuda")

    def sel_refused(status, **kw):
        a = dict(pick=t.pick, width=w, height=h, object=0, state=state, gaussian_count=600, pick_pitch=t.pick_pitch,
                 mask=None, mask_pitch=w, matched=matched)
        a.update(kw)
        with pytest.raises(gsm.RendererError) as e:
            r.select_pick(a["pick"], a["width"], a["height"], a["object"], a["state"], a["gaussian_count"], 0, 1,
                          mask=a["mask"], matched=a["matched"], pick_pitch=a["pick_pitch"], mask_pitch=a["mask_pitch"])
        assert e.value.status == status, (status, kw)
        cuda.cuda.synchronize()
        assert (state.cpu().numpy() == FILL).all() and int(matched.item()) == 0x5A5A, kw

    r.render_frame(t.color, t.depth, two, w, h, occluder=occ_t)
    sel_refused(ERR_RENDER_FAILED, object=9)
    r.render_frame(t.color, t.depth, two, w, h, pick=t.pick, occluder=occ_t, pick_pitch=t.pick_pitch)
    mask = cuda.full((h, w), 1, dtype=cuda.uint8, device="cuda")
    sel_refused(ERR_ARG, object=2, gaussian_count=5000)
    sel_refused(ERR_COUNT, gaussian_count=5000, width=0)
    sel_refused(ERR_DIMS, width=0, pick=None)
    sel_refused(ERR_DIMS, width=w - 1, pick=None)
    sel_refused(ERR_DIMS, height=h + 1, pick=None)
    sel_refused(ERR_MISSING, pick=None, pick_pitch=4)
    sel_refused(ERR_MISSING, state=None, pick_pitch=4)
    sel_refused(ERR_SIZE, pick_pitch=4 * w - 4)
    sel_refused(ERR_SIZE, pick_pitch=4 * w + 2)
    sel_refused(ERR_SIZE, mask=mask, mask_pitch=w - 1)
    sel_refused(ERR_SIZE, matched=int(matched.data_ptr()) + 2)
    r.select_pick(t.pick, w, h, 1, state, 600, 0, 1, mask=mask, matched=matched, pick_pitch=t.pick_pitch)
    cuda.cuda.synchronize()
    assert int(matched.item()) != 0x5A5A
    r.close()
