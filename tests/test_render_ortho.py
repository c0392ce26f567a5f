"""Orthographic frames (GSM_FRAME_ORTHOGRAPHIC; include/gsm_renderer.h) bit for bit against the checker
(tests/ortho/ortho_ref.c): the single frame and its options, the composite, the mixed batch, handle reuse, graph
replay and the refusals.  The schedule key's orthographic word is covered on the CPU (tests/host/ortho_key_test.cpp):
no debug entry shows a handle's key, so here an alternating handle is held to its frames' bytes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_render_pick import NONE, Targets, gen, handle, to_dev  # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 14, 15
COUNTS = (1, 255, 256, 257, 3001)
SIZES = ((97, 45), (200, 120), (640, 360))
KINDS = ((1, 16), (0, 1), (0, 16), (1, 1))  # (precision, sh components): both precisions, SH degrees 3 and 0
STYLES = [(0, 0, 0, 0, 255, 0), (255, 32, 0, 160, 255, 0), (0, 0, 0, 0, 90, 0), (0, 0, 0, 0, 255, 1)]


def ortho_cam(w, h, half_height=3.0, angle=0.0, near=0.1):
    """An orthographic camera that frames gen_scene's cloud; angle (radians) turns it about the y axis through the
    cloud's middle."""
    from gsm_amd import scenes
    if angle == 0.0:
        return scenes.ortho_camera(w, h, half_height, near=near)
    c, s = np.float32(np.cos(angle)), np.float32(np.sin(angle))
    V = np.eye(4, dtype=np.float32)
    V[0, 0], V[0, 2], V[2, 0], V[2, 2] = c, s, -s, c
    pivot = np.array([0, 0, 5.5], np.float32)
    V[:3, 3] = pivot - V[:3, :3] @ pivot
    return scenes.ortho_camera(w, h, half_height, near=near, view=V.T.reshape(-1))


def dev_f32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def gsm_styles(gsm, styles):
    return [gsm.Style((s[0], s[1], s[2]), s[3], s[4], bool(s[5])) for s in styles]


def states_of(n, seed):
    return np.random.default_rng(seed).integers(0, len(STYLES) + 1, n).astype(np.uint8)  # (one past the table: identity)


def run(gsm, torch, r, objects, w, h, pick=True, occ=None, states=None, styles=None, ortho=True, stream=None):
    t = Targets(torch, w, h)
    r.render_frame(t.color, t.depth, objects, w, h, pick=t.pick if pick else None,
                   occluder=None if occ is None else dev_f32(torch, occ), states=states, styles=styles,
                   pick_pitch=t.pick_pitch, stream=stream, orthographic=ortho)
    c, d, p = t.read(with_pick=pick)
    return (c, d, p) if pick else (c, d, None)


def assert_frame(got, res, h, w, what=""):
    gc, gd, gp = got
    oc, od = res["color"].view(np.uint8).reshape(h, -1), res["depth"].view(np.uint8).reshape(h, -1)
    bad = np.argwhere(gc.reshape(h, w, 8) != oc.reshape(h, w, 8))
    assert len(bad) == 0, f"{what}: {len(bad)} colour bytes differ, first (y, x, byte) {bad[:4].tolist()}"
    assert np.array_equal(gd, od), f"{what}: depth differs"
    if gp is not None:
        bad = np.argwhere(gp != res["items"])
        assert len(bad) == 0, f"{what}: {len(bad)} picks differ, first (y, x) {bad[:4].tolist()}"


def single(gsm, sc, cam):
    return (sc.input(gsm), gsm.CameraParams.from_dict(cam))


def occluder_for(fr, free, h, w):
    """A depth image from the checker's own depths: a surface through the middle of the visible range on the left
    two thirds, open (+inf) on the right, so pixels close, stay open and lose their pick."""
    dep = free["records"][:, 9].view(np.float16).astype(np.float32)
    vals = dep[np.unique(fr.sorted_values[fr.sorted_values >= 0])] if len(fr.sorted_values) else np.array([5.0])
    occ = np.full((h, w), np.float32(np.median(vals)), np.float32)
    occ[:, (2 * w) // 3:] = np.inf
    return occ


# ---- 0. declaration, export, binding (no GPU) ----
def test_ortho_entries_are_declared_exported_and_bound(gsm):
    import re
    import subprocess
    root = os.path.dirname(HERE)
    src = open(os.path.join(root, "include", "gsm_renderer.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"#define\s+GSM_FRAME_ORTHOGRAPHIC\s+2u\b", src) and gsm.FRAME_ORTHOGRAPHIC == 2
    assert re.search(r"gsm_status\s+gsm_global_select_mask_ortho\s*\(", src)
    assert " T gsm_global_select_mask_ortho\n" in out
    assert gsm._SIGNATURES["gsm_global_select_mask_ortho"] == gsm._SIGNATURES["gsm_global_select_mask"]
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    assert gsm.GLOBAL_FRAME_BYTES == 112
    assert gsm.Frame(None, 1, 1, None).orthographic is False


# ---- 1. the plain single frame: every intermediate ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec,sh", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", COUNTS)
def test_plain_ortho_frame_matches_the_checker_stage_by_stage(gsm, cuda, n, w, h, prec, sh):
    import ortho_ref
    sc = gen(cuda, n, w, h, sh, prec, 7 + n)
    cam = ortho_cam(w, h, angle=0.35)
    r = handle(gsm, n, w, h, prec)
    r.set_profiling(stage_events=True, keep_unsorted=False, capture=True)
    got = run(gsm, cuda, r, single(gsm, sc, cam), w, h)
    with ortho_ref.frame([(sc.world_np, sc.harm_np, cam)], sc.sh, w, h, max_gaussians=n) as fr:
        ref, res = fr.data(), fr.walk()
    assert ref["overflow"] == 0 and r.counters()["overflow"] == 0
    vis = ref["mask"] == 1
    rd = r.copy_buffer(gsm.BufferId.RENDER_DATA)[:n]
    assert np.array_equal(rd[vis], ref["render_data"][vis]), "render data"
    assert np.array_equal(r.copy_buffer(gsm.BufferId.BOUNDS)[:n], ref["bounds"]), "bounds"
    assert np.array_equal(r.copy_buffer(gsm.BufferId.TILE_COUNTS)[:n], ref["tile_counts"]), "tile counts"
    assert r.counters()["total_assignments"] == ref["total_assignments"]
    assert np.array_equal(r.copy_buffer(gsm.BufferId.SORTED_KEYS), ref["sorted_keys"]), "sorted keys"
    assert np.array_equal(r.copy_buffer(gsm.BufferId.SORTED_VALUES), ref["sorted_values"]), "sorted values"
    assert np.array_equal(r.copy_buffer(gsm.BufferId.HEADERS), ref["headers"]), "headers"
    r.close()
    assert_frame(got, res, h, w, "plain")
    if n >= 255:
        assert ref["total_assignments"] > 0 and (res["pick"] != NONE).any()


# ---- 2. styled, pick, occluded, all three ----
@pytest.mark.gpu
@pytest.mark.parametrize("n,w,h,prec,sh", [(3001, 200, 120, 1, 16), (257, 97, 45, 0, 1), (3001, 640, 360, 0, 16),
                                           (256, 200, 120, 1, 1), (255, 640, 360, 1, 16), (1, 97, 45, 0, 16)])
def test_ortho_frame_options_match_the_checker(gsm, cuda, n, w, h, prec, sh):
    """One scene, four frames on one handle: styled (no pick), pick, occluded (no pick), and occluder + styles + pick."""
    import ortho_ref
    sc = gen(cuda, n, w, h, sh, prec, 21 + n)
    cam = ortho_cam(w, h, angle=-0.5)
    states = states_of(n, 3)
    table = ortho_ref.style_table(STYLES)
    objs = single(gsm, sc, cam)
    dstates, dstyles = to_dev(cuda, states), gsm_styles(gsm, STYLES)
    with ortho_ref.frame([(sc.world_np, sc.harm_np, cam)], sc.sh, w, h, max_gaussians=n) as fr, \
            ortho_ref.frame([(sc.world_np, sc.harm_np, cam, states)], sc.sh, w, h, styles=table, max_gaussians=n) as fs:
        free, sfree = fr.walk(), fs.walk()
        occ = occluder_for(fr, free, h, w)
        occluded, full = fr.walk(occ), fs.walk(occ)
        closes = bool(occluded["closed"].any())
    r = handle(gsm, n, w, h, prec)
    assert_frame(run(gsm, cuda, r, objs, w, h, pick=False, states=dstates, styles=dstyles), sfree, h, w, "styled")
    assert_frame(run(gsm, cuda, r, objs, w, h), free, h, w, "pick")
    assert_frame(run(gsm, cuda, r, objs, w, h, pick=False, occ=occ), occluded, h, w, "occluded")
    assert_frame(run(gsm, cuda, r, objs, w, h, occ=occ, states=dstates, styles=dstyles), full, h, w, "all three")
    r.close()
    if n >= 3001:  # from the checker alone: the options change the frame
        assert closes and not np.array_equal(occluded["color"], free["color"])
        assert not np.array_equal(sfree["color"], free["color"]) and not np.array_equal(full["pick"], free["pick"])


# ---- 3. a composite of three objects, one of them empty ----
def three_objects(torch, w, h, prec, sh, n):
    from gsm_amd import scenes
    cam = ortho_cam(w, h, half_height=3.5, angle=0.2)
    scs = [gen(torch, n, w, h, sh, prec, 31), gen(torch, 0, w, h, sh, prec, 1), gen(torch, max(n // 3, 1), w, h, sh, prec, 33)]
    Ms = [np.eye(4), np.eye(4), np.eye(4)]
    a = 0.7
    Ms[0][:3, 3] = [0.5, -0.25, 0.0]
    Ms[2][:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    Ms[2][:3, 3] = [-1.0, 0.5, 2.0]
    cams = [scenes.object_camera(cam, M.T.reshape(-1)) for M in Ms]
    return scs, cams


@pytest.mark.gpu
@pytest.mark.parametrize("n,w,h,prec,sh", [(3001, 200, 120, 1, 16), (257, 640, 360, 0, 1), (256, 97, 45, 0, 16)])
def test_ortho_composite_matches_the_checker(gsm, cuda, n, w, h, prec, sh):
    import ortho_ref
    scs, cams = three_objects(cuda, w, h, prec, sh, n)
    total = sum(s.n for s in scs)
    M = 256 * sum((s.n + 255) // 256 for s in scs)
    states = [states_of(scs[0].n, 5), 1, states_of(scs[2].n, 6)]
    table = ortho_ref.style_table(STYLES)
    objects = [gsm.SceneObject(s.input(gsm), gsm.CameraParams.from_dict(c)) for s, c in zip(scs, cams)]
    dstates = [to_dev(cuda, states[0]), 1, to_dev(cuda, states[2])]
    plain = [(s.world_np, s.harm_np, c) for s, c in zip(scs, cams)]
    with ortho_ref.frame(plain, sh, w, h, max_gaussians=M) as fr, \
            ortho_ref.frame([p + (st,) for p, st in zip(plain, states)], sh, w, h, styles=table, max_gaussians=M) as fs:
        free = fr.walk()
        occ = occluder_for(fr, free, h, w)
        full = fs.walk(occ)
        assert fr.overflow == 0 and fr.count == total
    r = handle(gsm, M, w, h, prec)
    assert_frame(run(gsm, cuda, r, objects, w, h), free, h, w, "composite")
    assert_frame(run(gsm, cuda, r, objects, w, h, occ=occ, states=dstates, styles=gsm_styles(gsm, STYLES)), full, h, w,
                 "composite, all three")
    r.close()
    if n >= 3001:
        owners = set(np.searchsorted(np.cumsum([256 * ((s.n + 255) // 256) for s in scs]),
                                     free["items"][free["items"] != NONE], side="right").tolist())
        assert owners == {0, 2}, "both non-empty objects are picked somewhere"


# ---- 4. the quad view: one perspective and three orthographic views in one batch ----
def quad(gsm, torch, prec, sh, n, sizes):
    from gsm_amd import scenes
    sc = gen(torch, n, sizes[0][0], sizes[0][1], sh, prec, 41)
    cams = [scenes.make_camera(*sizes[0]), ortho_cam(*sizes[1]), ortho_cam(*sizes[2], angle=np.pi / 2),
            ortho_cam(*sizes[3], half_height=4.0, angle=-0.4)]
    return sc, cams


@pytest.mark.gpu
@pytest.mark.parametrize("prec,sh,n", [(1, 16, 3001), (0, 1, 257), (0, 16, 255), (1, 1, 256)])
def test_quad_batch_equals_each_view_alone(gsm, cuda, prec, sh, n):
    """Mixed options: view 0 perspective with a pick target, view 1 orthographic and styled, view 2 orthographic with
    an occluder and a pick target, view 3 orthographic and plain.  Each view equals render_frame of that view alone,
    and the orthographic ones equal the checker."""
    import ortho_ref
    sizes = [(200, 120), (97, 45), (200, 120), (640, 360)]
    sc, cams = quad(gsm, cuda, prec, sh, n, sizes)
    states, dstyles = to_dev(cuda, states_of(n, 8)), gsm_styles(gsm, STYLES)
    occ = np.full((sizes[2][1], sizes[2][0]), 5.5, np.float32)
    occ[:, : sizes[2][0] // 4] = np.inf
    opts = [dict(pick=True, ortho=False), dict(pick=False, states=states, styles=dstyles), dict(pick=True, occ=occ),
            dict(pick=False)]
    M, mw, mh = 4 * 256 * ((n + 255) // 256), 640 + 200, 360 + 120
    alone = []
    for (w, h), cam, o in zip(sizes, cams, opts):
        r = handle(gsm, M, mw, mh, prec)
        alone.append(run(gsm, cuda, r, single(gsm, sc, cam), w, h, **o))
        r.close()
    ts = [Targets(cuda, w, h) for w, h in sizes]
    frames = []
    for (w, h), cam, o, t in zip(sizes, cams, opts, ts):
        frames.append(gsm.Frame(single(gsm, sc, cam), w, h, t.color, t.depth, pick=t.pick if o["pick"] else None,
                                occluder=dev_f32(cuda, o["occ"]) if "occ" in o else None, states=o.get("states"),
                                styles=o.get("styles"), pick_pitch=t.pick_pitch, orthographic=o.get("ortho", True)))
    r = handle(gsm, M, mw, mh, prec)
    r.render_frames(frames)
    for v, (t, o, want) in enumerate(zip(ts, opts, alone)):
        c, d, p = t.read(with_pick=o["pick"])
        assert np.array_equal(c, want[0]) and np.array_equal(d, want[1]), f"view {v}"
        if o["pick"]:
            assert np.array_equal(p, want[2]), f"view {v}: pick"
    assert r.counters()["overflow"] == 0
    r.close()
    w, h = sizes[3]  # the plain orthographic view against the checker (views 1 and 2: test 2's frames, alone)
    with ortho_ref.frame([(sc.world_np, sc.harm_np, cams[3])], sh, w, h, max_gaussians=M, max_width=mw,
                         max_height=mh) as fr:
        assert_frame((alone[3][0], alone[3][1], None), fr.walk(), h, w, "view 3")


@pytest.mark.gpu
def test_batch_without_an_orthographic_view_is_todays_batch(gsm, cuda):
    """render_frames with the flag in no frame: the bytes and the blend kernel of render_batch for the same views
    (the plain batch's path), and of render_frames with an option (the batch-with-options path) as before."""
    from gsm_amd import scenes
    sizes, n, prec, sh = [(200, 120), (97, 45)], 3001, 1, 16
    sc = gen(cuda, n, 200, 120, sh, prec, 43)
    cams = [scenes.make_camera(*s) for s in sizes]
    M, mw, mh = 2 * 256 * ((n + 255) // 256), 297, 120
    out, kinds = {}, {}
    for mode in ("batch", "frames", "frames_pick"):
        ts = [Targets(cuda, w, h) for w, h in sizes]
        r = handle(gsm, M, mw, mh, prec)
        if mode == "batch":
            r.render_batch([gsm.BatchView(sc.input(gsm), gsm.CameraParams.from_dict(c), w, h, t.color, t.depth)
                            for (w, h), c, t in zip(sizes, cams, ts)])
        else:
            r.render_frames([gsm.Frame(single(gsm, sc, c), w, h, t.color, t.depth,
                                       pick=t.pick if mode == "frames_pick" else None, pick_pitch=t.pick_pitch,
                                       orthographic=False) for (w, h), c, t in zip(sizes, cams, ts)])
        out[mode] = [t.read(with_pick=mode == "frames_pick")[:2] for t in ts]
        kinds[mode] = r.blend_kernel_kind()
        r.close()
    for v in range(2):
        for k in range(2):
            assert np.array_equal(out["frames"][v][k], out["batch"][v][k]), (v, k)
            assert np.array_equal(out["frames_pick"][v][k], out["batch"][v][k]), (v, k)
    assert kinds["frames"] == kinds["batch"]


# ---- 5. one handle alternating perspective and orthographic frames; graph replay ----
@pytest.mark.gpu
def test_alternating_handle_keeps_every_frames_bytes_and_replays(gsm, cuda):
    from gsm_amd import scenes
    n, w, h, prec, sh = 3001, 200, 120, 1, 16
    sc = gen(cuda, n, w, h, sh, prec, 51)
    pcam, ocam = scenes.make_camera(w, h), ortho_cam(w, h, angle=0.3)
    fresh = {}
    for ortho, cam in ((False, pcam), (True, ocam)):
        r = handle(gsm, n, w, h, prec)
        fresh[ortho] = (run(gsm, cuda, r, single(gsm, sc, cam), w, h, ortho=ortho), r.counters())
        r.close()
    assert not np.array_equal(fresh[False][0][0], fresh[True][0][0])
    r = handle(gsm, n, w, h, prec)
    for rnd, ortho in enumerate((False, True, True, False, True, False, False, True)):
        got = run(gsm, cuda, r, single(gsm, sc, ocam if ortho else pcam), w, h, ortho=ortho)
        for k in range(3):
            assert np.array_equal(got[k], fresh[ortho][0][k]), f"frame {rnd} (orthographic {ortho}): output {k}"
        assert r.counters() == fresh[ortho][1]
    # the perspective frame through this entry is gsm_global_render's
    t = Targets(cuda, w, h)
    r.render(t.color, t.depth, sc.input(gsm), gsm.CameraParams.from_dict(pcam), w, h)
    c, d, _ = t.read(with_pick=False)
    assert np.array_equal(c, fresh[False][0][0]) and np.array_equal(d, fresh[False][0][1])
    # one captured orthographic frame, replayed into refilled targets
    t = Targets(cuda, w, h)
    objs = single(gsm, sc, ocam)
    s = cuda.cuda.Stream()
    with cuda.cuda.stream(s):
        r.render_frame(t.color, t.depth, objs, w, h, pick=t.pick, pick_pitch=t.pick_pitch, orthographic=True)
        cuda.cuda.synchronize()
        g = cuda.cuda.CUDAGraph()
        with cuda.cuda.graph(g, stream=s):
            r.render_frame(t.color, t.depth, objs, w, h, pick=t.pick, pick_pitch=t.pick_pitch, orthographic=True)
    for _ in range(2):
        t.refill()
        g.replay()
        got = t.read()
        for k in range(3):
            assert np.array_equal(got[k], fresh[True][0][k]), f"replay: output {k}"
    r.close()


# ---- 6. refusals ----
@pytest.mark.gpu
def test_flag_refusals_enqueue_nothing(gsm, cuda):
    n, w, h = 256, 97, 45
    sc = gen(cuda, n, w, h, 1, 0, 61)
    cam = ortho_cam(w, h)
    objs = single(gsm, sc, cam)
    r = handle(gsm, n, w, 2 * h, 0)
    t = Targets(cuda, w, h)

    def status(fn):
        with pytest.raises(gsm.RendererError) as e:
            fn()
        assert t.untouched()
        return e.value.status

    for flags in (1, 3, 4, 0x80000002):  # bit 0 stays reserved; every other unknown bit too
        assert status(lambda: r.render_frame(t.color, t.depth, objs, w, h, flags=flags)) == ERR_ARG, flags
        assert status(lambda: r.render_frames([gsm.Frame(objs, w, h, t.color, t.depth, flags=flags)])) == ERR_ARG
    # (flags == 1 with the keyword too: the reserved bit is refused before the flag is looked at)
    assert status(lambda: r.render_frame(t.color, t.depth, objs, w, h, flags=1, orthographic=True)) == ERR_ARG
    # a handle restricted to tile rows: the plain perspective frame runs, the orthographic one is refused
    r.set_tile_rows(1, 3)
    assert status(lambda: r.render_frame(t.color, t.depth, objs, w, h, orthographic=True)) == ERR_UNSUPPORTED
    assert status(lambda: r.render_frames([gsm.Frame(objs, w, h, t.color, t.depth, orthographic=True)])) == ERR_UNSUPPORTED
    r.render_frame(t.color, t.depth, objs, w, h)
    cuda.cuda.synchronize()
    r.set_tile_rows(0, 0)
    r.render_frame(t.color, t.depth, objs, w, h, orthographic=True)
    t.read(with_pick=False)
    r.close()
