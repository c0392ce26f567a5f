"""gsm_global_render_frames and gsm_global_select_pick_ids (include/gsm_renderer.h): several frame
descriptors, each with its own nullable pick target, occluder and styles, in one Global batch.  The acceptance test is
byte equality, per frame, with gsm_global_render_frame of that frame alone on a fresh handle -- an entry that is itself
held to the CPU checker (tests/test_render_frame.py) -- plus one direct comparison with the checker, the identities
with the batch and the single entries, handle reuse and graph replay, the stateless select, and the refusals."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_render_pick import FILL, NONE, PFILL, Scene, Targets, cus, far_scene, gen, handle  # noqa: E402
from test_render_occluded import random_occluder  # noqa: E402
from test_render_frame import (assert_frame, assert_not_vacuous, dev_f32, gsm_styles, occluder_depths,  # noqa: E402
                               ref_frame)

ERR_COUNT, ERR_DIMS, ERR_TILES, ERR_SIZE, ERR_RENDER_FAILED, ERR_MISSING, ERR_ARG, ERR_UNSUPPORTED = \
    6, 7, 9, 8, 11, 13, 14, 15
ENTRIES = ("gsm_global_render_frames", "gsm_global_select_pick_ids")
# hidden, tinted and faded styles next to the identity
STYLES = [(0, 0, 0, 0, 255, 0), (255, 40, 0, 200, 255, 0), (0, 0, 0, 0, 90, 0), (0, 0, 0, 0, 255, 1)]


# ---- 0. declaration, export, binding (no GPU) ----
def test_frames_entries_are_declared_exported_and_bound(gsm):
    root = os.path.dirname(HERE)
    src = open(os.path.join(root, "include", "gsm_renderer.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    for name in ENTRIES:
        assert re.search(r"gsm_status\s+%s\s*\(" % name, src), name
        assert f" T {name}\n" in out, name
        assert name in gsm._SIGNATURES
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    assert len(gsm._SIGNATURES["gsm_global_render_frames"][0]) == 4
    assert len(gsm._SIGNATURES["gsm_global_select_pick_ids"][0]) == 13
    for name in ("render_frames", "select_pick_ids"):
        assert callable(getattr(gsm.GlobalRenderer, name, None)), name


def test_header_no_longer_says_the_batch_takes_no_options():
    src = open(os.path.join(HERE, "..", "include", "gsm_renderer.h")).read()
    flat = " ".join(src.replace("*", " ").split())
    for m in re.finditer(r"gsm_global_render_batch[^.;]*?(have no|take no)[^.;]*", flat):
        raise AssertionError("the header still excludes the batch: " + m.group(0))
    assert "gsm_global_render_views" in flat and re.search(r"gsm_global_render_views[^.;]*?(have no|take no|stays without)",
                                                           flat), "render_views itself stays without options"


def test_frames_c_program_uses_only_declared_entry_points():
    src = open(os.path.join(HERE, "c", "frames_sequence.c")).read()
    hdr = open(os.path.join(HERE, "..", "include", "gsm_renderer.h")).read()
    names = set(re.findall(r"\b(gsm_\w+)\(", src))
    assert set(ENTRIES) <= names
    for name in names:
        assert re.search(rf"\b{name}\(", hdr), name


# ---- helpers ----
class Spec:
    """One frame of a batch: a scene, a camera, a size and its option set."""

    def __init__(self, sc, cam, w, h, pick=True, depth=True, occ=None, states=None, styles=None, pad=2):
        self.sc, self.cam, self.w, self.h = sc, cam, w, h
        self.pick, self.depth, self.occ, self.states, self.styles, self.pad = pick, depth, occ, states, styles, pad


def dev_state(torch, s):
    return s if np.isscalar(s) else torch.from_numpy(np.ascontiguousarray(s, dtype=np.uint8).copy()).cuda()


def descriptor(gsm, torch, sp, t):
    """The gsm.Frame of `sp` into the sentinel targets `t`."""
    return gsm.Frame((sp.sc.input(gsm), gsm.CameraParams.from_dict(sp.cam)), sp.w, sp.h, t.color,
                     t.depth if sp.depth else None, pick=t.pick if sp.pick else None,
                     occluder=None if sp.occ is None else dev_f32(torch, sp.occ),
                     states=None if sp.states is None else dev_state(torch, sp.states),
                     styles=None if sp.styles is None else gsm_styles(gsm, sp.styles), pick_pitch=t.pick_pitch)


def render_alone(r, f):
    r.render_frame(f.color, f.depth, f.objects, f.width, f.height, pick=f.pick, occluder=f.occluder, states=f.states,
                   styles=f.styles, pick_pitch=f.pick_pitch)


def read(t, sp):
    """(colour, depth or None, pick or None) of a frame; a target the frame does not have must hold its sentinel."""
    c, d, p = t.read(with_pick=sp.pick)
    if not sp.depth:
        assert (d == FILL).all(), "a frame without a depth target wrote depth"
    if not sp.pick:
        assert (p == PFILL).all(), "a frame without a pick target wrote picks"
    return c, d if sp.depth else None, p if sp.pick else None


def same(a, b, what):
    for k, name in enumerate(("colour", "depth", "pick")):
        assert (a[k] is None) == (b[k] is None), (what, name)
        if a[k] is not None:
            bad = np.argwhere(a[k] != b[k])
            assert len(bad) == 0, f"{what}: {len(bad)} {name} values differ, first {bad[:4].tolist()}"


def batch_size(specs, min_tiles=0):
    """(max_gaussians, max_width, max_height) of a handle that holds the batch: the items of every scene on 256-item
    boundaries with room for every assignment, and a tile space of at least the frames' tiles (and min_tiles)."""
    items = sum((sp.sc.n + 255) // 256 * 256 for sp in specs)
    tiles = max(sum(((sp.w + 31) // 32) * ((sp.h + 15) // 16) for sp in specs), min_tiles)
    mw = max(sp.w for sp in specs)
    tx = (mw + 31) // 32
    mh = max(max(sp.h for sp in specs), 16 * ((tiles + tx - 1) // tx))
    return max(4 * items, 256), mw, mh


def alone_frames(gsm, torch, specs, prec):
    """Every frame by gsm_global_render_frame on a fresh handle of its own."""
    out = []
    for sp in specs:
        r = handle(gsm, 4 * max(sp.sc.n, 1), sp.w, sp.h, prec)
        t = Targets(torch, sp.w, sp.h, sp.pad)
        render_alone(r, descriptor(gsm, torch, sp, t))
        out.append(read(t, sp))
        assert r.counters()["overflow"] == 0
        r.close()
    return out


def batch_frames(gsm, torch, r, specs, stream=None):
    ts = [Targets(torch, sp.w, sp.h, sp.pad) for sp in specs]
    r.render_frames([descriptor(gsm, torch, sp, t) for sp, t in zip(specs, ts)], stream=stream)
    return [read(t, sp) for sp, t in zip(specs, ts)]


def check_batch(gsm, torch, specs, prec, kind=None, min_tiles=0, want=None):
    """One render_frames on a fresh handle against every frame alone; returns the batch's outputs."""
    want = want or alone_frames(gsm, torch, specs, prec)
    r = handle(gsm, *batch_size(specs, min_tiles), prec)
    got = batch_frames(gsm, torch, r, specs)
    assert r.counters()["overflow"] == 0
    if kind is not None:
        assert r.blend_kernel_kind() == kind
    r.close()
    for v, (a, b) in enumerate(zip(got, want)):
        same(a, b, f"frame {v}")
    return got


def empty_like(torch, sc):
    return Scene(torch, sc.world_np[:0], sc.harm_np[:0], sc.sh)


# ---- 1, 2. mixed options in both precisions; one frame directly against the checker ----
@functools.lru_cache(maxsize=None)
def mixed_case(prec, sh):
    """Three frames of three scenes and three sizes.  Frame 0: occluder + pick + styles, its occluder drawn from the
    checker's own visible depths; frame 1: pick only, no depth target; frame 2: nothing.  The checker's results for
    frame 0 (occluded, free, active pixels) are computed once and shared."""
    import frame_ref
    from gsm_amd import scenes
    sizes = [(320, 180), (203, 77), (96, 64)]
    scs = [gen(None, 4096, w, h, sh, prec, 3 + i) for i, (w, h) in enumerate(sizes)]
    cams = [scenes.make_camera(w, h) for w, h in sizes]
    state = np.random.default_rng(2).integers(0, 5, 4096).astype(np.uint8)  # (4: past the table, the identity)
    w, h = sizes[0]
    with ref_frame([(scs[0].world_np, scs[0].harm_np, cams[0], state)], sh, w, h,
                   styles=frame_ref.style_table(STYLES)) as fr:
        free = fr.walk(None)
        occ = random_occluder(occluder_depths(fr, free), w, h, 7)
        res = fr.walk(occ)
        active = fr.active_pixels()
    return sizes, scs, cams, state, occ, res, free, active


def mixed_specs(torch, prec, sh):
    sizes, scs, cams, state, occ, res, free, active = mixed_case(prec, sh)
    dev = [Scene(torch, s.world_np, s.harm_np, s.sh) for s in scs]
    return [Spec(dev[0], cams[0], *sizes[0], occ=occ, states=state, styles=STYLES),
            Spec(dev[1], cams[1], *sizes[1], depth=False),
            Spec(dev[2], cams[2], *sizes[2], pick=False)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,sh", [(1, 16), (0, 1)])
def test_mixed_options_equal_every_frame_alone_and_the_checker(gsm, cuda, prec, sh):
    specs = mixed_specs(cuda, prec, sh)
    got = check_batch(gsm, cuda, specs, prec)
    # directly against the CPU checker: guards against an error common to both GPU entries
    _, _, _, _, _, res, free, active = mixed_case(prec, sh)
    assert_not_vacuous(res, free, active)
    assert_frame(got[0], res, specs[0].h, specs[0].w, "frame 0 against the checker")
    assert (res["pick"] != NONE).any()


# ---- 3. the pick holds ids, not items ----
@pytest.mark.gpu
def test_pick_pixels_hold_gaussian_ids_not_batch_items(gsm, cuda):
    from gsm_amd import scenes
    w, h = 203, 77
    sc = gen(cuda, 4096, w, h, 1, 0, 3)
    cam = scenes.make_camera(w, h)
    specs = [Spec(sc, cam, w, h), Spec(sc, scenes.orbit_camera(w, h, 15.0), w, h)]
    got = check_batch(gsm, cuda, specs, 0)
    p1 = got[1][2]
    hit = p1 != NONE
    # the second frame's items start at 256 * blockBase = 4096: a stored item would lie at or past it
    assert hit.any() and (p1[hit] < 4096).all() and (p1[hit] < 256).any()


# ---- 4. stereo pair: two frames into one colour, depth and pick image, out of one occluder ----
@pytest.mark.gpu
def test_side_by_side_stereo_pair_with_per_view_alignment(gsm, cuda):
    """Width 203 per eye: the right eye's pick and occluder pointers are 4-byte but not 8-byte aligned (203 * 4 =
    812), its colour pointer 8-byte but not 16-byte aligned; the left eye's are aligned for every wide access.  The
    alignment bits therefore differ between the views of one launch."""
    from gsm_amd import scenes
    w, h, pad = 203, 77, 2
    sc = gen(cuda, 4096, w, h, 1, 0, 5)
    cams = [scenes.orbit_camera(w, h, -2.0), scenes.orbit_camera(w, h, 2.0)]
    with ref_frame([(sc.world_np, sc.harm_np, cams[0])], sc.sh, w, h) as fr:
        deps = occluder_depths(fr, fr.walk(None))
    occ = random_occluder(deps, 2 * w, h, 13)
    specs = [Spec(sc, cams[e], w, h, occ=np.ascontiguousarray(occ[:, e * w:(e + 1) * w])) for e in range(2)]
    want = alone_frames(gsm, cuda, specs, 0)
    t = Targets(cuda, 2 * w, h, pad)
    occ_t = dev_f32(cuda, occ)
    assert t.pick.data_ptr() % 8 == 0 and t.pick_pitch % 8 == 0 and occ_t.data_ptr() % 8 == 0
    frames = []
    for e in range(2):
        frames.append(gsm.Frame((sc.input(gsm), gsm.CameraParams.from_dict(cams[e])), w, h,
                                t.color[:, e * w * 8:], t.depth[:, e * w * 2:], pick=t.pick[:, e * w * 4:],
                                occluder=occ_t[:, e * w:], color_pitch=2 * w * 8, depth_pitch=2 * w * 2,
                                pick_pitch=t.pick_pitch, occluder_pitch=2 * w * 4))
    assert frames[1].pick.data_ptr() % 8 == 4 and frames[1].occluder.data_ptr() % 8 == 4
    r = handle(gsm, *batch_size(specs), 0)
    r.render_frames(frames)
    c, d, p = t.read()
    assert r.counters()["overflow"] == 0
    r.close()
    for e in range(2):
        same((c[:, e * w * 8:(e + 1) * w * 8], d[:, e * w * 2:(e + 1) * w * 2], p[:, e * w:(e + 1) * w]), want[e],
             f"eye {e}")


# ---- 5. every instance ----
def padding_frame(torch, sc, tiles):
    """A frame of an empty scene that only adds `tiles` tiles to the batch (32 tiles per row), colour only."""
    rows = (tiles + 31) // 32
    return Spec(empty_like(torch, sc), None, 1024, 16 * rows, pick=False, depth=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["quadrant-8", "quadrant-12", "quadrant-16", "half-8", "half-12", "half-16"])
def test_both_unit_shapes_and_every_wave_count(gsm, cuda, monkeypatch, case):
    """launch_blend takes the batch's summed tile count: quadrant units while it is <= 8 C, half-tile units beyond.
    The wave count comes from the handle's create-time GSM_BLEND_WAVES override.  Two frames with occluder + pick;
    the half-tile cases add a frame of an empty scene whose tiles carry the sum past 8 C."""
    from gsm_amd import scenes
    shape, waves = case.split("-")
    monkeypatch.setenv("GSM_BLEND_WAVES", waves)
    w, h = 320, 180
    sc = gen(cuda, 4096, w, h, 1, 0, 4)
    cams = [scenes.make_camera(w, h), scenes.orbit_camera(w, h, 10.0)]
    specs = []
    for i, cam in enumerate(cams):
        with ref_frame([(sc.world_np, sc.harm_np, cam)], sc.sh, w, h) as fr:
            occ = random_occluder(occluder_depths(fr, fr.walk(None)), w, h, 11 + i)
        specs.append(Spec(sc, cam, w, h, occ=occ))
    kind = 1
    if shape == "half":
        kind = 2
        pad_sp = padding_frame(cuda, sc, 8 * cus(cuda) + 1 - 240)
        pad_sp.cam = cams[0]
        specs.insert(1, pad_sp)
    tiles = sum(((sp.w + 31) // 32) * ((sp.h + 15) // 16) for sp in specs)
    assert (tiles <= 8 * cus(cuda)) == (kind == 1) and tiles <= 65535
    check_batch(gsm, cuda, specs, 0, kind=kind)


# ---- 6. the exact rewalk ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
def test_units_walked_again_exactly_keep_the_per_view_terms(gsm, cuda, kind):
    """far_scene's inf-depth records in the second frame of a batch (blockBase > 0, tileBase > 0), under an occluder
    whose left half is +inf: walk_unit_exact runs with that view's occluder, pick target and item base."""
    from gsm_amd import scenes
    w, h = 320, 180
    sc, cam, far = far_scene(cuda, 0)
    first = gen(cuda, 4096, w, h, 1, 0, 4)
    with ref_frame([(sc.world_np, sc.harm_np, cam)], sc.sh, w, h, M=4 * sc.n) as fr:
        free = fr.walk(None)
        deps = occluder_depths(fr, free)
        occ = random_occluder(deps[np.isfinite(deps)], w, h, 5)
        occ[:, : w // 2] = np.inf  # the far records stay visible on the left half
        res = fr.walk(occ)
    assert np.isin(res["pick"], far).any(), "the test's premise: an inf-depth record is picked"
    assert (res["pick"] != free["pick"]).any() and res["closed"].any(), "the test's premise: the occluder changes picks"
    specs = [Spec(first, scenes.make_camera(w, h), w, h, pick=False), Spec(sc, cam, w, h, occ=occ)]
    if kind == 2:
        pad_sp = padding_frame(cuda, first, 8 * cus(cuda) + 1 - 240)
        pad_sp.cam = cam
        specs.append(pad_sp)
    got = check_batch(gsm, cuda, specs, 0, kind=kind)
    assert_frame(got[1], res, h, w, "the far frame against the checker")


# ---- 7. views without work ----
@pytest.mark.gpu
def test_an_empty_frame_and_a_fully_occluded_frame(gsm, cuda):
    from gsm_amd import scenes
    w, h = 203, 77
    sc = gen(cuda, 4096, w, h, 1, 0, 3)
    cam = scenes.make_camera(w, h)
    with ref_frame([(sc.world_np, sc.harm_np, cam)], sc.sh, w, h) as fr:
        active = fr.active_pixels()
    specs = [Spec(sc, cam, w, h), Spec(empty_like(cuda, sc), cam, 96, 64),
             Spec(sc, cam, w, h, occ=np.zeros((h, w), np.float32))]
    got = check_batch(gsm, cuda, specs, 0)
    c, d, p = got[2]
    px = c.reshape(h, w, 8)
    assert active.any() and not active.all()
    # closed before the first entry: colour 0, alpha +0, depth 0 and no pick in active tiles; the clear value elsewhere
    assert (px[active] == 0).all() and (d.reshape(h, w, 2)[active] == 0).all() and (p[active] == NONE).all()
    clear = np.array([0, 0, 0, 0x3C00], np.uint16).view(np.uint8)
    assert (px[~active] == clear).all() and (p[~active] == NONE).all()
    ce, de, pe = got[1]
    assert (ce.reshape(64, 96, 8) == clear).all() and (pe == NONE).all()


# ---- 8. identities on one handle ----
@pytest.mark.gpu
def test_identities_with_the_batch_and_the_single_entries(gsm, cuda):
    from gsm_amd import scenes
    sizes = [(203, 77), (96, 64)]
    scs = [gen(cuda, 4096, w, h, 4, 1, 3 + i) for i, (w, h) in enumerate(sizes)]
    cams = [scenes.make_camera(w, h) for w, h in sizes]
    plain = [Spec(s, c, w, h, pick=False, depth=(i == 0)) for i, (s, c, (w, h)) in enumerate(zip(scs, cams, sizes))]
    r = handle(gsm, *batch_size(plain), 1)
    # every option NULL: gsm_global_render_batch's bytes
    ts = [Targets(cuda, sp.w, sp.h) for sp in plain]
    r.render_batch([gsm.BatchView(sp.sc.input(gsm), gsm.CameraParams.from_dict(sp.cam), sp.w, sp.h, t.color,
                                  t.depth if sp.depth else None) for sp, t in zip(plain, ts)])
    want = [read(t, sp) for sp, t in zip(plain, ts)]
    for v, (a, b) in enumerate(zip(batch_frames(gsm, cuda, r, plain), want)):
        same(a, b, f"all options NULL, view {v}")
    # frame_count == 1: gsm_global_render_frame's bytes, on the same handle
    w, h = sizes[0]
    occ = np.full((h, w), 4.0, np.float32)
    occ[:, : w // 3] = np.inf
    state = np.random.default_rng(1).integers(0, 4, 4096).astype(np.uint8)
    one = Spec(scs[0], cams[0], w, h, occ=occ, states=state, styles=STYLES)
    t = Targets(cuda, w, h)
    render_alone(r, descriptor(gsm, cuda, one, t))
    same(batch_frames(gsm, cuda, r, [one])[0], read(t, one), "frame_count == 1")
    # an all-inf occluder: the pick frame's three targets; an identity style table: the unstyled bytes
    pickf = [Spec(s, c, ww, hh) for s, c, (ww, hh) in zip(scs, cams, sizes)]
    want = batch_frames(gsm, cuda, r, pickf)
    inf = [Spec(s, c, ww, hh, occ=np.full((hh, ww), np.inf, np.float32)) for s, c, (ww, hh) in zip(scs, cams, sizes)]
    for v, (a, b) in enumerate(zip(batch_frames(gsm, cuda, r, inf), want)):
        same(a, b, f"all-inf occluder, frame {v}")
    ident = [Spec(s, c, ww, hh, states=0, styles=[STYLES[0]]) for s, c, (ww, hh) in zip(scs, cams, sizes)]
    for v, (a, b) in enumerate(zip(batch_frames(gsm, cuda, r, ident), want)):
        same(a, b, f"identity styles, frame {v}")
    # a styled frame next to an unstyled one: the unstyled one keeps the plain bytes, the styled one does not
    mixed = [Spec(scs[0], cams[0], w, h, states=state, styles=STYLES), pickf[1]]
    got = batch_frames(gsm, cuda, r, mixed)
    same(got[1], want[1], "the unstyled view of a styled batch")
    assert not np.array_equal(got[0][0], want[0][0])
    r.close()


# ---- 9. handle reuse and capture ----
@pytest.mark.gpu
def test_one_handle_through_every_entry_and_a_captured_replay(gsm, cuda):
    specs_a = mixed_specs(cuda, 1, 16)
    # other option sets on the same frames: the options move to the neighbours
    specs_b = [Spec(specs_a[0].sc, specs_a[0].cam, specs_a[0].w, specs_a[0].h, pick=False),
               Spec(specs_a[1].sc, specs_a[1].cam, specs_a[1].w, specs_a[1].h,
                    occ=np.full((specs_a[1].h, specs_a[1].w), 3.5, np.float32), states=1, styles=STYLES),
               Spec(specs_a[2].sc, specs_a[2].cam, specs_a[2].w, specs_a[2].h, depth=False)]
    want_a, want_b = alone_frames(gsm, cuda, specs_a, 1), alone_frames(gsm, cuda, specs_b, 1)
    plain = [Spec(sp.sc, sp.cam, sp.w, sp.h, pick=False) for sp in specs_a]
    want_plain = alone_frames(gsm, cuda, plain, 1)
    r = handle(gsm, *batch_size(specs_a), 1)

    def batch(specs, want, what):
        for v, (a, b) in enumerate(zip(batch_frames(gsm, cuda, r, specs), want)):
            same(a, b, f"{what}, frame {v}")

    batch(specs_a, want_a, "render_frames")
    ts = [Targets(cuda, sp.w, sp.h) for sp in plain]
    r.render_batch([gsm.BatchView(sp.sc.input(gsm), gsm.CameraParams.from_dict(sp.cam), sp.w, sp.h, t.color, t.depth)
                    for sp, t in zip(plain, ts)])
    for v, (sp, t) in enumerate(zip(plain, ts)):
        same(read(t, sp), want_plain[v], f"render_batch, view {v}")
    t = Targets(cuda, specs_a[1].w, specs_a[1].h)
    render_alone(r, descriptor(gsm, cuda, specs_a[1], t))
    same(read(t, specs_a[1]), want_a[1], "render_frame (pick)")
    batch(specs_b, want_b, "render_frames with other option sets")
    t = Targets(cuda, plain[0].w, plain[0].h)
    r.render(t.color, t.depth, plain[0].sc.input(gsm), gsm.CameraParams.from_dict(plain[0].cam), plain[0].w, plain[0].h)
    same(read(t, plain[0]), want_plain[0], "render")
    batch(specs_a, want_a, "render_frames again")
    # one captured replay of a render_frames call into refilled targets
    ts = [Targets(cuda, sp.w, sp.h, sp.pad) for sp in specs_a]
    frames = [descriptor(gsm, cuda, sp, t) for sp, t in zip(specs_a, ts)]
    s = cuda.cuda.Stream()
    with cuda.cuda.stream(s):
        r.render_frames(frames)  # (a warm call: the lazy allocations are done)
        cuda.cuda.synchronize()
        g = cuda.cuda.CUDAGraph()
        with cuda.cuda.graph(g, stream=s):
            r.render_frames(frames)
    for t in ts:
        t.refill()
    g.replay()
    for v, (sp, t) in enumerate(zip(specs_a, ts)):
        same(read(t, sp), want_a[v], f"replay, frame {v}")
    r.close()


# ---- 10. selects ----
def select_ids_ref(pick, mask, state, gaussian_count, and_mask, xor_mask):
    """gsm_global_select_pick_ids' set rule from its contract, in numpy: S = the ids below gaussian_count of the
    pixels under the mask; every id of S is updated once.  Returns (new state, |S|)."""
    h, w = pick.shape
    under = np.ones((h, w), bool) if mask is None else np.asarray(mask)[:h, :w] != 0
    ids = np.unique(pick[under & (pick < gaussian_count)])
    out = np.asarray(state, np.uint8).copy()
    out[ids] = ((out[ids].astype(np.uint32) & (and_mask & 0xFFFFFFFF)) ^ (xor_mask & 0xFFFFFFFF)) & 0xFF
    return out, int(len(ids))


@pytest.mark.gpu
def test_select_pick_ids_and_the_cleared_pick_state(gsm, cuda):
    from gsm_amd import scenes
    w, h = 203, 77
    sc = gen(cuda, 4096, w, h, 1, 0, 3)
    specs = [Spec(sc, scenes.make_camera(w, h), w, h), Spec(sc, scenes.orbit_camera(w, h, 15.0), w, h)]
    r = handle(gsm, *batch_size(specs), 0)
    ts = [Targets(cuda, w, h) for _ in specs]
    # a pick frame first: the batch after it must clear the handle's last-pick state
    render_alone(r, descriptor(gsm, cuda, specs[0], ts[0]))
    r.render_frames([descriptor(gsm, cuda, sp, t) for sp, t in zip(specs, ts)])
    t = ts[1]
    _, _, gp = t.read()
    n, GUARD = sc.n, 16
    with pytest.raises(gsm.RendererError) as e:
        r.pick_owner(gp)
    assert e.value.status == ERR_RENDER_FAILED
    host = np.random.default_rng(0).integers(0, 256, n + GUARD).astype(np.uint8)
    dev = cuda.from_numpy(host.copy()).cuda()
    matched = cuda.full((1,), 12345, dtype=cuda.int32, device="cuda")
    with pytest.raises(gsm.RendererError) as e:
        r.select_pick(t.pick, w, h, 0, dev, n, 0xFF, 1, matched=matched, pick_pitch=t.pick_pitch)
    assert e.value.status == ERR_RENDER_FAILED
    brush = np.zeros((h, w + 5), np.uint8)
    brush[10:60, 40:170] = 7
    brush_t = cuda.from_numpy(brush).cuda()
    multi = np.unique(gp[gp != NONE], return_counts=True)[1].max()
    assert multi > 1, "the test's premise: a splat that covers several pixels"
    for what, am, xm, mask, cnt in (("set", ~4, 4, None, n), ("clear", ~1, 0, brush, n), ("toggle", 0xFF, 2, None, n),
                                    ("assign", 0, 77, brush, n - 1500), ("toggle", 0xFF, 2, brush, n)):
        want, m = select_ids_ref(gp, mask, host[:n], cnt, am, xm)
        r.select_pick_ids(t.pick, w, h, dev, cnt, am, xm, mask=None if mask is None else brush_t, matched=matched,
                          pick_pitch=t.pick_pitch, mask_pitch=w + 5)
        cuda.cuda.synchronize()
        got = dev.cpu().numpy()
        assert int(matched.item()) == m and m > 0, what
        assert np.array_equal(got[:n], want), what
        assert np.array_equal(got[n:], host[n:]), "bytes past gaussian_count were written"
        host[:n] = want
    before = host.copy()
    for _ in range(2):  # toggling twice restores the bytes
        r.select_pick_ids(t.pick, w, h, dev, n, 0xFF, 0x80, pick_pitch=t.pick_pitch)
    cuda.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), before)
    r.select_pick_ids(t.pick, w, h, None, 0, 0, 1, matched=matched, pick_pitch=t.pick_pitch)  # a count of 0 writes 0
    cuda.cuda.synchronize()
    assert int(matched.item()) == 0
    r.close()


# ---- 11. refusals ----
@pytest.mark.gpu
def test_refusals_enqueue_nothing(gsm, cuda):
    """Every row of both check tables in precedence: a call that fails two rows reports the earlier one, two failing
    frames the lower index's (visible where the rows differ).  The sentinel targets stay untouched."""
    from gsm_amd import scenes
    w, h = 96, 48
    sc = gen(cuda, 600, w, h, 4, 1, 11)
    sc2 = gen(cuda, 300, w, h, 1, 1, 12)
    camp = gsm.CameraParams.from_dict(scenes.make_camera(w, h))
    inp, inp2 = sc.input(gsm), sc2.input(gsm)
    big = gsm.GaussianInput(sc.world, sc.harm, 5000, 4)
    r = handle(gsm, 2048, 2 * w, h, 1)
    ta, tb = Targets(cuda, w, h), Targets(cuda, w, h)
    occ_t = dev_f32(cuda, np.full((h, w), 3.0, np.float32))
    st = [gsm.Style()]

    def F(t, objects=None, **kw):
        a = dict(pick=t.pick, occluder=occ_t, pick_pitch=t.pick_pitch, width=w, height=h, color=t.color, depth=t.depth)
        a.update(kw)
        return gsm.Frame(objects if objects is not None else (inp, camp), a.pop("width"), a.pop("height"),
                         a.pop("color"), a.pop("depth"), **a)

    def refused(status, frames):
        with pytest.raises(gsm.RendererError) as e:
            r.render_frames(frames)
        assert e.value.status == status, status
        assert ta.untouched() and tb.untouched()

    two_objects = [gsm.SceneObject(inp, camp), gsm.SceneObject(inp, camp)]
    refused(ERR_MISSING, None)                                              # frames NULL, frame_count 1
    refused(ERR_ARG, [F(ta, two_objects), F(tb, flags=1)])                  # flags before object_count
    refused(ERR_UNSUPPORTED, [F(ta), F(tb, two_objects, width=0)])          # object_count before the batch's rows
    refused(ERR_UNSUPPORTED, [F(ta, [])])                                   # object_count 0
    f = F(tb)
    f.objects = None                                                       # a NULL objects array, object_count 1
    refused(ERR_MISSING, [F(ta, (big, camp)), f])                           # objects NULL before the counts
    refused(ERR_COUNT, [])                                                  # frame_count 0
    refused(ERR_COUNT, [F(ta, width=0), F(tb, (big, camp))])                # counts before dimensions
    refused(ERR_COUNT, [F(ta), F(tb), F(ta), F(tb)])                        # 4 * roundup(600, 256) > 2048
    refused(ERR_DIMS, [F(ta), F(tb, width=2 * w + 1, color=None)])          # dimensions before missing buffers
    refused(ERR_TILES, [F(ta, width=2 * w, color=None), F(tb)])             # tiles before missing buffers
    refused(ERR_MISSING, [F(ta, pick_pitch=4), F(tb, color=None)])          # missing before sizes
    refused(ERR_MISSING, [F(ta), F(tb, (gsm.GaussianInput(None, sc.harm, 600, 4), camp))])
    refused(ERR_SIZE, [F(ta), F(tb, pick_pitch=4 * w - 4, objects=(inp2, camp))])   # sizes before sh_components
    refused(ERR_SIZE, [F(ta), F(tb, occluder_pitch=4 * w - 4)])
    refused(ERR_SIZE, [F(ta, pick_pitch=4 * w + 2), F(tb)])
    refused(ERR_SIZE, [F(ta), F(tb, occluder=int(occ_t.data_ptr()) + 2)])
    refused(ERR_SIZE, [F(ta, color_pitch=8 * w - 4), F(tb)])
    refused(ERR_ARG, [F(ta), F(tb, (inp2, camp))])                          # frames that differ in sh_components
    refused(ERR_ARG, [F(ta), F(tb, styles=st)])                             # styles without states
    refused(ERR_ARG, [F(ta, states=0), F(tb)])                              # states without styles
    refused(ERR_ARG, [F(ta, states=300, styles=st), F(tb)])
    refused(ERR_ARG, [F(ta), F(tb, states=0, styles=st, style_count=257)])
    refused(ERR_ARG, [F(ta, states=0, styles=st), F(tb, states=0, styles=st + st)])          # style counts differ
    refused(ERR_ARG, [F(ta, states=0, styles=st), F(tb, states=0, styles=[gsm.Style(opacity_scale=9)])])
    r.set_tile_rows(0, 1)
    refused(ERR_ARG, [F(ta), F(tb, styles=st)])                             # the styled row before the tile rows
    refused(ERR_UNSUPPORTED, [F(ta), F(tb)])
    refused(ERR_UNSUPPORTED, [F(ta, pick=None, occluder=None), F(tb, pick=None, occluder=None)])
    r.set_tile_rows(0, 0)
    # two frames that give the same table in two arrays: the call is accepted
    r.render_frames([F(ta, states=0, styles=st), F(tb, states=1, styles=[gsm.Style()])])
    cuda.cuda.synchronize()
    assert not ta.untouched() and not tb.untouched()

    # select_pick_ids: select_pick's rows in its order, without the last-pick rows
    state = cuda.full((600,), FILL, dtype=cuda.uint8, device="cuda")
    matched = cuda.full((1,), 0x5A5A, dtype=cuda.int32, device="cuda")
    mask = cuda.full((h, w), 1, dtype=cuda.uint8, device="cuda")

    def sel_refused(status, **kw):
        a = dict(pick=ta.pick, width=w, height=h, state=state, gaussian_count=600, pick_pitch=ta.pick_pitch, mask=None,
                 mask_pitch=w, matched=matched)
        a.update(kw)
        with pytest.raises(gsm.RendererError) as e:
            r.select_pick_ids(a["pick"], a["width"], a["height"], a["state"], a["gaussian_count"], 0, 1, mask=a["mask"],
                              matched=a["matched"], pick_pitch=a["pick_pitch"], mask_pitch=a["mask_pitch"])
        assert e.value.status == status, (status, kw)
        cuda.cuda.synchronize()
        assert (state.cpu().numpy() == FILL).all() and int(matched.item()) == 0x5A5A, kw

    sel_refused(ERR_COUNT, gaussian_count=5000, width=0)
    sel_refused(ERR_DIMS, width=0, pick=None)
    sel_refused(ERR_DIMS, height=h + 1, pick=None)
    sel_refused(ERR_MISSING, pick=None, pick_pitch=4)
    sel_refused(ERR_MISSING, state=None, pick_pitch=4)
    sel_refused(ERR_SIZE, pick_pitch=4 * w - 4)
    sel_refused(ERR_SIZE, pick_pitch=4 * w + 2)
    sel_refused(ERR_SIZE, mask=mask, mask_pitch=w - 1)
    sel_refused(ERR_SIZE, matched=int(matched.data_ptr()) + 2)
    # any size within the handle's is accepted (no "not the pick frame's" row), whatever the handle rendered last
    r.select_pick_ids(ta.pick, w - 1, h, state, 600, 0, 1, mask=mask, matched=matched, pick_pitch=ta.pick_pitch)
    cuda.cuda.synchronize()
    assert int(matched.item()) != 0x5A5A
    r.close()


# ---- 12. the C program ----
@pytest.mark.gpu
def test_c_program_renders_two_frames_and_selects_through_the_c_abi(gsm, cuda, tmp_path):
    from gsm_amd import scenes
    exe = os.path.join(HERE, "c", "frames_sequence")
    assert os.path.exists(exe), "tests/c/frames_sequence not built (__graft_entry__.build)"
    n, W, H, sh = 4096, 203, 77, 1
    world, harm, cam = scenes.gen_scene(n, W, H, sh, 0, seed=3)
    sc = Scene(cuda, world, harm, sh)
    with ref_frame([(sc.world_np, sc.harm_np, cam)], sh, W, H) as fr:
        deps = occluder_depths(fr, fr.walk(None))
    Z = float(deps[int(0.1 * len(deps))])  # (a near surface: it hides most of the scene)
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
    # the Python path: the same two frames on a handle of the same size
    specs = [Spec(sc, cam, W, H, occ=np.full((H, W), Z, np.float32), pad=0), Spec(sc, cam, W, H, depth=False, pad=0)]
    r = handle(gsm, 2 * 4096, 2 * W + 32, H, 0)
    want = batch_frames(gsm, cuda, r, specs)
    r.close()
    for v in range(2):
        color = np.frombuffer(raw[v * px * 12: v * px * 12 + px * 8], np.uint8).reshape(H, W * 8)
        pick = np.frombuffer(raw[v * px * 12 + px * 8: (v + 1) * px * 12], np.uint32).reshape(H, W)
        assert np.array_equal(color, want[v][0]) and np.array_equal(pick, want[v][2]), v
    state = np.frombuffer(raw[2 * px * 12: 2 * px * 12 + n], np.uint8)
    matched = int(np.frombuffer(raw[2 * px * 12 + n:], np.uint32)[0])
    wstate, m = select_ids_ref(want[1][2], None, np.zeros(n, np.uint8), n, 0xFF, 1)
    assert np.array_equal(state, wstate) and matched == m > 0
    assert not np.array_equal(want[0][2], want[1][2]), "the occluder of frame 0 changes its picks"
