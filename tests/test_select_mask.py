"""gsm_global_select_mask against its contract written in numpy (tests/style_ref.py, select_mask)
over the oracle's render data and visibility of the plain frame: every state byte, the guard bytes past the count and
the matched count, bit for bit; then the round trips select -> render_styled and select -> render_composite_styled
against the styled frames' checker on the numpy-selected state."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_render_pick import NONE, Scene, gen, handle, roundup256  # noqa: E402
from test_render_styled import check_styled, posed, py_styles, styled  # noqa: E402

ERR_COUNT, ERR_DIMS, ERR_SIZE, ERR_MISSING, ERR_ARG = 6, 7, 8, 13, 14
GUARD, PAD = 37, 5   # guard bytes after the state array; padding bytes per mask row (nonzero)


def masks(w, h, seed):
    """name -> (h, w + PAD) uint8 mask whose padding columns are nonzero"""
    rng = np.random.default_rng(seed)
    out = {}
    for name in ("rect", "brush", "full", "empty"):
        m = np.zeros((h, w + PAD), np.uint8)
        if name == "rect":
            m[h // 5:h // 2, w // 4:3 * w // 4] = 1
        elif name == "brush":
            m[:, :w] = (rng.random((h, w)) < 0.4) * rng.integers(1, 256, (h, w))
        elif name == "full":
            m[:, :w] = 255
        m[:, w:] = 0xEE
        out[name] = m
    return out


def edge_scene(torch, w, h, prec, seed):
    """gen_scene plus 48 gaussians whose centres sit a quarter pixel inside and outside each frame edge
    (screen x, y of -0.75, -0.5, -0.25 and their mirrors at the far edges; make_camera's projection)."""
    from gsm_amd import scenes
    world, harm, cam = scenes.gen_scene(1200, w, h, 1, prec, seed=seed)
    P = cam["proj"]
    z = 5.0
    k = 0
    for axis, size, p in (("px", w, P[0]), ("py", h, P[5])):
        other, osize, op = ("py", h, P[5]) if axis == "px" else ("px", w, P[0])
        for s in (-0.75, -0.5, -0.25, size - 0.75, size - 0.5, size - 0.25):
            for frac in (0.2, 0.4, 0.6, 0.8):
                world[axis][k] = ((2 * s + 1) / size - 1) * z / p
                world[other][k] = ((2 * frac * osize + 1) / osize - 1) * z / op
                world["pz"][k] = z
                k += 1
    return Scene(torch, world, harm, 1), cam, k


def run_select(gsm, torch, r, sc, cam, w, h, mask, state, a, x, styles=None, harm=True):
    """(new state with its guard bytes, matched) from the GPU"""
    dstate = torch.from_numpy(np.concatenate([state, np.full(GUARD, 0xC3, np.uint8)])).cuda()
    dmask = torch.from_numpy(mask).cuda()
    matched = torch.full((1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    inp = sc.input(gsm) if harm else gsm.GaussianInput(sc.world, None, sc.n, 0)
    r.select_mask(inp, gsm.CameraParams.from_dict(cam), w, h, dmask, dstate, a, x,
                  styles=None if styles is None else py_styles(gsm, styles), matched=matched,
                  mask_pitch=mask.shape[1])
    torch.cuda.synchronize()
    out = dstate.cpu().numpy()
    assert (out[len(state):] == 0xC3).all(), "bytes past gaussian_count were written"
    return out[:len(state)], int(matched.item())


def test_select_is_declared_exported_and_bound(gsm):
    import re
    import subprocess
    src = open(os.path.join(os.path.dirname(HERE), "include", "gsm_renderer.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"gsm_status\s+gsm_global_select_mask\s*\(", src)
    assert " T gsm_global_select_mask\n" in out and "gsm_global_select_mask" in gsm._SIGNATURES
    assert callable(getattr(gsm.GlobalRenderer, "select_mask", None))


OPS = {"set": (~0x40, 0x40), "clear": (~0x01, 0), "toggle": (0xFF, 0x02), "assign": (0, 0x9C)}


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("w,h", [(97, 45), (200, 120)])
def test_select_matches_the_numpy_contract(gsm, cuda, oracle, prec, w, h):
    """Four masks x four operations, centres on both sides of every frame edge, harmonics NULL; then the hidden
    skip with and without the table."""
    import style_ref
    sc, cam, edge = edge_scene(cuda, w, h, prec, 90 + w)
    ref = oracle.render(sc.world_np, sc.harm_np, 1, cam, w, h)
    rd, vis = ref["render_data"], ref["mask"]
    e_in = style_ref.select_mask(rd[:edge], vis[:edge], w, h, np.ones((h, w), np.uint8), np.zeros(edge, np.uint8),
                                 0, 1)[0]
    assert vis[:edge].all() and e_in.any() and not e_in.all(), "the premise: edge centres on both sides, all visible"
    rng = np.random.default_rng(w)
    state0 = rng.integers(0, 256, sc.n).astype(np.uint8)
    r = handle(gsm, sc.n, w, h, prec)
    for name, m in masks(w, h, 3).items():
        for op, (a, x) in OPS.items():
            want, nwant = style_ref.select_mask(rd, vis, w, h, m, state0, a, x)
            got, ngot = run_select(gsm, cuda, r, sc, cam, w, h, m, state0, a, x, harm=False)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, f"{name}/{op}: {len(bad)} states differ, first {bad[:5].tolist()}"
            assert ngot == nwant, (name, op)
        if name == "empty":
            assert nwant == 0 and np.array_equal(got, state0)
        if name == "full":
            assert nwant > sc.n // 4
    # hidden: states 2 and 5 are hidden styles -- skipped with the table, selected without it
    table = style_ref.style_table([(0, 0, 0, 0, 255, 0)] * 6)
    table["hidden"][[2, 5]] = 1
    st = rng.integers(0, 8, sc.n).astype(np.uint8)
    m = masks(w, h, 4)["full"]
    for styles in (table, None):
        want, nwant = style_ref.select_mask(rd, vis, w, h, m, st, 0, 7, styles=styles)
        got, ngot = run_select(gsm, cuda, r, sc, cam, w, h, m, st, 0, 7, styles=styles)
        assert np.array_equal(got, want) and ngot == nwant
    assert np.isin(want[(st == 2) | (st == 5)], 7).any(), "without the table hidden states are selectable"
    r.close()


@pytest.mark.gpu
def test_select_count_zero_and_refusals(gsm, cuda):
    from gsm_amd import scenes
    w, h = 97, 45
    sc = gen(cuda, 300, w, h, 1, 0, 95)
    cam = gsm.CameraParams.from_dict(scenes.make_camera(w, h))
    r = handle(gsm, 512, w, h, 0)
    mask = cuda.ones((h, w), dtype=cuda.uint8, device="cuda")
    state = cuda.full((300 + GUARD,), 9, dtype=cuda.uint8, device="cuda")
    matched = cuda.full((2,), 77, dtype=cuda.int32, device="cuda")
    r.select_mask(gsm.GaussianInput(None, None, 0, 0), cam, w, h, mask, None, 0, 1, matched=matched)
    cuda.cuda.synchronize()
    assert matched.tolist() == [0, 77]
    matched.fill_(77)

    def status(inp=None, ww=w, hh=h, m=mask, st=state, styles=None, mt=matched, **kw):
        try:
            r.select_mask(inp or sc.input(gsm), cam, ww, hh, m, st, 0, 1, styles=styles, matched=mt, **kw)
        except gsm.RendererError as e:
            return int(e.status)
        return 0

    good = [gsm.Style()]
    assert status(inp=gsm.GaussianInput(sc.world, None, 513, 0)) == ERR_COUNT
    assert status(ww=0) == ERR_DIMS and status(hh=h + 1) == ERR_DIMS
    assert status(m=None) == ERR_MISSING and status(st=None) == ERR_MISSING
    assert status(inp=gsm.GaussianInput(None, None, 300, 0)) == ERR_MISSING
    assert status(mask_pitch=w - 1) == ERR_SIZE and status(mt=int(matched.data_ptr()) + 2) == ERR_SIZE
    assert status(style_count=3) == ERR_ARG
    assert status(styles=good, style_count=0) == ERR_ARG and status(styles=good, style_count=257) == ERR_ARG
    # the order: count, dimensions, missing, size, argument
    assert status(inp=gsm.GaussianInput(sc.world, None, 513, 0), ww=0) == ERR_COUNT
    assert status(ww=0, m=None) == ERR_DIMS and status(m=None, mask_pitch=1) == ERR_MISSING
    assert status(mask_pitch=1, style_count=3) == ERR_SIZE
    cuda.cuda.synchronize()
    assert (state == 9).all().item() and matched.tolist() == [77, 77], "a refused call wrote"
    assert status() == 0 and status(mt=None) == 0
    cuda.cuda.synchronize()
    assert (state[300:] == 9).all().item() and matched[1].item() == 77 and 0 < matched[0].item() <= 300
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_round_trip_select_then_render_styled(gsm, cuda, oracle, prec):
    """A rectangle select on the device, then a styled frame from that state array: the frame is the checker's for
    the numpy-selected state."""
    import style_ref
    from gsm_amd import scenes
    w, h, sh = 200, 120, 4
    sc = gen(cuda, 3000, w, h, sh, prec, 96)
    cam = scenes.make_camera(w, h)
    ref = oracle.render(sc.world_np, sc.harm_np, sh, cam, w, h)
    m = masks(w, h, 5)["rect"]
    want, n = style_ref.select_mask(ref["render_data"], ref["mask"], w, h, m, np.zeros(sc.n, np.uint8), ~1, 1)
    assert 0 < n < sc.n
    table = style_ref.style_table([(0, 0, 0, 0, 90, 0), (255, 200, 0, 170, 255, 0)])   # fade the rest, highlight
    r = handle(gsm, sc.n, w, h, prec)
    state = cuda.zeros(sc.n, dtype=cuda.uint8, device="cuda")
    r.select_mask(sc.input(gsm), gsm.CameraParams.from_dict(cam), w, h, cuda.from_numpy(m).cuda(), state, ~1, 1,
                  mask_pitch=m.shape[1])
    c, d, p = styled(gsm, cuda, r, [(sc, cam)], w, h, [state], table)
    r.close()
    assert np.array_equal(state.cpu().numpy(), want)
    fr = style_ref.render(sc.world_np, sc.harm_np, sh, cam, w, h, want, table)
    assert fr["differ"] == 0
    assert np.array_equal(c, fr["color"].view(np.uint8).reshape(h, -1))
    assert np.array_equal(d, fr["depth"].view(np.uint8).reshape(h, -1)) and np.array_equal(p, fr["pick"])
    check_styled(gsm, cuda, [(sc, cam)], w, h, [want], table)


@pytest.mark.gpu
def test_round_trip_select_per_object_then_composite(gsm, cuda, oracle):
    """The select once per object with that object's camera, then the styled composite on those state arrays."""
    import style_ref
    from gsm_amd import scenes
    w, h = 200, 120
    counts = (700, 1000)
    scs = [gen(cuda, n, w, h, 1, 0, 97 + i) for i, n in enumerate(counts)]
    pairs = posed(scs, scenes.make_camera(w, h))
    m = masks(w, h, 6)["brush"]
    table = style_ref.style_table([(0, 0, 0, 0, 255, 0), (0, 255, 255, 200, 255, 0)])
    M_ = sum(roundup256(n) for n in counts)
    r = handle(gsm, M_, w, h, 0)
    dm = cuda.from_numpy(m).cuda()
    dev, want = [], []
    for sc, cam in pairs:
        ref = oracle.render(sc.world_np, sc.harm_np, 1, cam, w, h)
        wnt, n = style_ref.select_mask(ref["render_data"], ref["mask"], w, h, m, np.zeros(sc.n, np.uint8), 0, 1)
        assert 0 < n < sc.n
        st = cuda.zeros(sc.n, dtype=cuda.uint8, device="cuda")
        r.select_mask(sc.input(gsm), gsm.CameraParams.from_dict(cam), w, h, dm, st, 0, 1, mask_pitch=m.shape[1])
        dev.append(st)
        want.append(wnt)
    c, d, p = styled(gsm, cuda, r, pairs, w, h, dev, table, composite=True)
    r.close()
    for st, wnt in zip(dev, want):
        assert np.array_equal(st.cpu().numpy(), wnt)
    fr = style_ref.render_composite([(s.world_np, s.harm_np, cm, wn) for (s, cm), wn in zip(pairs, want)], 1, w, h,
                                    table, max_gaussians=M_)
    assert fr["differ"] == 0
    assert np.array_equal(c, fr["color"].view(np.uint8).reshape(h, -1))
    assert np.array_equal(d, fr["depth"].view(np.uint8).reshape(h, -1))
    assert (p != NONE).any()
