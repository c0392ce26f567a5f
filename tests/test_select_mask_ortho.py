"""gsm_global_select_mask_ortho against the select's contract written in numpy (tests/style_ref.py,
select_mask) over the orthographic checker's render data and visibility: every state byte, the guard bytes past the
count and the matched count, bit for bit -- the masks, operations and edge-centre cases of tests/test_select_mask.py,
with the centres placed by the orthographic projection."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_render_pick import Scene, handle  # noqa: E402
from test_render_styled import py_styles  # noqa: E402
from test_select_mask import GUARD, OPS, masks  # noqa: E402

ERR_COUNT, ERR_DIMS, ERR_SIZE, ERR_MISSING, ERR_ARG = 6, 7, 8, 13, 14


def edge_scene(torch, w, h, prec, seed, half_height=3.0):
    """gen_scene plus 48 gaussians whose centres sit a quarter pixel inside and outside each frame edge (screen x, y
    of -0.75, -0.5, -0.25 and their mirrors at the far edges) under scenes.ortho_camera: sx = ((x p00 + 1) W - 1) / 2
    whatever the depth, so the depths are spread over the cloud's."""
    from gsm_amd import scenes
    world, harm, _ = scenes.gen_scene(1200, w, h, 1, prec, seed=seed)
    cam = scenes.ortho_camera(w, h, half_height)
    P = cam["proj"]
    k = 0
    for axis, size, p in (("px", w, P[0]), ("py", h, P[5])):
        other, osize, op = ("py", h, P[5]) if axis == "px" else ("px", w, P[0])
        for s in (-0.75, -0.5, -0.25, size - 0.75, size - 0.5, size - 0.25):
            for frac in (0.2, 0.4, 0.6, 0.8):
                world[axis][k] = ((2 * s + 1) / size - 1) / p
                world[other][k] = ((2 * frac * osize + 1) / osize - 1) / op
                world["pz"][k] = 2.0 + 7.0 * frac
                k += 1
    return Scene(torch, world, harm, 1), cam, k


def run_select(gsm, torch, r, sc, cam, w, h, mask, state, a, x, styles=None, harm=True, ortho=True):
    dstate = torch.from_numpy(np.concatenate([state, np.full(GUARD, 0xC3, np.uint8)])).cuda()
    dmask = torch.from_numpy(mask).cuda()
    matched = torch.full((1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    inp = sc.input(gsm) if harm else gsm.GaussianInput(sc.world, None, sc.n, 0)
    r.select_mask(inp, gsm.CameraParams.from_dict(cam), w, h, dmask, dstate, a, x,
                  styles=None if styles is None else py_styles(gsm, styles), matched=matched,
                  mask_pitch=mask.shape[1], orthographic=ortho)
    torch.cuda.synchronize()
    out = dstate.cpu().numpy()
    assert (out[len(state):] == 0xC3).all(), "bytes past gaussian_count were written"
    return out[:len(state)], int(matched.item())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("w,h", [(97, 45), (200, 120)])
def test_ortho_select_matches_the_numpy_contract(gsm, cuda, prec, w, h):
    import ortho_ref
    import style_ref
    sc, cam, edge = edge_scene(cuda, w, h, prec, 90 + w)
    ref = ortho_ref.render(sc.world_np, sc.harm_np, 1, cam, w, h)
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
    # the two entries differ on this camera: the perspective select reads the same matrix by the perspective rule
    m = masks(w, h, 4)["full"]
    want, _ = style_ref.select_mask(rd, vis, w, h, m, state0, 0, 7)
    persp, _ = run_select(gsm, cuda, r, sc, cam, w, h, m, state0, 0, 7, ortho=False)
    assert not np.array_equal(persp, want)
    # hidden: states 2 and 5 are hidden styles -- skipped with the table, selected without it
    table = style_ref.style_table([(0, 0, 0, 0, 255, 0)] * 6)
    table["hidden"][[2, 5]] = 1
    st = rng.integers(0, 8, sc.n).astype(np.uint8)
    for styles in (table, None):
        want, nwant = style_ref.select_mask(rd, vis, w, h, m, st, 0, 7, styles=styles)
        got, ngot = run_select(gsm, cuda, r, sc, cam, w, h, m, st, 0, 7, styles=styles)
        assert np.array_equal(got, want) and ngot == nwant
    r.close()


@pytest.mark.gpu
def test_ortho_select_checks_are_the_selects(gsm, cuda):
    """The same refusals in the same order, and the count-0 no-op that writes *matched = 0."""
    from gsm_amd import scenes
    w, h = 97, 45
    cam = gsm.CameraParams.from_dict(scenes.ortho_camera(w, h, 3.0))
    r = handle(gsm, 512, w, h, 0)
    mask = cuda.ones((h, w), dtype=cuda.uint8, device="cuda")
    state = cuda.full((300,), 9, dtype=cuda.uint8, device="cuda")
    world = cuda.zeros((300 * 48,), dtype=cuda.uint8, device="cuda")
    matched = cuda.full((2,), 77, dtype=cuda.int32, device="cuda")
    r.select_mask(gsm.GaussianInput(None, None, 0, 0), cam, w, h, mask, None, 0, 1, matched=matched, orthographic=True)
    cuda.cuda.synchronize()
    assert matched.tolist() == [0, 77]
    inp = gsm.GaussianInput(world, None, 300, 0)

    def status(**kw):
        a = dict(input=inp, camera=cam, width=w, height=h, mask=mask, state=state, and_mask=0, xor_mask=1)
        a.update(kw)
        with pytest.raises(gsm.RendererError) as e:
            r.select_mask(a.pop("input"), a.pop("camera"), a.pop("width"), a.pop("height"), a.pop("mask"),
                          a.pop("state"), a.pop("and_mask"), a.pop("xor_mask"), orthographic=True, **a)
        return e.value.status

    assert status(input=gsm.GaussianInput(world, None, 513, 0), width=0) == ERR_COUNT
    assert status(width=w + 1, mask=None) == ERR_DIMS
    assert status(mask=None, mask_pitch=1) == ERR_MISSING
    assert status(state=None) == ERR_MISSING
    assert status(mask_pitch=w - 1, style_count=3) == ERR_SIZE
    assert status(style_count=3) == ERR_ARG
    cuda.cuda.synchronize()
    assert (state.cpu().numpy() == 9).all()
    r.close()
