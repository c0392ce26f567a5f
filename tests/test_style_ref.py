"""The styled frames' checker (tests/style/style_ref.c) on the CPU: with the identity it is the
oracle; hidden styles are the oracle on the compacted scene; its two integer formulas are the contract's; an opacity
scale of 0 empties the frame; a faded gaussian's tile count is count_range's on the styled byte.  The numpy
reference of gsm_global_select_mask is checked on hand-placed centres."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

NONE = 0xFFFFFFFF
INTERMEDIATES = ("render_data", "bounds", "mask", "tile_counts", "keys", "values", "sorted_keys", "sorted_values",
                 "headers", "color", "depth")


def _scene(n, w, h, sh, prec, seed, **kw):
    from gsm_amd import scenes
    world, harm, cam = scenes.gen_scene(n, w, h, sh, prec, seed=seed, **kw)
    return world, np.asarray(harm).reshape(-1), cam


def big_splat_scene(n, w, h, prec, seed, big=6):
    """gen_scene with `big` close, large gaussians whose tile rects exceed 32 tiles (the scatter's re-test)."""
    world, harm, cam = _scene(n, w, h, 1, prec, seed)
    val = (lambda v: np.float32(v)) if prec == 0 else (lambda v: np.float16(v).view(np.uint16))
    for i in range(big):
        world["pz"][i] = 0.8 + 0.1 * i
        world["px"][i] = -0.25 + 0.1 * i
        world["py"][i] = 0.1 - 0.04 * i
        for axis in ("sx", "sy", "sz"):
            world[axis][i] = val(0.06 + 0.01 * i)
        world["opacity"][i] = val(0.9)
    return world, harm, cam


@pytest.mark.parametrize("prec,sh", [(1, 16), (0, 1)])
def test_identity_table_is_the_oracle(oracle, prec, sh):
    import style_ref
    w, h = 203, 77
    world, harm, cam = _scene(3000, w, h, sh, prec, 5)
    ref = oracle.render(world, harm, sh, cam, w, h)
    rng = np.random.default_rng(1)
    # an identity table of three entries, states drawn from all 256 values: most are past the table
    table = style_ref.style_table([(9, 9, 9, 0, 255, 0)] * 3)
    for state in (rng.integers(0, 256, len(world)).astype(np.uint8), 7):
        got = style_ref.render(world, harm, sh, cam, w, h, state, table)
        assert got["status"] == 0 and got["differ"] == 0 and got["total_assignments"] == ref["total_assignments"] > 0
        for k in INTERMEDIATES:
            assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("prec", [0, 1])
def test_hidden_styles_are_the_compacted_scene(oracle, prec):
    import style_ref
    w, h, sh = 200, 120, 4
    world, harm, cam = _scene(2500, w, h, sh, prec, 6)
    n = len(world)
    rng = np.random.default_rng(2)
    state = rng.integers(0, 3, n).astype(np.uint8)
    table = style_ref.style_table([(0, 0, 0, 0, 255, 0), (1, 2, 3, 0, 255, 1), (0, 0, 0, 0, 255, 0)])
    got = style_ref.render(world, harm, sh, cam, w, h, state, table)
    keep = np.nonzero(state != 1)[0]
    ref = oracle.render(world[keep], harm.reshape(n, -1)[keep].reshape(-1), sh, cam, w, h, max_gaussians=n)
    assert got["differ"] == 0 and 0 < ref["total_assignments"] == got["total_assignments"]
    assert np.array_equal(got["color"], ref["color"]) and np.array_equal(got["depth"], ref["depth"])
    assert np.array_equal(got["sorted_keys"], ref["sorted_keys"])
    assert np.array_equal(got["sorted_values"], keep[ref["sorted_values"]]), "values map through the compaction"
    assert (got["mask"][state == 1] == 0).all() and (got["tile_counts"][state == 1] == 0).all()
    assert (got["bounds"][state == 1] == (0, -1, 0, -1)).all()
    pick = got["pick"]
    assert (pick != NONE).any() and not np.isin(pick[pick != NONE], np.nonzero(state == 1)[0]).any()


def test_integer_formulas_over_every_pair(oracle):
    import style_ref
    L = style_ref.lib()
    c = np.arange(256, dtype=np.int64)[:, None]
    k = np.arange(256, dtype=np.int64)[None, :]
    for t in (0, 1, 127, 128, 200, 254, 255):
        # independently: the nearest integer to (c (255 - k) + t k) / 255, halves up, in exact integers
        want = (2 * (c * (255 - k) + t * k) + 255) // 510
        got = np.array([[L.sr_tint(int(ci), t, int(ki)) for ki in range(256)] for ci in range(256)], np.int64)
        assert np.array_equal(got, want), t
        assert np.array_equal(got[:, 0], np.arange(256)) and (got[:, 255] == t).all()
    want = (2 * c * k + 255) // 510
    got = np.array([[L.sr_fade(int(o), int(s)) for s in range(256)] for o in range(256)], np.int64)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 255], np.arange(256)) and (got[:, 0] == 0).all()


def test_opacity_scale_zero_is_the_clear_frame(oracle):
    import style_ref
    w, h = 97, 45
    world, harm, cam = _scene(600, w, h, 1, 0, 8)
    got = style_ref.render(world, harm, 1, cam, w, h, 0, style_ref.style_table([(0, 0, 0, 0, 0, 0)]))
    ref = oracle.render(world, harm, 1, cam, w, h)
    assert got["total_assignments"] == 0 and got["differ"] == 0 and (got["pick"] == NONE).all()
    assert np.array_equal(got["mask"], ref["mask"]) and ref["mask"].any(), "o' == 0 leaves the gaussian visible"
    assert np.array_equal(got["bounds"], ref["bounds"])
    assert (got["color"][..., :3] == 0).all() and (got["color"][..., 3] == 0x3C00).all() and (got["depth"] == 0).all()


def test_a_faded_large_rect_counts_tiles_on_the_styled_byte(oracle):
    """A gaussian whose rect exceeds 32 tiles, faded: its count equals count_range's for a scene whose own opacity
    gives the same byte, and differs from the unfaded count (the level 2 computePower(o') moved)."""
    import style_ref
    w, h = 640, 360
    world, harm, cam = big_splat_scene(300, w, h, 0, 9)
    plain = oracle.render(world, harm, 1, cam, w, h)
    b = plain["bounds"][:6]
    area = (b[:, 1] - b[:, 0] + 1) * (b[:, 3] - b[:, 2] + 1)
    assert (area > 32).all(), "the test's premise: rects over 32 tiles"
    state = np.zeros(len(world), np.uint8)
    state[:6] = 1
    got = style_ref.render(world, harm, 1, cam, w, h, state,
                           style_ref.style_table([(0, 0, 0, 0, 255, 0), (0, 0, 0, 0, 20, 0)]))
    faded = (plain["render_data"]["opacity"][:6].astype(np.uint32) * 20 + 127) // 255
    assert np.array_equal(got["render_data"]["opacity"][:6], faded)
    # the same bytes from the scene's own opacity: (byte + 0.5) / 255 truncates back to the byte
    w2 = world.copy()
    w2["opacity"][:6] = ((faded + 0.5) / 255.0).astype(np.float32)
    ref = oracle.render(w2, harm, 1, cam, w, h)
    assert np.array_equal(ref["render_data"]["opacity"][:6], faded) and np.array_equal(ref["mask"][:6], got["mask"][:6])
    assert np.array_equal(got["tile_counts"][:6], ref["tile_counts"][:6])
    assert (got["tile_counts"][:6] != plain["tile_counts"][:6]).any()
    assert np.array_equal(got["tile_counts"][6:], plain["tile_counts"][6:])


def test_select_reference_on_hand_placed_centres():
    import style_ref
    from oracle import RENDER_DATA
    w, h = 8, 4
    xs = np.array([-0.5, -0.25, 0.0, 7.49, 7.5, 3.5, 3.25, np.inf, np.nan, 2.0], np.float16)
    rd = np.zeros(len(xs), RENDER_DATA)
    rd["meanX"] = xs.view(np.uint16)
    rd["meanY"] = np.float16(1.0).view(np.uint16)
    vis = np.ones(len(xs), np.uint8)
    vis[9] = 0
    mask = np.ones((h, w + 3), np.uint8)
    new, matched = style_ref.select_mask(rd, vis, w, h, mask, np.zeros(len(xs), np.uint8), 0, 5)
    # floor(x + 0.5): -0.5 -> 0, -0.25 -> 0, 7.49 -> 7, 7.5 -> 8 (outside), 3.5 -> 4, inf / NaN never, culled never
    assert new.tolist() == [5, 5, 5, 5, 0, 5, 5, 0, 0, 0] and matched == 6
    mask[:] = 0
    mask[1, 4] = 1
    new, matched = style_ref.select_mask(rd, vis, w, h, mask, np.full(len(xs), 2, np.uint8), 0xFF, 1)
    assert new.tolist() == [2, 2, 2, 2, 2, 3, 2, 2, 2, 2] and matched == 1
    hid = style_ref.style_table([(0, 0, 0, 0, 255, 0), (0, 0, 0, 0, 255, 0), (0, 0, 0, 0, 255, 1)])
    new, matched = style_ref.select_mask(rd, vis, w, h, mask, np.full(len(xs), 2, np.uint8), 0xFF, 1, styles=hid)
    assert matched == 0 and (new == 2).all()
