"""CPU tests of gsm_global_render_frame's checker (tests/frame/frame_ref.c) and of the numpy restatement of
gsm_global_select_pick: with no occluder the one walk is pick_ref's / style_ref's, with an occluder its colour and
depth are occlude_ref's, and the select's set rule holds on hand-made pick images."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

NONE = 0xFFFFFFFF


def _scene(n, w, h, sh, prec, seed, **kw):
    sys.path.insert(0, os.path.join(HERE, "..", "gsm-renderer_amd"))
    from gsm_amd import scenes
    return scenes.gen_scene(n, w, h, sh, prec, seed=seed, **kw)


@pytest.mark.parametrize("prec,sh", [(1, 16), (0, 1)])
def test_without_an_occluder_the_walk_is_pick_refs(oracle, prec, sh):
    import frame_ref
    import pick_ref
    w, h = 203, 77
    world, harm, cam = _scene(4096, w, h, sh, prec, 3)
    want = pick_ref.render(world, harm, sh, cam, w, h)
    assert want["status"] == 0 and want["differ"] == 0
    with frame_ref.frame([(world, harm, cam)], sh, w, h) as fr:
        got = fr.walk(None)
        inf = fr.walk(np.full((h, w), np.inf, np.float32))
    for k in ("color", "depth", "pick"):
        assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(inf[k], want[k]), k + " under an occluder of all +inf"
    assert np.array_equal(got["items"], want["pick"]) and not got["closed"].any()
    assert (got["pick"] != NONE).any() and (got["pick"] == NONE).any()


def test_without_an_occluder_the_styled_walk_is_style_refs(oracle):
    import frame_ref
    import style_ref
    w, h, sh = 160, 90, 4
    a, ha, cam = _scene(1500, w, h, sh, 1, 5)
    b, hb, _ = _scene(700, w, h, sh, 1, 6)
    rng = np.random.default_rng(2)
    objs = [(a, ha, cam, rng.integers(0, 4, len(a)).astype(np.uint8)), (b, hb, cam, 1)]
    styles = style_ref.style_table([(0, 0, 0, 0, 255, 0), (255, 40, 0, 200, 255, 0), (0, 0, 0, 0, 90, 0),
                                    (0, 0, 0, 0, 255, 1)])
    want = style_ref.render_composite(objs, sh, w, h, styles)
    assert want["status"] == 0 and want["differ"] == 0
    with frame_ref.frame(objs, sh, w, h, styles=styles) as fr:
        got = fr.walk(None)
    for k in ("color", "depth", "pick"):
        assert np.array_equal(got[k], want[k]), k
    # the composite layout: object 1's items start at the next multiple of 256 past object 0's count
    hit1 = (want["pick"] != NONE) & (want["pick"] >= 1500)
    assert hit1.any() and np.array_equal(got["items"][hit1], want["pick"][hit1] - 1500 + 1536)


@pytest.mark.parametrize("prec,sh", [(1, 16), (0, 1)])
def test_without_a_pick_the_occluded_walk_is_occlude_refs(oracle, prec, sh):
    import frame_ref
    import occlude_ref
    from test_render_occluded import random_occluder, ramp_occluder, visible_depths
    w, h = 203, 77
    world, harm, cam = _scene(4096, w, h, sh, prec, 3)
    with occlude_ref.frame(world, harm, sh, cam, w, h) as of, frame_ref.frame([(world, harm, cam)], sh, w, h) as fr:
        deps = visible_depths(of.base)
        free = fr.walk(None)
        for name, occ in (("random", random_occluder(deps, w, h, 7)), ("ramp", ramp_occluder(deps, w, h))):
            want, got = of.occlude(occ), fr.walk(occ)
            assert np.array_equal(got["color"], want["color"]) and np.array_equal(got["depth"], want["depth"]), name
            assert int(got["closed"].sum()) == want["closed_pixels"] > 0, name
            # the pick under the occluder: never an item behind the pixel's surface, never on a closed-at-once pixel
            dep = got["records"][:, 9].view(np.float16).astype(np.float32)
            hit = got["pick"] != NONE
            with np.errstate(invalid="ignore", over="ignore"):
                z = occ.astype(np.float16).astype(np.float32)
                assert not (dep[got["pick"][hit]] > z[hit]).any(), name
            assert (got["pick"] != free["pick"]).any(), name
            assert (got["closed"] & (got["pick"] == NONE) & (free["pick"] != NONE)).any(), name


def test_select_pick_rule_on_hand_made_images():
    import frame_ref
    # two objects: object 0 has 300 gaussians (items 0..299, blocks 0-1), object 1 has 10 (items 512..521)
    img = np.full((4, 6), NONE, np.uint32)
    img[0, 0:3] = 7            # one item on several pixels
    img[1, 1] = 7
    img[1, 2] = 299
    img[2, 0] = 512            # object 1, id 0
    img[2, 1:4] = 515          # object 1, id 3, three pixels
    img[3, 5] = 521            # object 1, id 9
    img[3, 0] = 305            # a padding item of object 0's last block: owned by nobody
    state0 = np.arange(300, dtype=np.uint8)
    # toggle bit 0 on everything: an id on four pixels toggles once
    out, m = frame_ref.select_pick(img, None, 0, 300, state0, 300, 0xFF, 1)
    assert m == 2 and out[7] == (7 ^ 1) and out[299] == ((299 & 0xFF) ^ 1)
    assert np.array_equal(np.delete(out, [7, 299]), np.delete(state0, [7, 299]))
    # an item past gaussian_count is not selected
    out, m = frame_ref.select_pick(img, None, 0, 300, state0, 299, 0, 200)
    assert m == 1 and out[7] == 200 and out[299] == state0[299]
    # object 1 under a brush mask that covers row 2 only
    mask = np.zeros((4, 8), np.uint8)
    mask[2, :] = 255
    state1 = np.full(10, 0x10, np.uint8)
    out, m = frame_ref.select_pick(img, mask, 512, 10, state1, 10, ~2, 2)
    assert m == 2 and out.tolist() == [0x12, 0x10, 0x10, 0x12] + [0x10] * 6
    out, m = frame_ref.select_pick(img, None, 512, 10, state1, 10, ~0x10, 0)
    assert m == 3 and out.tolist() == [0, 0x10, 0x10, 0, 0x10, 0x10, 0x10, 0x10, 0x10, 0]
    # nothing of object 0 under that mask, a count of 0, and GSM_PICK_NONE with base 0
    assert frame_ref.select_pick(img, mask, 0, 300, state0, 300, 0, 1)[1] == 0
    assert frame_ref.select_pick(img, None, 0, 300, state0, 0, 0, 1)[1] == 0
    assert frame_ref.select_pick(np.full((2, 2), NONE, np.uint32), None, 0, 300, state0, 300, 0, 1)[1] == 0
