"""Every kind of Global frame on ONE handle, one after another, twice over.

Twelve frames -- plain, render_views, render_batch, composite, pick, occluded, styled, styled with a pick target,
composite_pick, composite_occluded, composite_styled, plain -- run in that order on one handle, then all twelve
again, so that every frame of the second round meets the schedule its own kind left in the first.  Each frame's
colour, depth and pick bytes and its debug counters must equal, bit for bit, those of the same call on a fresh handle
(no tolerance); after composite_pick, pick_owner of three picked pixels must equal the fresh handle's too.  This
guards the kind tag that runFrame, launch_scatter and launch_blend dispatch on.

Scenes: ~600 gaussians each from the fixture generator, SH degree 1, fp16 input, three where the entry takes several
(a composite's second object is empty).  Every frame is at most 96 x 48 (3 x 3 tiles) and the handle holds 4096
gaussians.  The handle's own size is 192 x 48: a batch's views lie one after another in the handle's tile space, and
the batch of 96 x 48, 64 x 32 and 33 x 17 (9 + 4 + 4 tiles) needs 17 tiles, which a 96 x 48 handle (9 tiles) refuses
with GSM_ERR_INVALID_TILE_COUNT; 6 x 3 = 18 tiles is the smallest handle of the frames' three tile rows that holds it.
For the same reason the three render_views cameras are 64 x 48 each (3 x 6 = 18 tiles).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_render_pick import FILL, NONE, Targets, gen, handle  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 96, 48
MAX_W, MAX_H, MAX_G = 192, 48, 4096
VW, VH = 64, 48                                   # render_views: 3 cameras of this size
BATCH_SIZES = [(96, 48), (64, 32), (33, 17)]
SH, PREC = 4, 1                                   # SH degree 1, fp16 input
COUNTS = (600, 611, 593)


class Setup:
    """The scenes, cameras, states, styles and the occluder all 12 frames draw from (built once, never changed)."""

    def __init__(self, gsm, torch):
        from gsm_amd import scenes
        self.gsm, self.torch = gsm, torch
        self.scenes = [gen(torch, n, W, H, SH, PREC, seed=11 + i) for i, n in enumerate(COUNTS)]
        cam = lambda w, h, a: gsm.CameraParams.from_dict(scenes.orbit_camera(w, h, a))  # noqa: E731
        self.cam = cam(W, H, 0.0)
        self.view_cams = [cam(VW, VH, a) for a in (-12.0, 0.0, 9.0)]
        self.batch_cams = [cam(w, h, a) for (w, h), a in zip(BATCH_SIZES, (5.0, -7.0, 15.0))]
        self.obj_cams = [cam(W, H, a) for a in (0.0, 20.0, -14.0)]
        empty = gsm.GaussianInput(None, None, 0, SH)
        self.objects = [gsm.SceneObject(self.scenes[0].input(gsm), self.obj_cams[0]),
                        gsm.SceneObject(empty, self.obj_cams[1]),
                        gsm.SceneObject(self.scenes[2].input(gsm), self.obj_cams[2])]
        rng = np.random.default_rng(5)
        self.styles = [gsm.Style(), gsm.Style((255, 40, 0), 200, 255, False), gsm.Style((0, 0, 0), 0, 90, False),
                       gsm.Style((0, 0, 0), 0, 255, True)]
        self.state = torch.from_numpy(rng.integers(0, 4, COUNTS[0]).astype(np.uint8)).cuda()
        self.obj_states = [self.state, 1, torch.from_numpy(rng.integers(0, 4, COUNTS[2]).astype(np.uint8)).cuda()]
        occ = np.full((H, W), 5.0, np.float32)
        occ[:, : W // 3] = np.inf   # nothing occluded on the left third
        occ[H // 2:, W // 2:] = 2.5
        self.occluder = torch.from_numpy(occ).cuda()

    # ---- the frames: each fills fresh sentinel targets on handle r and returns their bytes ----
    def _single(self, call, pick):
        t = Targets(self.torch, W, H)
        call(t)
        return t.read(with_pick=pick)[: 3 if pick else 2]

    def plain(self, r):
        return self._single(lambda t: r.render(t.color, t.depth, self.scenes[0].input(self.gsm), self.cam, W, H), False)

    def views(self, r):
        n = len(self.view_cams)
        color = self.torch.full((n * VH + 3, VW * 8), FILL, dtype=self.torch.uint8, device="cuda")
        depth = self.torch.full((n * VH + 3, VW * 2), FILL, dtype=self.torch.uint8, device="cuda")
        r.render_views(color, depth, self.scenes[1].input(self.gsm), self.view_cams, VW, VH)
        self.torch.cuda.synchronize()
        return color.cpu().numpy(), depth.cpu().numpy()

    def batch(self, r):
        ts = [Targets(self.torch, w, h) for w, h in BATCH_SIZES]
        r.render_batch([self.gsm.BatchView(sc.input(self.gsm), c, w, h, t.color, t.depth)
                        for sc, c, (w, h), t in zip(self.scenes, self.batch_cams, BATCH_SIZES, ts)])
        return tuple(a for t in ts for a in t.read(with_pick=False)[:2])

    def composite(self, r):
        return self._single(lambda t: r.render_composite(t.color, t.depth, self.objects, W, H), False)

    def pick(self, r):
        return self._single(lambda t: r.render_pick(t.color, t.depth, t.pick, self.scenes[0].input(self.gsm), self.cam,
                                                    W, H, pick_pitch=t.pick_pitch), True)

    def occluded(self, r):
        return self._single(lambda t: r.render_occluded(t.color, t.depth, self.occluder,
                                                        self.scenes[0].input(self.gsm), self.cam, W, H), False)

    def styled(self, r):
        return self._single(lambda t: r.render_styled(t.color, t.depth, None, self.scenes[0].input(self.gsm), self.cam,
                                                      W, H, self.state, self.styles), False)

    def styled_pick(self, r):
        return self._single(lambda t: r.render_styled(t.color, t.depth, t.pick, self.scenes[0].input(self.gsm),
                                                      self.cam, W, H, self.state, self.styles,
                                                      pick_pitch=t.pick_pitch), True)

    def composite_pick(self, r):
        c, d, p = self._single(lambda t: r.render_composite_pick(t.color, t.depth, t.pick, self.objects, W, H,
                                                                 pick_pitch=t.pick_pitch), True)
        # pick_owner of three picked pixels (the first, the middle and the last pixel that picked a gaussian)
        hit = np.flatnonzero(p.reshape(-1) != NONE)
        assert len(hit) >= 3, "the composite picked fewer than three pixels"
        items = p.reshape(-1)[hit[[0, len(hit) // 2, -1]]]
        obj, gid = r.pick_owner(items)
        assert (obj != NONE).all() and (gid != NONE).all()
        return c, d, p, obj, gid

    def composite_occluded(self, r):
        return self._single(lambda t: r.render_composite_occluded(t.color, t.depth, self.occluder, self.objects, W, H),
                            False)

    def composite_styled(self, r):
        return self._single(lambda t: r.render_composite_styled(t.color, t.depth, None, self.objects, W, H,
                                                                self.obj_states, self.styles), False)

    def sequence(self):
        return [self.plain, self.views, self.batch, self.composite, self.pick, self.occluded, self.styled,
                self.styled_pick, self.composite_pick, self.composite_occluded, self.composite_styled, self.plain]


def new_handle(gsm):
    return handle(gsm, MAX_G, MAX_W, MAX_H, PREC)


def test_every_frame_kind_on_one_handle_equals_a_fresh_handle(gsm, cuda):
    S = Setup(gsm, cuda)
    frames = S.sequence()
    assert len(frames) == 12
    # the same call on a fresh handle, once per frame: the reference both rounds are held to
    fresh = []
    for f in frames:
        r = new_handle(gsm)
        out = f(r)
        fresh.append((out, r.counters()))
        r.close()
    r = new_handle(gsm)
    for rnd in range(2):
        for i, (f, (want, want_counters)) in enumerate(zip(frames, fresh)):
            what = f"round {rnd + 1}, frame {i + 1} ({f.__name__})"
            got = f(r)
            assert len(got) == len(want), what
            for k, (a, b) in enumerate(zip(got, want)):
                assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: output {k} differs from a fresh handle's"
            assert r.counters() == want_counters, f"{what}: debug counters"
    r.close()
    # the frames are not trivially equal: something was drawn, picked, occluded and styled
    plain, occl, styl = fresh[0][0], fresh[5][0], fresh[6][0]
    assert fresh[0][1]["total_assignments"] > 0 and plain[0].any()
    assert not np.array_equal(plain[0], occl[0]) and not np.array_equal(plain[0], styl[0])
    assert not np.array_equal(fresh[3][0][0], fresh[9][0][0]) and not np.array_equal(fresh[3][0][0], fresh[10][0][0])
    assert (fresh[4][0][2] != NONE).any() and (fresh[7][0][2] != NONE).any()
