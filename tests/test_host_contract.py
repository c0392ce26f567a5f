"""The host plumbing the Global, DepthFirst and Local renderers share (csrc/gsm_host.h), through the
Python API over the C ABI: the status a refused frame gets and the precedence among them, and the
stage-event ring behind set_profiling / stage_times_ms / last_gpu_time.

The pixel and intermediate tests pin what a frame computes; this file pins what they do not: which
error wins when several apply, the colour pitch of the side-by-side target, and the profiling
window (lazy start, restart on set_profiling, blend-only sampling, the wrap of the ring).  No number
here is a tolerance: times are only checked for presence and sign.
"""
import ctypes
import functools
import math

import pytest

from test_gpu_parity import to_dev

N, W, H, MAX_G = 64, 32, 32, 256
BPP = 8  # the default colour format, rgba16f

# frame: (renderer class, stage names, frames the event ring holds, depth target, empty frame allowed)
FRAMES = {
    "global": ("GlobalRenderer", "STAGES", 128, True, True),
    "df_stereo": ("DepthFirstRenderer", "DF_STAGES", 64, False, True),
    "df_mono": ("DepthFirstRenderer", "DF_STAGES", 64, True, False),
    "local": ("LocalRenderer", "LOCAL_STAGES", 64, True, False),
}
BLEND_ONLY = ("global", "df_stereo", "df_mono")  # Local has the every-stage mode only


@functools.lru_cache(maxsize=None)
def _scene():
    """(world, harmonics, left camera, right camera): computed once, shared, never modified."""
    from gsm_amd import scenes
    world, harm, _ = scenes.gen_scene(N, W, H, 1, 1, seed=7)
    return world, harm, scenes.make_camera(W, H, -0.032), scenes.make_camera(W, H, 0.032)


class Frame:
    """One renderer of `kind` with its targets; render() takes the arguments the cases vary."""

    def __init__(self, gsm, torch, kind):
        cls, stages, self.ring, self.has_depth, self.allow_empty = FRAMES[kind]
        self.gsm, self.kind = gsm, kind
        self.stages = getattr(gsm, stages)
        self.eyes = 2 if kind == "df_stereo" else 1  # the side-by-side target holds two frames a row
        self.renderer = getattr(gsm, cls)(config=gsm.RendererConfig(max_gaussians=MAX_G, max_width=W, max_height=H))
        world, harm, left, right = _scene()
        self.world, self.harm = to_dev(torch, world), to_dev(torch, harm)
        self.left, self.right = gsm.CameraParams.from_dict(left), gsm.CameraParams.from_dict(right)
        # (every target two frames and a spare column wide: each pitch the cases accept stays inside it)
        self.color = torch.zeros((H, 2 * W + 1, 4), dtype=torch.float16, device="cuda")
        self.depth = torch.zeros((H, W + 1), dtype=torch.float16, device="cuda")
        self.pitch = self.eyes * W * BPP

    NO_ARG = object()

    def render(self, count=N, width=W, height=H, color=NO_ARG, gaussians=NO_ARG, color_pitch=None,
               depth_pitch=None):
        g = self.gsm
        color = self.color if color is Frame.NO_ARG else color
        inp = g.GaussianInput(self.world if gaussians is Frame.NO_ARG else gaussians, self.harm, count, 1)
        cp = self.pitch + BPP if color_pitch is None else color_pitch
        dp = (W + 1) * 2 if depth_pitch is None else depth_pitch
        r = self.renderer
        if self.kind == "df_stereo":
            r.render_stereo_sbs(color, inp, self.left, self.right, width, height, color_pitch=cp)
        else:
            r.render(color, self.depth, inp, self.left, width, height, color_pitch=cp, depth_pitch=dp)

    def status(self, **kw):
        try:
            self.render(**kw)
        except self.gsm.RendererError as e:
            return e.status
        return self.gsm.Status.OK

    def frames(self, torch, n):
        for _ in range(n):
            self.render()
        torch.cuda.synchronize()

    def blend_only(self, period=1):
        self.renderer.set_profiling(stage_events=False, blend_events=True, blend_event_period=period)


ALL = pytest.mark.parametrize("frame", sorted(FRAMES), indirect=True)
WITH_DEPTH = pytest.mark.parametrize("frame", sorted(k for k, v in FRAMES.items() if v[3]), indirect=True)
WITH_BLEND_ONLY = pytest.mark.parametrize("frame", sorted(BLEND_ONLY), indirect=True)


@pytest.fixture
def frame(request, gsm, cuda):
    f = Frame(gsm, cuda, request.param)
    yield f
    f.renderer.close()


@pytest.mark.gpu
@ALL
def test_status_precedence(frame):
    S = frame.gsm.Status
    # count, then dimensions, then a missing buffer, then the buffer sizes
    assert frame.status(count=MAX_G + 1, width=0, color=None) == S.INVALID_GAUSSIAN_COUNT
    assert frame.status(width=0, color=None) == S.INVALID_DIMENSIONS
    assert frame.status(width=W + 1, color=None) == S.INVALID_DIMENSIONS
    assert frame.status(height=0, color=None) == S.INVALID_DIMENSIONS
    assert frame.status(color=None, color_pitch=4) == S.MISSING_REQUIRED_BUFFER
    assert frame.status(gaussians=None, color_pitch=4) == S.MISSING_REQUIRED_BUFFER
    assert frame.status(color_pitch=frame.pitch - 4) == S.INVALID_BUFFER_SIZE
    assert frame.status(color_pitch=frame.pitch + 2) == S.INVALID_BUFFER_SIZE  # not a multiple of 4
    assert frame.status(color_pitch=frame.pitch) == S.OK
    assert frame.status() == S.OK


@pytest.mark.gpu
@ALL
def test_side_by_side_pitch_is_two_frames_wide(frame):
    """width * bpp holds one eye: enough for every mono frame, short for the side-by-side target."""
    S = frame.gsm.Status
    expect = S.INVALID_BUFFER_SIZE if frame.kind == "df_stereo" else S.OK
    assert frame.status(color_pitch=W * BPP) == expect
    assert frame.status(color_pitch=2 * W * BPP) == S.OK


@pytest.mark.gpu
@WITH_DEPTH
def test_depth_pitch(frame):  # (the side-by-side frame has no depth target)
    S = frame.gsm.Status
    assert frame.status(depth_pitch=W * 2 + 1) == S.INVALID_BUFFER_SIZE  # odd
    assert frame.status(depth_pitch=W * 2 - 2) == S.INVALID_BUFFER_SIZE  # short
    assert frame.status(depth_pitch=W * 2) == S.OK
    # the count and the dimensions still come first
    assert frame.status(count=MAX_G + 1, depth_pitch=1) == S.INVALID_GAUSSIAN_COUNT
    assert frame.status(width=0, depth_pitch=1) == S.INVALID_DIMENSIONS


@pytest.mark.gpu
@ALL
def test_empty_frame(frame):
    S = frame.gsm.Status
    assert frame.status(count=0) == (S.OK if frame.allow_empty else S.INVALID_GAUSSIAN_COUNT)


def _assert_no_times(frame):
    with pytest.raises(frame.gsm.RendererError):
        frame.renderer.stage_times_ms()
    assert frame.renderer.last_gpu_time is None


def _assert_every_stage(frame):
    t = frame.renderer.stage_times_ms()
    assert tuple(t) == tuple(frame.stages)
    for k, v in t.items():
        assert math.isfinite(v) and v >= 0.0, (k, v)
    assert frame.renderer.last_gpu_time > 0


def _assert_blend_only(frame):
    t = frame.renderer.stage_times_ms()
    assert tuple(t) == tuple(frame.stages)
    for k, v in t.items():
        if k == "blend":
            assert math.isfinite(v) and v >= 0.0, v
        else:
            assert v == 0.0, (k, v)
    assert frame.renderer.last_gpu_time is None


@pytest.mark.gpu
@ALL
def test_every_stage_profiling(frame, cuda):
    _assert_no_times(frame)
    frame.frames(cuda, 1)  # an unprofiled frame leaves no times
    _assert_no_times(frame)
    frame.renderer.set_profiling(True)
    _assert_no_times(frame)
    frame.frames(cuda, 3)
    _assert_every_stage(frame)
    frame.renderer.set_profiling(True)  # the window restarts
    _assert_no_times(frame)
    frame.frames(cuda, 1)
    _assert_every_stage(frame)
    frame.renderer.set_profiling(False)
    _assert_no_times(frame)
    frame.frames(cuda, 1)
    _assert_no_times(frame)


@pytest.mark.gpu
@WITH_BLEND_ONLY
def test_blend_only_profiling(frame, cuda):
    frame.blend_only()
    _assert_no_times(frame)
    frame.frames(cuda, 3)
    _assert_blend_only(frame)
    frame.blend_only(period=4)  # frames 0 and 4 of the 8 are bracketed
    _assert_no_times(frame)
    frame.frames(cuda, 8)
    _assert_blend_only(frame)
    frame.blend_only(period=4)
    frame.frames(cuda, 1)  # the first frame after set_profiling is a sampled one
    _assert_blend_only(frame)
    frame.renderer.set_profiling(True)  # from blend-only to every stage on the same events
    _assert_no_times(frame)
    frame.frames(cuda, 2)
    _assert_every_stage(frame)


@pytest.mark.gpu
@ALL
def test_event_ring_wraps(frame, cuda):
    frame.renderer.set_profiling(True)
    frame.frames(cuda, frame.ring + 2)
    _assert_every_stage(frame)
    if frame.kind in BLEND_ONLY:
        frame.blend_only()
        frame.frames(cuda, frame.ring + 2)
        _assert_blend_only(frame)


@pytest.mark.gpu
def test_local_any_profiling_flag_is_every_stage(gsm, cuda):
    f = Frame(gsm, cuda, "local")
    assert gsm._lib().gsm_local_set_profiling(f.renderer._h, ctypes.c_int(2)) == 0
    _assert_no_times(f)
    f.frames(cuda, 3)
    _assert_every_stage(f)
    f.renderer.close()
