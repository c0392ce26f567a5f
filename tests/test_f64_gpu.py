"""The HIP path against the float64 model (tests/f64_model.py), through the C ABI.

The checks and constants of tests/test_f64_model.py applied to what the library returns: RENDER_DATA,
BOUNDS, HEADERS, SORTED_VALUES, colour and depth of a Global frame; PROJECTED, TILE_COUNTS, TILE_LISTS, colour
and depth of a Local frame.  The oracle is not consulted, so these stand even if it is wrong or does not
build.  Frames: the smallest at which each Global blend kernel runs (asserted), and the Local frame.
"""

import numpy as np
import pytest

import f64_model as M
import test_f64_model as T
from test_gpu_parity import gpu_render
from test_local import gpu_local

pytestmark = pytest.mark.gpu

QUADRANT, HALF_TILE, PAIR_WALK = 1, 2, 3  # gsm_blend_kernel (include/gsm_debug.h)


def _global_view(g):
    b = g["bounds"]
    mask = (b[:, 0] <= b[:, 1]) & (b[:, 2] <= b[:, 3])
    return T.global_view(g["render_data"], mask, g["headers"], g["sorted_values"], g["color"], g["depth"])


@pytest.mark.parametrize("name", ["sparse_sh1_f16_200x150", "sparse_sh3_f16_rolled_200x150", "dense_sh0_f32_128x64",
                                  "dense_sh1_f16_200x150", "plane_ties_128x64", "opaque_splat_64x64"])
def test_quadrant_frames(gsm, cuda, name):
    """200x150 and smaller (quadrant units): every check, the whole frame included where the CPU test has it."""
    c, pr = T.case_of(name), T.projection_of(name)
    w, h = c["width"], c["height"]
    g = gpu_render(gsm, cuda, c, keep=False)
    assert g["renderer"].blend_kernel_kind() == QUADRANT
    v = _global_view(g)
    g["renderer"].close()
    T.check_visibility(pr, v["mask"])
    T.check_records(pr, v, w, h)
    T.check_order(pr, v)
    T.check_blend("lists", T.measure_lists(v, w, h), v)
    if name in T.FRAME_SCENES:
        T.check_blend("frame", T.measure_frame(pr, v, w, h), v)


def _sample(lists, k):
    """Every k-th active tile plus the 32 deepest."""
    by_depth = sorted(range(len(lists)), key=lambda i: -len(lists[i][1]))[:32]
    return [lists[i] for i in sorted(set(range(0, len(lists), k)) | set(by_depth))]


@pytest.mark.parametrize("w,h,n,env,kind", [(1600, 656, 5000, {}, HALF_TILE),
                                            (1920, 1080, 6000, {"GSM_BLEND_WAVES": "16"}, PAIR_WALK)])
def test_large_frames(gsm, cuda, monkeypatch, w, h, n, env, kind):
    """The half-tile and the pair-walk kernels: visibility, records and order of the whole frame, compositing
    on a fixed sample of the active tiles."""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    c = T.make_case(("gen", n, w, h, 4, 1, 0, 21, None, {}))
    pr = M.project(c["world"], c["harm"], c["sh"], c["cam"], w, h, 0)
    g = gpu_render(gsm, cuda, c, keep=False)
    assert g["renderer"].blend_kernel_kind() == kind
    v = _global_view(g)
    g["renderer"].close()
    T.check_visibility(pr, v["mask"])
    T.check_records(pr, v, w, h)
    T.check_order(pr, v)
    T.check_blend("lists", T.measure_lists(v, w, h, lists=_sample(v["lists"], 16)), v)


@pytest.mark.parametrize("name", sorted(T.LOCAL_SCENES))
def test_local_frame(gsm, cuda, name):
    c, pr = T.case_of(name), T.projection_of(name)
    w, h = c["width"], c["height"]
    g = gpu_local(gsm, cuda, c["world"], c["harm"], c["sh"], c["cam"], w, h, color_space=c["color_space"])
    g["renderer"].close()
    # the compacted records keep gaussian order; which gaussian each belongs to follows from the model's
    # visible set when no gaussian of the scene is in doubt
    assert not T.left_out(pr).any()
    source = np.nonzero(pr["visible"])[0]
    assert g["counters"]["visible"] == len(source) == len(g["projected"])
    v = T.local_view(g["projected"], source, pr["visible"], g["tile_counts"], g["tile_lists"], g["color"], g["depth"])
    T.check_records(pr, v, w, h)
    T.check_order(pr, v)
    T.check_blend("lists", T.measure_lists(v, w, h), v)
    T.check_blend("frame", T.measure_frame(pr, v, w, h), v)
