"""The HIP DepthFirst frames against the float64 model (tests/f64_df_model.py), through the C ABI.

The checks and constants of tests/test_f64_df_model.py applied to what the library returns: RENDER_DATA, BOUNDS,
TOUCHED, DEPTH_KEYS, DEPTH_ORDER, SORTED_DEPTH_KEYS, INSTANCE_TILES, INSTANCE_GAUSSIANS, HEADERS, the side-by-side
target of a stereo frame, colour and depth of a mono frame.  Neither the oracle nor a *_ref module is consulted,
so these stand even if a restatement is wrong or does not build.  One frame per scene: the smallest frames that
reach every DepthFirst kernel (both projections, both instance expansions, the depth and tile sorts with 32-bit
and 16-bit keys, both blends, the copy pass).
"""
import pytest

import test_f64_df_model as D
from test_depthfirst import gpu_df
from test_depthfirst_mono import gpu_mono

pytestmark = pytest.mark.gpu


def _renderer(gsm, c):
    """A renderer with the case's create options, and room for every instance (8 per gaussian)."""
    n = len(c["world"])
    prec = 1 if c["world"].dtype.itemsize == 32 else 0
    cfg = gsm.RendererConfig(max_gaussians=8 * n, max_width=c["width"], max_height=c["height"], precision=prec,
                             gaussian_color_space=c["color_space"])
    return gsm.DepthFirstRenderer(config=cfg, depth_key_bits=c["bits"][0], tile_id_bits=c["bits"][1])


@pytest.mark.parametrize("name", D.ALL)
def test_frame(gsm, cuda, name):
    c, pr = D.case_of(name), D.projection_of(name)
    w, h = c["width"], c["height"]
    rend = _renderer(gsm, c)
    if c["stereo"]:
        g = gpu_df(gsm, cuda, c["world"], c["harm"], c["sh"], c["cams"][0], c["cams"][1], w, h,
                   color_space=c["color_space"], scene_transform=c["transform"], renderer=rend)
    else:
        g = gpu_mono(gsm, cuda, c["world"], c["harm"], c["sh"], c["cam"], w, h, color_space=c["color_space"],
                     renderer=rend)
    g["sorted_keys"] = rend.copy_buffer(gsm.DepthFirstBuffer.SORTED_DEPTH_KEYS)
    assert g["counters"]["overflow"] == 0
    assert rend.options == {"depth_key_bits": c["bits"][0], "tile_id_bits": c["bits"][1]}
    rend.close()
    view = (D.stereo_view if c["stereo"] else D.mono_view)(g, w, h, c["bits"][0])
    D.check_all(name, pr, view)
