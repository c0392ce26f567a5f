"""The HIP path's orthographic frames and its orthographic select against the float64 model of the rule
(tests/f64_ortho_model.py), through the C ABI.

The checks and constants of tests/test_f64_ortho_model.py applied to what the library returns: colour, depth and
pick targets, RENDER_DATA, BOUNDS, HEADERS and SORTED_VALUES of render_frame(orthographic=True) and the state bytes
of select_mask(orthographic=True).  No checker and no oracle is consulted.  One case has proj[10] < 0 (sigma = -1).
"""
import numpy as np
import pytest

import f64_model as M
import test_f64_features_model as F
import test_f64_model as T
import test_f64_ortho_model as X
from test_f64_features_gpu import QUADRANT, _captured_view, _dev_states, _handle_for, _objects, _styles
from test_render_pick import Targets, handle

pytestmark = pytest.mark.gpu


def gpu_frame(gsm, torch, name, pick=True, occ=None, states=None, styles=None):
    """One orthographic render_frame of the case into sentinel targets, captured: the view indexed by item."""
    case = X.case_of(name)
    w, h = case["width"], case["height"]
    items = len(X.projection_of(name)[1])
    scs, objects = _objects(gsm, torch, case)
    r, mw = _handle_for(gsm, torch, case, QUADRANT, items)
    t = Targets(torch, w, h)
    r.render_frame(t.color, t.depth, objects, w, h, pick=t.pick if pick else None,
                   occluder=None if occ is None else torch.from_numpy(np.ascontiguousarray(occ, np.float32)).cuda(),
                   states=None if states is None else _dev_states(torch, states),
                   styles=None if styles is None else _styles(gsm, styles), pick_pitch=t.pick_pitch,
                   orthographic=True)
    c, d, p = t.read(with_pick=pick)
    assert r.counters()["overflow"] == 0
    view = _captured_view(gsm, r, case, items, mw, c, d, p if pick else None)
    r.close()
    return view


@pytest.mark.parametrize("name", X.ALL)
def test_frame_and_pick(gsm, cuda, name):
    """Every case, the sigma = -1 camera and the three-object composite among them."""
    pr, owner = X.projection_of(name)
    v = gpu_frame(gsm, cuda, name)
    X.check_frame(name, v, pr, owner, pick=True, what=name)
    assert (pr["visible"] & ~T.left_out(pr)).sum() > 0.3 * len(pr["visible"])


@pytest.mark.parametrize("name,kind", [("ortho_sparse_sh1_f16_200x150", "ramp"), ("ortho_dense_sh0_f32_128x64", "step")])
def test_occluded(gsm, cuda, name, kind):
    pr, owner = X.projection_of(name)
    occ = X.occluder_of(name, kind)
    v = gpu_frame(gsm, cuda, name, occ=occ)
    model = X.check_frame(name, v, pr, owner, occ=occ, pick=True, what=f"{name} {kind}")
    if "sparse" in name:
        F.assert_occluder_not_vacuous(model, f"{name} {kind}")


def test_all_options_composite(gsm, cuda):
    name = X.COMPOSITE
    states = F.all_options_states(F.counts_of(X.case_of(name)))
    spr, owner = X.styled_projection(name, states)
    occ = X.occluder_of(name, "step")
    v = gpu_frame(gsm, cuda, name, occ=occ, states=states, styles=F.STYLES)
    X.check_frame(name, v, spr, owner, occ=occ, pick=True, what="composite, all options")
    assert spr["visible"][v["pick"][v["pick"] >= 0]].all(), "a hidden gaussian is picked"


def test_select_mask_ortho(gsm, cuda):
    c, pr, before, at = X.select_inputs()
    w, h = c["width"], c["height"]
    scs, objects = _objects(gsm, cuda, c)
    n = scs[0].n
    r = handle(gsm, n, w, h, scs[0].prec)
    matched = cuda.zeros(1, dtype=cuda.int32, device="cuda")
    total = 0
    for what, mname, am, xm, styled in F.select_cases():
        mask = F.masks(w, h, at)[mname]
        dev = cuda.from_numpy(before.copy()).cuda()
        r.select_mask(objects[0].input, objects[0].camera, w, h, cuda.from_numpy(mask.copy()).cuda(), dev, am, xm,
                      styles=_styles(gsm, F.STYLES) if styled else None, matched=matched, orthographic=True)
        cuda.cuda.synchronize()
        want, mcnt, doubt = M.select_mask(pr, before, mask, w, h, am, xm, styles=F.STYLES if styled else None,
                                          eps=T.BOUNDARY_EPS["mean"] * max(w, h))
        F.check_select(X.SELECT, dev.cpu().numpy(), int(matched.item()), before, want, mcnt, doubt | T.left_out(pr),
                       what)
        total += mcnt
    r.close()
    assert total > 100
