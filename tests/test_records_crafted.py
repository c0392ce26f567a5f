"""gsm_global_render_records on crafted records (tests/records_cases.py): the scatter
(k_records_in / k_scatter), the frame sort and every blend kernel get exactly the fp16 bits, rects and tile masks a
case wants, and colour, depth, the unsorted and sorted keys / values and the headers must equal the reference
(tests/records_ref.py: the lists in numpy, the blend by the oracle's blend_tiles) bit for bit.  The properties each
case is there for are asserted in test_records_ref.py, without a device.

Every case renders three times on one renderer -- the first frame captured (keys, values, headers read back), the
later ones on the product path, taking the first frame's cost order -- into targets of a different layout each
time (tight, padded and 16-byte aligned, offset by 8 bytes, no depth), all pre-filled with a sentinel whose
padding, guard row and leading bytes must stay untouched.  Then another case renders on the same renderer."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import records_cases as K  # noqa: E402
import records_ref as R  # noqa: E402

QUADRANT, HALF_TILE, PAIR_WALK = 1, 2, 3  # gsm_blend_kernel (include/gsm_debug.h)
BLEND_ENV = ("GSM_BLEND_WAVES", "GSM_BLEND_PAIR_SPLIT", "GSM_BLEND_SCHED", "GSM_BLEND_PAIRS", "GSM_BLEND_CLAIM",
             "GSM_SORT_RANK", "GSM_SORT_WIDE", "GSM_SORT", "GSM_SCAN_FUSED")
# name -> (geometry, environment at create, the blend kernel the frames must report)
CONFIGS = {
    "quadrant": ("small", {}, QUADRANT),
    "half_tile": ("wide", {}, HALF_TILE),
    "pair_walk_split1": ("wide", {"GSM_BLEND_WAVES": "16", "GSM_BLEND_PAIR_SPLIT": "1"}, PAIR_WALK),
    "pair_walk_split256": ("wide", {"GSM_BLEND_WAVES": "16", "GSM_BLEND_PAIR_SPLIT": "256"}, PAIR_WALK),
    "index_order": ("wide", {"GSM_BLEND_SCHED": "0"}, HALF_TILE),
    "ballot_ranks": ("small", {"GSM_SORT_RANK": "ballot"}, QUADRANT),
}
CASE_NAMES = list(K.CASES)
LAYOUTS = ("tight", "padded", "offset8", "no_depth")
SENTINEL = 0xA5


def open_renderer(gsm, monkeypatch, geo, env):
    for k in BLEND_ENV:  # read at create
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, _, mw, mh = K.GEOMETRIES[geo] if isinstance(geo, str) else geo
    r = gsm.GlobalRenderer(config=gsm.RendererConfig(max_gaussians=K.MAX_GAUSSIANS, max_width=mw, max_height=mh,
                                                      precision=1, gaussian_color_space=0))
    for k in env:
        monkeypatch.delenv(k)
    return r


class Target:
    """colour and depth targets of one layout inside sentinel-filled byte buffers with a guard row"""

    def __init__(self, torch, w, h, layout):
        self.w, self.h, self.layout = w, h, layout
        pad = layout in ("padded", "offset8")
        self.cp = -(-(w * 8 + (24 if pad else 0)) // 16) * 16 if pad else w * 8
        self.dp = -(-(w * 2 + (10 if pad else 0)) // 16) * 16 if pad else w * 2
        self.off = 8 if layout == "offset8" else 0
        self.cbuf = torch.full(((h + 1) * self.cp + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.dbuf = None if layout == "no_depth" else \
            torch.full(((h + 1) * self.dp + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.cbuf.data_ptr() % 16 == 0 and (self.dbuf is None or self.dbuf.data_ptr() % 16 == 0)
        if layout == "padded":
            assert self.cp % 16 == 0 and self.dp % 16 == 0  # the wide stores
        if layout == "tight" and w % 2:
            assert self.cp % 16 == 8  # an odd width: rows 8 bytes off
        self.color = self.cbuf[self.off:]
        self.depth = None if self.dbuf is None else self.dbuf[self.off:]

    def read(self):
        """(colour [h, w, 4], depth [h, w] or None) as fp16 bits, after asserting that nothing else was written"""
        out = []
        for buf, pitch, px in ((self.cbuf, self.cp, 8), (self.dbuf, self.dp, 2)):
            if buf is None:
                out.append(None)
                continue
            raw = buf.cpu().numpy()
            assert (raw[:self.off] == SENTINEL).all(), "bytes before the target were written"
            body = raw[self.off:self.off + (self.h + 1) * pitch].reshape(self.h + 1, pitch)
            assert (body[self.h] == SENTINEL).all(), "the guard row was written"
            assert (body[:self.h, self.w * px:] == SENTINEL).all(), "the padding past a row's pixels was written"
            assert (raw[self.off + (self.h + 1) * pitch:] == SENTINEL).all()
            img = np.ascontiguousarray(body[:self.h, :self.w * px]).view(np.uint16)
            out.append(img.reshape(self.h, self.w, 4) if px == 8 else img.reshape(self.h, self.w))
        return out


def check_image(fr, ref, color, depth, what):
    bad = np.argwhere((color != ref["color"]).any(axis=2))
    if depth is not None:
        bad_d = np.argwhere(depth != ref["depth"])
        bad = np.concatenate([bad, bad_d]) if len(bad_d) else bad
    if len(bad):
        y, x = (int(v) for v in bad[np.lexsort((bad[:, 1], bad[:, 0]))][0])
        got = [int(v) for v in color[y, x]] + ([int(depth[y, x])] if depth is not None else [])
        want = [int(v) for v in ref["color"][y, x]] + [int(ref["depth"][y, x])]
        tiles = np.unique((bad[:, 0] // 16) * fr.tiles_x + bad[:, 1] // 32)
        raise AssertionError("%s, %s: %d pixels differ in tiles %s; first: got %s, want %s; %s" %
                             (fr.name, what, len(np.unique(bad, axis=0)), tiles[:8].tolist(),
                              [hex(v) for v in got], [hex(v) for v in want], R.explain_pixel(fr, ref, y, x, got)))


def first_diff(name, got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.shape != want.shape:
        return "%s: %d values, want %d" % (name, got.size, want.size)
    i = np.flatnonzero(got != want)
    return "%s: %d differ, first at %d: got %s, want %s" % (name, i.size, i[0], got[i[0]], want[i[0]]) if i.size \
        else name + ": equal"


def render_and_check(gsm, torch, oracle, renderer, name, geo, kind, layouts, capture_first=True):
    fr = K.frame(name, geo)
    ref = R.reference(fr, oracle)
    assert ref["keys"].size <= 4 * K.MAX_GAUSSIANS and fr.count <= K.MAX_GAUSSIANS
    rec = torch.from_numpy(R.pack(fr).view(np.uint8).reshape(-1).copy()).cuda()
    for n, layout in enumerate(layouts):
        capture = capture_first and n == 0
        renderer.set_profiling(stage_events=False, keep_unsorted=capture, capture=capture)
        t = Target(torch, fr.width, fr.height, layout)
        renderer.render_records(t.color, t.depth, rec, fr.count, fr.width, fr.height, color_pitch=t.cp,
                                depth_pitch=t.dp)
        torch.cuda.synchronize()
        what = "frame %d (%s)" % (n, layout)
        assert renderer.blend_kernel_kind() == kind, "%s: blend kernel %d" % (what, renderer.blend_kernel_kind())
        c = renderer.counters()
        assert c["total_assignments"] == ref["keys"].size and c["overflow"] == 0, (what, c)
        if capture:
            B = gsm.BufferId
            for buf, key in ((B.KEYS, "keys"), (B.VALUES, "values"), (B.HEADERS, "headers"),
                             (B.SORTED_KEYS, "sorted_keys"), (B.SORTED_VALUES, "sorted_values")):
                got = renderer.copy_buffer(buf)
                assert np.array_equal(got.reshape(-1), ref[key].reshape(-1)), \
                    "%s, %s: %s" % (fr.name, what, first_diff(key, got, ref[key]))
        color, depth = t.read()
        check_image(fr, ref, color, depth, what)


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_crafted_records(gsm, cuda, oracle, monkeypatch, config, name):
    geo, env, kind = CONFIGS[config]
    i = CASE_NAMES.index(name)
    layouts = [LAYOUTS[(i + n) % 4] for n in range(3)]
    other = CASE_NAMES[(i + 3) % len(CASE_NAMES)]
    r = open_renderer(gsm, monkeypatch, geo, env)
    try:
        render_and_check(gsm, cuda, oracle, r, name, geo, kind, layouts)
        # another case on the same renderer: the unit costs and half counts of the frames before are stale
        render_and_check(gsm, cuda, oracle, r, other, geo, kind, [LAYOUTS[(i + 3) % 4]], capture_first=False)
    finally:
        r.close()


def test_every_layout_meets_every_kernel():
    """(no device) the rotation above gives every blend kernel every target layout on some case"""
    assert len(CASE_NAMES) >= 4 and {kind for _, _, kind in CONFIGS.values()} == {QUADRANT, HALF_TILE, PAIR_WALK}
    used = {LAYOUTS[(i + n) % 4] for i in range(len(CASE_NAMES)) for n in range(4)}
    assert used == set(LAYOUTS)


@pytest.mark.parametrize("shape", K.TINY_SHAPES)
def test_small_frame_shapes(gsm, cuda, oracle, monkeypatch, shape):
    """frames of a few pixels, of one tile and a sliver of a second: every layout, the stores at the frame's edge"""
    geo = shape + shape
    r = open_renderer(gsm, monkeypatch, geo, {})
    try:
        render_and_check(gsm, cuda, oracle, r, "sprinkle", geo, QUADRANT, list(LAYOUTS))
    finally:
        r.close()


def test_a_bent_reference_fails_against_the_gpu(gsm, cuda, oracle, monkeypatch):
    """the comparison tells the frame from a reference with its ties reversed (the 600 equal keys of `scatter`)"""
    fr = K.frame("scatter", "small")
    ref = R.reference(fr, oracle)
    tile = fr.notes["ties"][0]
    bent_lists = R.lists(fr, "ties_reversed")
    hdr = np.zeros_like(ref["headers"])
    hdr[tile] = ref["headers"][tile]
    bent = R.blend(fr, dict(bent_lists, headers=hdr))
    x0, y0 = (tile % fr.tiles_x) * 32, (tile // fr.tiles_x) * 16
    r = open_renderer(gsm, monkeypatch, "small", {})
    try:
        t = Target(cuda, fr.width, fr.height, "tight")
        rec = cuda.from_numpy(R.pack(fr).view(np.uint8).reshape(-1).copy()).cuda()
        r.render_records(t.color, t.depth, rec, fr.count, fr.width, fr.height, color_pitch=t.cp, depth_pitch=t.dp)
        cuda.cuda.synchronize()
        color, _ = t.read()
    finally:
        r.close()
    assert np.array_equal(color[y0:y0 + 16, x0:x0 + 32], ref["color"][y0:y0 + 16, x0:x0 + 32])
    assert not np.array_equal(color[y0:y0 + 16, x0:x0 + 32], bent["color"][y0:y0 + 16, x0:x0 + 32])
