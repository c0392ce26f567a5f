"""gsm_global_extract, gsm_global_state_histogram and the keep-set helpers against their restatement
in numpy (tests/extract_ref.py): every output compared whole, sentinel rows included, so the rows at and past
min(K, capacity) are proven untouched; then the styled entries' identity (render of the extracted scene ==
render_styled of the full scene with hidden styles), the split, the histogram, every refusal row in order, graph
replay, and the same through the C ABI alone (tests/c/extract_sequence.c)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import extract_ref  # noqa: E402

ERR_COUNT, ERR_SIZE, ERR_MISSING, ERR_ARG = 6, 8, 13, 14
FILL, KFILL, GUARD = 0xA5, 0x7FFFFFFF, 3
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1000, 65_795]
CSRC = os.path.join(ROOT, "gsm-renderer_amd", "csrc")
CHECK_SRC = os.path.join(HERE, "host", "extract_check_test.cpp")
SEQ_BIN = os.path.join(HERE, "c", "extract_sequence")


# ---- CPU: declaration, layout, helpers, refusals without a device ----
def test_entries_are_declared_exported_and_bound(gsm):
    src = open(os.path.join(ROOT, "include", "gsm_renderer.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.library_path()], capture_output=True, text=True,
                         check=True).stdout
    for name, ret in (("gsm_global_extract", "gsm_status"), ("gsm_global_state_histogram", "gsm_status"),
                      ("gsm_global_keep_visible", "void"), ("gsm_global_keep_masked", "void")):
        assert re.search(r"%s\s+%s\s*\(" % (ret, name), src), name
        assert f" T {name}\n" in out, name
        assert name in gsm._SIGNATURES, name
    assert re.search(r"#define\s+GSM_ABI_VERSION\s+1\b", src), "the ABI only grows"
    for name in ("extract", "state_histogram"):
        assert callable(getattr(gsm.GlobalRenderer, name, None)), name
    assert callable(gsm.keep_visible) and callable(gsm.keep_masked)


def test_extract_out_is_40_bytes(gsm, tmp_path):
    prog = tmp_path / "size.c"
    prog.write_text('#include "gsm_renderer.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(gsm_global_extract_out),'
                    ' offsetof(gsm_global_extract_out, gaussians), offsetof(gsm_global_extract_out, harmonics),'
                    ' offsetof(gsm_global_extract_out, state), offsetof(gsm_global_extract_out, ids),'
                    ' offsetof(gsm_global_extract_out, capacity));return 0;}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    E = gsm._ExtractOut
    assert got == [40, E.gaussians.offset, E.harmonics.offset, E.state.offset, E.ids.offset, E.capacity.offset]
    assert C.sizeof(E) == 40


@pytest.mark.parametrize("entries", [0, 1, 7, 256])
def test_keep_visible_agrees_with_numpy(gsm, entries):
    rng = np.random.default_rng(entries)
    hidden = rng.random(entries) < 0.4
    if entries:
        hidden[entries - 1] = True
    styles = [gsm.Style((1, 2, 3), 9, 200, bool(h)) for h in hidden]
    want = extract_ref.keep_visible(hidden)
    assert gsm.keep_visible(styles) == want
    bits = extract_ref.keep_bits(want)
    assert np.array_equal(bits[:entries], ~hidden) and bits[entries:].all()
    if entries == 0:
        assert gsm.keep_visible(None) == [0xFFFFFFFF] * 8 and want == [0xFFFFFFFF] * 8
    else:
        # a count of 0 reads no table; a count above 256 is read as 256 (the array holds 256 entries then)
        assert gsm.keep_visible(styles, style_count=0) == [0xFFFFFFFF] * 8
        if entries == 256:
            assert gsm.keep_visible(styles, style_count=1000) == want


@pytest.mark.parametrize("mask,value", [(0, 0), (0, 1), (1, 1), (1, 0), (0x80, 0x80), (0x80, 0), (0x80, 1),
                                        (0xFF, 0x9C), (0xFF, 0), (0x1FF, 0x19C)])
def test_keep_masked_agrees_with_numpy(gsm, mask, value):
    got = gsm.keep_masked(mask, value)
    assert got == extract_ref.keep_masked(mask, value)
    s = np.arange(256)
    assert np.array_equal(extract_ref.keep_bits(got), (s & mask & 0xFF) == (value & 0xFF))


def test_null_handle_is_refused(gsm):
    L = gsm._lib()
    inp, st, out = gsm._Input(None, None, 0, 0), gsm._State(None, 0, 0), gsm._ExtractOut(None, None, None, None, 0, 0)
    keep = (C.c_uint32 * 8)()
    assert L.gsm_global_extract(None, None, C.byref(inp), C.byref(st), keep, C.byref(out), 16) == ERR_ARG
    assert L.gsm_global_extract(None, None, None, None, None, None, None) == ERR_ARG
    assert L.gsm_global_state_histogram(None, None, None, 0, 16) == ERR_ARG
    assert L.gsm_global_state_histogram(None, None, None, 1, None) == ERR_ARG


def test_every_refusal_row_on_the_cpu(tmp_path):
    """tests/host/extract_check_test.cpp: the checks' header alone, every row of both tables and their order, the
    helpers for all 256 states -- a stand-alone program built with the address and undefined-behaviour sanitizers
    and run here, with no device and no Python in its process."""
    exe = tmp_path / "extract_check_test"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", "-I" + CSRC, "-o", str(exe), CHECK_SRC], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout


def test_c_source_uses_only_declared_entry_points():
    src = open(os.path.join(HERE, "c", "extract_sequence.c")).read()
    hdrs = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("gsm_renderer.h", "gsm_debug.h"))
    names = set(re.findall(r"\b(gsm_\w+)\(", src))
    assert {"gsm_global_select_mask", "gsm_global_extract", "gsm_global_render", "gsm_global_keep_masked",
            "gsm_global_state_histogram"} <= names
    for name in names:
        assert re.search(rf"\b{name}\(", hdrs), name


# ---- GPU helpers ----
def record_bytes(prec):
    return 32 if prec else 48


def row_bytes(prec, sh):
    return 3 * sh * (2 if prec else 4)


def random_rows(torch, rng, n, nbytes):
    """(host rows (n, nbytes) uint8, the same on the device): any bytes will do, rows are copied, never decoded"""
    a = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    return a, torch.from_numpy(a.reshape(-1).copy()).cuda() if a.size else None


class Outputs:
    """Sentinel-filled outputs of `rows` rows plus GUARD rows; the harmonics start `shift` bytes past a 16-byte
    boundary."""

    def __init__(self, torch, prec, sh, rows, shift=0):
        self.torch, self.rec, self.row, self.rows, self.shift = torch, record_bytes(prec), row_bytes(prec, sh), rows, shift
        n = rows + GUARD
        self.g = torch.empty(n * self.rec, dtype=torch.uint8, device="cuda")
        self.h = torch.empty(n * self.row + 16, dtype=torch.uint8, device="cuda")
        self.s = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.i = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
        self.kept = torch.empty(2, dtype=torch.int32, device="cuda")
        assert self.g.data_ptr() % 16 == 0 and self.h.data_ptr() % 16 == 0
        self.hview = self.h[shift:] if self.row else None

    def refill(self):
        for t in (self.g, self.h, self.s, self.i):
            t.fill_(FILL)
        self.kept.fill_(KFILL)

    def expect(self, ids, recs, harm, states, with_state, with_ids):
        """the whole buffers as the contract leaves them: rows [0, len(ids)) written, the rest the sentinel"""
        n, m = self.rows + GUARD, len(ids)
        g = np.full((n, self.rec), FILL, np.uint8)
        g[:m] = recs
        h = np.full(n * self.row + 16, FILL, np.uint8)
        h[self.shift:self.shift + m * self.row] = harm.reshape(-1)
        s = np.full(n, FILL, np.uint8)
        i = np.full(n, FILL * 0x01010101, np.uint32)
        if with_state:
            s[:m] = states
        if with_ids:
            i[:m] = ids
        return g.reshape(-1), h, s, i

    def read(self):
        self.torch.cuda.synchronize()
        return (self.g.cpu().numpy(), self.h.cpu().numpy(), self.s.cpu().numpy(), self.i.cpu().numpy().view(np.uint32),
                self.kept.cpu().numpy())


def patterns(rng, n):
    """name -> (state: uint8 array or int (a NULL array, that default), keep set)"""
    bit = gsm_keep_masked(1, 1)
    half = extract_ref.keep_words(rng.random(256) < 0.5)
    few = extract_ref.keep_words(np.isin(np.arange(256), [7, 200, 255]))   # 3 of 256 states: p = 0.012
    uniform = rng.integers(0, 256, n).astype(np.uint8)
    hole = (rng.integers(0, 128, n) * 2 + (rng.random(n) < 0.5)).astype(np.uint8)
    hole[64:128] &= 0xFE     # one whole wave ...
    hole[256:512] &= 0xFE    # ... and one whole block with nothing kept
    last = np.zeros(n, np.uint8)
    last[-1] = 0x81
    return {
        "nothing": (rng.integers(0, 128, n).astype(np.uint8) * 2, bit),
        "everything": (rng.integers(0, 128, n).astype(np.uint8) * 2 + 1, bit),
        "alternating": ((np.arange(n) % 2).astype(np.uint8), bit),
        "random 0.5": (uniform, half),
        "random 0.01": (uniform, few),
        "last": (last, bit),
        "wave and block": (hole, bit),
        "default inside": (0x21, bit),
        "default outside": (0x20, bit),
    }


def gsm_keep_masked(mask, value):
    import gsm_amd
    return gsm_amd.keep_masked(mask, value)


# ---- 1. the numpy contract ----
@pytest.mark.gpu
@pytest.mark.parametrize("sh", [0, 1, 4, 9, 16])
@pytest.mark.parametrize("prec", [0, 1])
def test_extract_matches_the_numpy_contract(gsm, cuda, prec, sh):
    """Counts across a wave, a block and 257 blocks (a 256-wide scan loops); nine state patterns; capacities count,
    K, K - 1 and 0; out.state / out.ids given and NULL in turn; the output harmonics on a 16-byte boundary and one
    element past it in turn.  Every output is compared whole, its guard rows included."""
    from test_render_pick import handle
    rng = np.random.default_rng(100 * prec + sh)
    elem = 2 if prec else 4
    r = handle(gsm, max(COUNTS), 64, 64, prec)
    case = 0
    for n in COUNTS:
        recs, drecs = random_rows(cuda, rng, n, record_bytes(prec))
        harm, dharm = random_rows(cuda, rng, n, row_bytes(prec, sh))
        outs = [Outputs(cuda, prec, sh, n, shift) for shift in (0, elem)]
        for name, (state, keep) in patterns(rng, n).items():
            dstate = state if isinstance(state, int) else cuda.from_numpy(state).cuda()
            K = extract_ref.extract(recs, harm, state, keep, n)[1]
            if name in ("nothing", "default outside"):
                assert K == 0, name
            if name in ("everything", "default inside"):
                assert K == n, name
            for capacity in sorted({n, K, max(K - 1, 0), 0}, reverse=True):
                case += 1
                o = outs[case & 1]
                with_state, with_ids = (case >> 1) & 1 == 0, (case >> 2) & 1 == 0
                ids, K_, wr, wh, ws = extract_ref.extract(recs, harm, state, keep, capacity)
                o.refill()
                r.extract(gsm.GaussianInput(drecs, dharm, n, sh), dstate, keep, o.g, o.hview,
                          o.s if with_state else None, o.i if with_ids else None, capacity=capacity, kept=o.kept)
                got = o.read()
                want = o.expect(ids, wr, wh, ws, with_state, with_ids)
                what = f"n {n} {name} capacity {capacity} K {K_} shift {o.shift}"
                assert got[4].tolist() == [K_, KFILL], what
                for label, a, b in zip(("records", "harmonics", "state", "ids"), got, want):
                    bad = np.nonzero(a != b)[0]
                    assert len(bad) == 0, f"{what}: {label} differ at {bad[:4].tolist()} of {len(a)}"
    r.close()


# ---- 2. the header's identity ----
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_render_of_the_extracted_scene_equals_render_styled(gsm, cuda, prec):
    """Hidden styles only (the other styles, and the hidden styles' other fields, the identity): colour and depth of
    `render` over the scene extracted with keep_visible equal `render_styled` of the full scene byte for byte, and
    the pick images agree through out.ids."""
    import style_ref
    from gsm_amd import scenes
    from test_render_pick import NONE, Targets, gen, handle
    from test_render_styled import py_styles, styled
    n, w, h, sh = 50_000, 640, 360, 16
    sc = gen(cuda, n, w, h, sh, prec, 28)
    cam = scenes.make_camera(w, h)
    table = style_ref.style_table([(0, 0, 0, 0, 255, 0), (0, 0, 0, 0, 255, 1), (0, 0, 0, 0, 255, 0),
                                   (0, 0, 0, 0, 255, 0), (0, 0, 0, 0, 255, 1), (0, 0, 0, 0, 255, 0)])
    rng = np.random.default_rng(28)
    state = rng.integers(0, 9, n).astype(np.uint8)   # states 6, 7, 8: past the table
    r = handle(gsm, n, w, h, prec)
    dstate = cuda.from_numpy(state).cuda()
    c, d, p = styled(gsm, cuda, r, [(sc, cam)], w, h, [dstate], table)
    keep = gsm.keep_visible(py_styles(gsm, table))
    hidden = (state == 1) | (state == 4)
    assert np.array_equal(extract_ref.keep_bits(keep)[state], ~hidden) and 0 < hidden.sum() < n
    o = Outputs(cuda, prec, sh, n)
    o.refill()
    r.extract(sc.input(gsm), dstate, keep, o.g, o.hview, o.s, o.i, kept=o.kept)
    cuda.cuda.synchronize()
    K = int(o.kept[0].item())
    assert K == n - hidden.sum()
    ids = o.i.cpu().numpy().view(np.uint32)[:K]
    assert np.array_equal(ids, np.nonzero(~hidden)[0])
    t = Targets(cuda, w, h)
    r.render_pick(t.color, t.depth, t.pick, gsm.GaussianInput(o.g, o.hview, K, sh), gsm.CameraParams.from_dict(cam),
                  w, h, pick_pitch=t.pick_pitch)
    c2, d2, p2 = t.read()
    r.close()
    assert np.array_equal(c2, c), "colour"
    assert np.array_equal(d2, d), "depth"
    hit = p != NONE
    assert hit.any() and np.array_equal(hit, p2 != NONE), "GSM_PICK_NONE at different pixels"
    assert np.array_equal(ids[p2[hit].astype(np.int64)], p[hit]), "ids[pick of the extract] != styled pick"
    # and `render` itself, the entry the header names
    t.refill()
    r = handle(gsm, n, w, h, prec)
    r.render(t.color, t.depth, gsm.GaussianInput(o.g, o.hview, K, sh), gsm.CameraParams.from_dict(cam), w, h)
    c3, d3, _ = t.read(with_pick=False)
    r.close()
    assert np.array_equal(c3, c) and np.array_equal(d3, d)


# ---- 3. split ----
@pytest.mark.gpu
def test_split_by_the_selection_bit(gsm, cuda):
    from test_render_pick import handle
    n, prec, sh = 10_007, 1, 4
    rng = np.random.default_rng(3)
    recs, drecs = random_rows(cuda, rng, n, record_bytes(prec))
    harm, dharm = random_rows(cuda, rng, n, row_bytes(prec, sh))
    state = rng.integers(0, 256, n).astype(np.uint8)
    dstate = cuda.from_numpy(state).cuda()
    r = handle(gsm, n, 64, 64, prec)
    parts = []
    for value in (1, 0):
        o = Outputs(cuda, prec, sh, n)
        o.refill()
        r.extract(gsm.GaussianInput(drecs, dharm, n, sh), dstate, gsm.keep_masked(1, value), o.g, o.hview, o.s, o.i,
                  kept=o.kept)
        g, hh, s, i, kept = o.read()
        K = int(kept[0])
        ids = i[:K].astype(np.int64)
        assert (np.diff(ids) > 0).all(), "ascending"
        assert np.array_equal(g.reshape(-1, record_bytes(prec))[:K], recs[ids])
        assert np.array_equal(hh[:K * row_bytes(prec, sh)].reshape(K, -1), harm[ids]) and np.array_equal(s[:K], state[ids])
        parts.append(ids)
    r.close()
    a, b = parts
    assert len(a) + len(b) == n and len(np.intersect1d(a, b)) == 0
    assert np.array_equal(np.sort(np.concatenate([a, b])), np.arange(n))
    assert np.array_equal(a, np.nonzero(state & 1)[0])


# ---- 4. histogram ----
@pytest.mark.gpu
def test_state_histogram_matches_bincount(gsm, cuda):
    """The counts of the contract test, uniform random bytes and all bytes equal, the state array on a 4-byte
    boundary and 1, 2, 3 bytes past it; count 0.  The histogram starts from a sentinel and its guard words keep it."""
    from test_render_pick import handle
    rng = np.random.default_rng(4)
    r = handle(gsm, max(COUNTS), 64, 64, 1)
    hist = cuda.empty(256 + GUARD, dtype=cuda.int32, device="cuda")
    case = 0
    for n in [0] + COUNTS:
        for name in ("uniform", "equal"):
            state = rng.integers(0, 256, n).astype(np.uint8) if name == "uniform" else np.full(n, 0xC7, np.uint8)
            shift = case % 4
            case += 1
            dbuf = cuda.from_numpy(np.concatenate([np.full(shift, 0xC7, np.uint8), state,
                                                   np.full(5, 0xC7, np.uint8)])).cuda()
            hist.fill_(KFILL)
            r.state_histogram(dbuf[shift:] if n else None, n, hist)
            cuda.cuda.synchronize()
            got = hist.cpu().numpy()
            want = np.bincount(state, minlength=256)
            assert np.array_equal(want, extract_ref.histogram(state, n))
            assert np.array_equal(got[:256], want), (n, name, shift)
            assert (got[256:] == KFILL).all()
            assert got[:256].sum() == n
    r.close()


# ---- 5. refusals ----
@pytest.mark.gpu
def test_refusals_in_order_enqueue_nothing(gsm, cuda):
    from test_render_pick import handle
    n, prec, sh = 300, 1, 16
    rng = np.random.default_rng(5)
    _, drecs = random_rows(cuda, rng, n + 64, record_bytes(prec))
    _, dharm = random_rows(cuda, rng, n + 64, row_bytes(prec, sh))
    dstate = cuda.full((n + 64,), 1, dtype=cuda.uint8, device="cuda")
    before = [t.clone() for t in (drecs, dharm, dstate)]
    o = Outputs(cuda, prec, sh, n)
    o.refill()
    hist = cuda.full((256,), KFILL, dtype=cuda.int32, device="cuda")
    r = handle(gsm, 512, 64, 64, prec)
    all_ = [0xFFFFFFFF] * 8
    good = dict(g=drecs, h=dharm, n=n, sh=sh, st=dstate, keep=all_, og=o.g, oh=o.hview, os=o.s, oi=o.i, cap=n,
                kept=o.kept)

    def status(**kw):
        a = dict(good, **kw)
        try:
            r.extract(gsm.GaussianInput(a["g"], a["h"], a["n"], a["sh"]), a["st"], a["keep"], a["og"], a["oh"],
                      a["os"], a["oi"], capacity=a["cap"], kept=a["kept"])
        except gsm.RendererError as e:
            return int(e.status)
        return 0

    def ptr(t, off=0):
        return int(t.data_ptr()) + off

    L = gsm._lib()
    assert status(n=513) == ERR_COUNT
    # the structs (the binding always passes input and out: those two through ctypes)
    inp = gsm._Input(ptr(drecs), ptr(dharm), n, sh)
    st = gsm._State(ptr(dstate), 0, 0)
    out = gsm._ExtractOut(ptr(o.g), ptr(o.hview), None, None, n, 0)
    kw = (C.c_uint32 * 8)(*all_)
    assert L.gsm_global_extract(r._h, None, None, C.byref(st), kw, C.byref(out), ptr(o.kept)) == ERR_MISSING
    assert L.gsm_global_extract(r._h, None, C.byref(inp), C.byref(st), kw, None, ptr(o.kept)) == ERR_MISSING
    assert status(st=None) == ERR_MISSING and status(keep=None) == ERR_MISSING and status(kept=0) == ERR_MISSING
    assert status(g=None) == ERR_MISSING and status(h=None) == ERR_MISSING
    assert status(og=None) == ERR_MISSING and status(oh=None) == ERR_MISSING
    assert status(kept=ptr(o.kept, 2)) == ERR_SIZE and status(oi=ptr(o.i, 1)) == ERR_SIZE
    assert status(og=ptr(o.g, 8)) == ERR_SIZE and status(oh=ptr(o.h, 1)) == ERR_SIZE
    assert status(st=256) == ERR_ARG
    # overlap: an output that starts inside the input records; two outputs that share bytes; kept inside an input
    assert status(og=ptr(drecs, 32 * 10)) == ERR_ARG
    assert status(oi=ptr(o.s, 4 * (n // 8))) == ERR_ARG
    assert status(oh=ptr(o.g, 32 * (n - 1))) == ERR_ARG
    assert status(kept=ptr(dstate, n - 4)) == ERR_ARG and status(os=ptr(dharm, 96 * n - 1)) == ERR_ARG
    # the order: count, missing, size, argument
    assert L.gsm_global_extract(r._h, None, C.byref(gsm._Input(ptr(drecs), ptr(dharm), 513, sh)), None, kw,
                                C.byref(out), ptr(o.kept)) == ERR_COUNT
    assert status(g=None, kept=ptr(o.kept, 2)) == ERR_MISSING
    assert status(og=None, oi=ptr(o.i, 1)) == ERR_MISSING
    assert status(kept=ptr(o.kept, 2), st=256) == ERR_SIZE
    assert status(og=ptr(drecs, 8), st=256) == ERR_SIZE
    assert status(oh=ptr(o.h, 1), os=ptr(dstate)) == ERR_SIZE
    assert status(st=256, og=ptr(drecs, 32 * 10)) == ERR_ARG

    def hstatus(state=dstate, count=n, h=hist):
        try:
            r.state_histogram(state, count, h)
        except gsm.RendererError as e:
            return int(e.status)
        return 0

    assert hstatus(count=513) == ERR_COUNT
    assert hstatus(h=None) == ERR_MISSING and hstatus(state=None) == ERR_MISSING
    assert hstatus(h=ptr(hist, 2)) == ERR_SIZE
    assert hstatus(state=None, count=513) == ERR_COUNT and hstatus(state=None, h=ptr(hist, 2)) == ERR_MISSING
    cuda.cuda.synchronize()
    got = o.read()
    assert all((a == FILL).all() for a in got[:3]) and (got[3] == FILL * 0x01010101).all(), "a refused call wrote"
    assert got[4].tolist() == [KFILL, KFILL] and (hist == KFILL).all().item()
    assert all(cuda.equal(a, b) for a, b in zip(before, (drecs, dharm, dstate)))
    # what the rows leave alone: a NULL buffer without a count, or without a capacity; just apart is no overlap
    assert status(g=None, h=None, n=0) == 0
    cuda.cuda.synchronize()
    assert o.kept.tolist() == [0, KFILL]
    assert status(og=None, oh=None, os=None, oi=None, cap=0) == 0
    cuda.cuda.synchronize()
    assert o.kept.tolist() == [n, KFILL]
    assert status(og=ptr(drecs, 32 * n), cap=64, os=None, oi=None, oh=ptr(dharm, 96 * n)) == 0
    assert hstatus() == 0 and hstatus(state=None, count=0) == 0
    cuda.cuda.synchronize()
    r.close()


# ---- 6. capture ----
@pytest.mark.gpu
def test_captured_extract_and_histogram_follow_the_replays_state(gsm, cuda):
    """One extract and one histogram in a graph (a linear chain on one stream), replayed after the state bytes
    changed: the outputs follow the new bytes; the keep set and the pointers are the captured ones."""
    from test_render_pick import handle
    n, prec, sh = 5000, 0, 9
    rng = np.random.default_rng(6)
    recs, drecs = random_rows(cuda, rng, n, record_bytes(prec))
    harm, dharm = random_rows(cuda, rng, n, row_bytes(prec, sh))
    dstate = cuda.zeros(n, dtype=cuda.uint8, device="cuda")
    hist = cuda.empty(256, dtype=cuda.int32, device="cuda")
    o = Outputs(cuda, prec, sh, n)
    keep = gsm.keep_masked(0x81, 0x01)
    r = handle(gsm, n, 64, 64, prec)
    inp = gsm.GaussianInput(drecs, dharm, n, sh)
    o.refill()
    r.extract(inp, dstate, keep, o.g, o.hview, o.s, o.i, kept=o.kept)   # (the handle's first extract allocates)
    cuda.cuda.synchronize()
    assert o.kept[0].item() == 0
    s = cuda.cuda.Stream()
    g = cuda.cuda.CUDAGraph()
    with cuda.cuda.graph(g, stream=s):
        r.extract(inp, dstate, keep, o.g, o.hview, o.s, o.i, kept=o.kept, stream=s)
        r.state_histogram(dstate, n, hist, stream=s)
    cuda.cuda.synchronize()
    for seed in (1, 2):
        state = np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)
        dstate.copy_(cuda.from_numpy(state).cuda())
        o.refill()
        hist.fill_(KFILL)
        cuda.cuda.synchronize()
        g.replay()
        got = o.read()
        ids, K, wr, wh, ws = extract_ref.extract(recs, harm, state, keep, n)
        assert 0 < K < n and got[4].tolist() == [K, KFILL]
        for a, b in zip(got, o.expect(ids, wr, wh, ws, True, True)):
            assert np.array_equal(a, b)
        assert np.array_equal(hist.cpu().numpy(), extract_ref.histogram(state, n))
    r.close()


# ---- 7. through the C ABI alone ----
@pytest.mark.gpu
def test_extract_sequence_through_the_c_abi(tmp_path, oracle):
    """tests/c/extract_sequence.c: select_mask, state_histogram, extract, render of the extracted scene -- no Python
    and no torch in that process.  kept equals the select's matched count and the histogram's; the extracted rows
    and the frame are written out and compared here with numpy and the oracle."""
    from gsm_amd import scenes
    O = oracle
    assert os.path.exists(SEQ_BIN), "tests/c/extract_sequence not built (__graft_entry__.build)"
    n, W, H, sh = 20_000, 320, 180, 16
    world, harm, cam = scenes.gen_scene(n, W, H, sh, 1, seed=11)
    (tmp_path / "w.bin").write_bytes(world.tobytes())
    (tmp_path / "h.bin").write_bytes(harm.tobytes())
    cf = np.concatenate([cam["view"], cam["proj"], cam["position"],
                         np.array([cam["focal_x"], cam["focal_y"], cam["near"], cam["far"]], np.float32)])
    (tmp_path / "c.bin").write_bytes(cf.astype(np.float32).tobytes())
    p = subprocess.run([SEQ_BIN, str(tmp_path / "w.bin"), str(tmp_path / "h.bin"), str(n), str(sh), str(W), str(H),
                        str(tmp_path / "c.bin"), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr + p.stdout
    m = re.search(r"matched (\d+) kept (\d+) histogram (\d+)", p.stdout)
    assert m, p.stdout
    matched, kept, hsel = (int(x) for x in m.groups())
    assert 0 < matched < n and kept == matched and hsel == matched
    ids = np.frombuffer((tmp_path / "out.ids").read_bytes(), np.uint32)
    assert len(ids) == kept and (np.diff(ids.astype(np.int64)) > 0).all()
    w8 = np.frombuffer(world.tobytes(), np.uint8).reshape(n, -1)
    h8 = np.frombuffer(np.asarray(harm).tobytes(), np.uint8).reshape(n, -1)
    assert (tmp_path / "out.gaussians").read_bytes() == w8[ids].tobytes()
    assert (tmp_path / "out.harmonics").read_bytes() == h8[ids].tobytes()
    ref = O.render(world[ids], np.asarray(harm).reshape(n, -1)[ids].reshape(-1), sh, cam, W, H, max_gaussians=n)
    got = np.frombuffer((tmp_path / "out.color").read_bytes(), np.uint16).reshape(H, W, 4)
    assert np.array_equal(got, ref["color"])
