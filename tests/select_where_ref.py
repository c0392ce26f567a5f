"""gsm_global_select_where and gsm_global_state_bounds (include/gsm_renderer.h) restated in numpy.
Every product and sum of the shape test is its own np.float32 operation in the header's order; fp16 fields are
widened with .astype(np.float32); the results are exact: state bytes, the matched count and the eight words of the
bounds are compared for equality."""
import numpy as np

ALL, BOX, ELLIPSOID, OUTSIDE = 0, 1, 2, 1
F = np.float32
INF = F(np.inf)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def query(shape=ALL, flags=0, to_shape=IDENTITY, opacity=(-np.inf, np.inf), scale=(-np.inf, np.inf), test=(0, 0)):
    """the fields of gsm_global_select_query as a dict (the defaults are gsm_global_select_query_default's)"""
    return dict(shape=shape, flags=flags, to_shape=np.asarray(to_shape, F).reshape(12), opacity=tuple(F(v) for v in opacity),
                scale=tuple(F(v) for v in scale), test=tuple(int(v) for v in test))


def attributes(world):
    """(px, py, pz, opacity, sx, sy, sz) as float32 arrays of a WORLD32 or WORLD16 structured array"""
    def f(name):
        a = world[name]
        return a.view(np.float16).astype(F) if a.dtype == np.uint16 else a.astype(F)
    return tuple(f(k) for k in ("px", "py", "pz", "opacity", "sx", "sy", "sz"))


def shape_q(A, px, py, pz):
    """the three rows of q, each ((a0*px + a1*py) + a2*pz) + a3 in float32"""
    A = np.asarray(A, F).reshape(3, 4)
    with np.errstate(all="ignore"):
        return [((A[r, 0] * px + A[r, 1] * py) + A[r, 2] * pz) + A[r, 3] for r in range(3)]


def in_range(lo, hi, v):
    """None when the range is exactly (-inf, +inf): not applied"""
    if lo == -INF and hi == INF:
        return None
    with np.errstate(invalid="ignore"):
        return (lo <= v) & (v <= hi)


def matches(world, q, state, hidden=None):
    """the boolean match of every gaussian.  hidden: the `hidden` bytes of a style table, or None for no table"""
    px, py, pz, o, sx, sy, sz = attributes(world)
    old = np.asarray(state, np.uint8)[:len(world)].astype(np.uint32)
    m = (old & (q["test"][0] & 0xFF)) == (q["test"][1] & 0xFF)
    if hidden is not None:
        h = np.zeros(256, bool)
        h[:len(hidden)] = np.asarray(hidden) != 0
        m &= ~h[old]
    if q["shape"] != ALL:
        v = shape_q(q["to_shape"], px, py, pz)
        assert all(x.dtype == F for x in v)
        with np.errstate(all="ignore"):
            if q["shape"] == BOX:
                inside = (np.abs(v[0]) <= F(1)) & (np.abs(v[1]) <= F(1)) & (np.abs(v[2]) <= F(1))
            else:
                inside = ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) <= F(1)
        nan = np.isnan(v[0]) | np.isnan(v[1]) | np.isnan(v[2])
        m &= ~nan & (inside != bool(q["flags"] & OUTSIDE))
    r = in_range(*q["opacity"], o)
    if r is not None:
        m &= r
    with np.errstate(invalid="ignore"):
        r = in_range(*q["scale"], np.fmax(np.fmax(sx, sy), sz))   # fmax: maxNum, NaN only when all three are
    if r is not None:
        m &= r
    return m


def select_where(world, q, state, and_mask, xor_mask, hidden=None):
    """-> (the new state bytes, matched); bytes at or past len(world) keep their value"""
    state = np.asarray(state, np.uint8)
    m = matches(world, q, state, hidden)
    out = state.copy()
    old = state[:len(world)].astype(np.uint32)
    new = (((old & (and_mask & 0xFFFFFFFF)) ^ (xor_mask & 0xFFFFFFFF)) & 0xFF).astype(np.uint8)
    out[:len(world)][m] = new[m]
    return out, int(m.sum())


def state_bounds(world, state, keep_bits):
    """state: a uint8 array or an int (every gaussian's state); keep_bits: 256 booleans.
    -> the eight words of gsm_global_bounds as a uint32 array: min[3], max[3] (float32 bits), count, skipped"""
    n = len(world)
    s = np.full(n, int(state), np.uint8) if isinstance(state, (int, np.integer)) else np.asarray(state, np.uint8)[:n]
    part = np.asarray(keep_bits, bool)[s]
    p = np.stack([world["px"], world["py"], world["pz"]], axis=1).astype(F)[part]
    finite = np.isfinite(p).all(axis=1)
    p = p[finite]
    p[p == 0] = F(0)   # -0 counts as +0
    mn = p.min(axis=0) if len(p) else np.full(3, np.inf, F)
    mx = p.max(axis=0) if len(p) else np.full(3, -np.inf, F)
    out = np.empty(8, np.uint32)
    out[:3] = mn.astype(F).view(np.uint32)
    out[3:6] = mx.astype(F).view(np.uint32)
    out[6], out[7] = len(p), int(part.sum()) - len(p)
    return out
