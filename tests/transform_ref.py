"""gsm_global_transform (include/gsm_renderer.h) restated in numpy (TEST INFRASTRUCTURE).

apply() is the entry's arithmetic in float32, operation by operation in the header's order, with explicit float32
temporaries; fp16 fields are widened exactly and rounded back once by astype(np.float16).  desc_f64() derives the
descriptor of a pose in float64 from the property that defines it -- the band matrices as a least-squares fit over a
few hundred directions with f64_model.sh_basis, the quaternion as an eigenvector -- and shares no method with the C
helper (gsm_transform_check.h: an exact solve over 2l+1 directions, Shepperd's quaternion)."""
import numpy as np

import extract_ref
import f64_model

F = np.float32
BANDS = {0: [], 1: [], 4: [(1, 3)], 9: [(1, 3), (4, 5)], 16: [(1, 3), (4, 5), (9, 7)]}  # (first index, size)
NAMES = ("matrix", "quaternion", "scale", "sh1", "sh2", "sh3")


def desc(matrix, quaternion, scale, sh1, sh2, sh3):
    """a descriptor as a dict of float32 arrays (what apply takes)"""
    return dict(matrix=np.asarray(matrix, F).reshape(12).copy(), quaternion=np.asarray(quaternion, F).reshape(4).copy(),
                scale=F(scale), sh1=np.asarray(sh1, F).reshape(9).copy(), sh2=np.asarray(sh2, F).reshape(25).copy(),
                sh3=np.asarray(sh3, F).reshape(49).copy())


def desc_of(t):
    """the dict of a gsm_amd.Transform"""
    return desc(t.matrix, t.quaternion, t.scale, t.sh1, t.sh2, t.sh3)


def _h2f(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(F)


def _f2h(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, F).astype(np.float16).view(np.uint16)


def _rows(D, c):
    """c'_i = (..((D[i][0] c_0 + D[i][1] c_1) + D[i][2] c_2)..) + D[i][N-1] c_{N-1}, float32, for c [n, N]"""
    N = c.shape[1]
    D = np.asarray(D, F).reshape(N, N)
    out = np.empty_like(c)
    for i in range(N):
        acc = (D[i, 0] * c[:, 0]).astype(F)
        for j in range(1, N):
            acc = (acc + (D[i, j] * c[:, j]).astype(F)).astype(F)
        out[:, i] = acc
    return out


def apply(world, harm, sh_components, prec, state, keep, d):
    """(new records, new harmonics).  world: the structured records; harm: the flat harmonics (float32, or fp16 bits
    as uint16; None or anything with sh_components 0 or 1: returned as it came, never read); state: a uint8 array or
    an int; keep: the 8 words; d: desc().  Copies: the inputs stay as they are."""
    n = len(world)
    take = extract_ref.keep_bits(keep)[extract_ref.states_of(state, n)]
    out = world.copy()
    m = np.asarray(d["matrix"], F).reshape(3, 4)
    a = np.asarray(d["quaternion"], F)
    s = F(d["scale"])
    with np.errstate(all="ignore"):
        px, py, pz = (world[k][take].astype(F) for k in ("px", "py", "pz"))
        for r, k in enumerate(("px", "py", "pz")):
            t0 = (m[r, 0] * px).astype(F)
            t1 = (m[r, 1] * py).astype(F)
            t2 = (m[r, 2] * pz).astype(F)
            out[k][take] = (((t0 + t1).astype(F) + t2).astype(F) + m[r, 3]).astype(F)
        if prec:
            for k in ("sx", "sy", "sz"):
                out[k][take] = _f2h((_h2f(world[k][take]) * s).astype(F))
            x, y, z, w = (_h2f(world[k][take]) for k in ("rx", "ry", "rz", "rw"))
        else:
            for k in ("sx", "sy", "sz"):
                out[k][take] = (world[k][take] * s).astype(F)
            x, y, z, w = (world["rot"][take][:, i].astype(F) for i in range(4))
        ax, ay, az, aw = a
        P = lambda u, v: (u * v).astype(F)
        A = lambda u, v: (u + v).astype(F)
        S = lambda u, v: (u - v).astype(F)
        nx = S(A(A(P(aw, x), P(ax, w)), P(ay, z)), P(az, y))
        ny = A(A(S(P(aw, y), P(ax, z)), P(ay, w)), P(az, x))
        nz = A(S(A(P(aw, z), P(ax, y)), P(ay, x)), P(az, w))
        nw = S(S(S(P(aw, w), P(ax, x)), P(ay, y)), P(az, z))
        if prec:
            for k, v in zip(("rx", "ry", "rz", "rw"), (nx, ny, nz, nw)):
                out[k][take] = _f2h(v)
        else:
            out["rot"][take] = np.stack([nx, ny, nz, nw], 1)
        bands = BANDS[int(sh_components)]
        if not bands:
            return out, harm
        K = int(sh_components)
        h = np.asarray(harm).copy()
        rows = h.reshape(n, 3, K)   # (a view: writes go to h)
        for first, size in bands:
            D = d["sh%d" % ((size - 1) // 2)]
            for ch in range(3):
                c = rows[take, ch, first:first + size]
                c = _h2f(c) if prec else c.astype(F)
                o = _rows(D, c)
                rows[take, ch, first:first + size] = _f2h(o) if prec else o
    return out, h


# ---- the float64 derivation of a descriptor ----
def _directions(n=400, seed=0):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def band_matrix_f64(R, l):
    """D_l from its property: for every c and unit d, sum_k (D c)_k b_k(d) = sum_k c_k b_k(R^T d).  With the rows
    b(d_j) in B and b(R^T d_j) in B' (d_j @ R is (R^T d_j)^T), B D = B' in the least-squares sense over 400
    directions."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    d = _directions()
    lo, hi = l * l, (l + 1) * (l + 1)
    B = f64_model.sh_basis(d)[:, lo:hi]
    Bp = f64_model.sh_basis(d @ R)[:, lo:hi]
    D, *_ = np.linalg.lstsq(B, Bp, rcond=None)
    return D


def quaternion_f64(R):
    """(x, y, z, w), unit, w >= 0: the axis is the eigenvector of R at eigenvalue 1, the angle from the trace and the
    sense from the antisymmetric part.  At a half turn w is 0 and q and -q are the same rotation: the sign is then
    that of the axis component of largest magnitude, which the caller must not rely on."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    vals, vecs = np.linalg.eig(R)
    axis = np.real(vecs[:, np.argmin(np.abs(vals - 1.0))])
    axis /= np.linalg.norm(axis)
    anti = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])   # 2 sin(angle) axis
    sin_a = 0.5 * float(anti @ axis)
    cos_a = 0.5 * (np.trace(R) - 1.0)
    angle = np.arctan2(sin_a, cos_a)   # in (-pi, pi]: cos(angle / 2) >= 0
    q = np.append(np.sin(0.5 * angle) * axis, np.cos(0.5 * angle))
    if abs(q[3]) < 1e-9 and q[np.argmax(np.abs(q[:3]))] < 0:
        q = -q
    return q / np.linalg.norm(q)


def desc_f64(R, s, t):
    """the descriptor of (R, s, t) in float64: a dict with the keys of desc(), not rounded.  R, which may be float32
    values and so orthonormal only to 2^-24, stands for the rotation nearest to it."""
    U, _, Vt = np.linalg.svd(np.asarray(R, np.float64).reshape(3, 3))
    R = U @ Vt   # the rotation nearest to R (the helper reaches it by Newton steps)
    M = np.concatenate([float(s) * R, np.asarray(t, np.float64).reshape(3, 1)], 1)
    return dict(matrix=M.reshape(12), quaternion=quaternion_f64(R), scale=float(s),
                sh1=band_matrix_f64(R, 1).reshape(9), sh2=band_matrix_f64(R, 2).reshape(25),
                sh3=band_matrix_f64(R, 3).reshape(49))
