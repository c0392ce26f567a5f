"""Hand-built scenes and known-answer inputs of the LocalRenderer tests (test_local_ref.py on the CPU,
test_local.py on the GPU).  Test data only."""
import functools

import numpy as np

TILE = 16
MAX_PER_TILE = 2048


def cam(w, h):
    from gsm_amd import scenes
    return scenes.make_camera(w, h, 0.0)


def scene(n, w, h, sh, precision, seed, **kw):
    from gsm_amd import scenes
    world, harm, _ = scenes.gen_scene(n, w, h, sh, precision, seed=seed, **kw)
    return world, harm


def _world32(n):
    from gsm_amd.types import WORLD32
    w = np.zeros(n, WORLD32)
    w["rot"] = np.array([0, 0, 0, 1], np.float32)
    return w


def _pixel_to_world(px, py, z, w, h):
    """World x, y (identity view) whose ndcToScreenCentered position is the pixel (px, py)."""
    P = cam(w, h)["proj"]
    ndcx, ndcy = (2.0 * px + 1.0) / w - 1.0, (2.0 * py + 1.0) / h - 1.0
    return ndcx * z / float(P[0]), ndcy * z / float(P[5])


def _sigma_to_scale(sigma_px, z, h):
    P = cam(h, h)["proj"]
    return sigma_px * z / (h * float(P[5]) * 0.5)


def stack(k, w=64, h=64, centre=(23.5, 23.5), sigma_px=2.0, opacity=0.6, dc=0.5, others=0, seed=5):
    """k identical isotropic gaussians (same position, scale, rotation, opacity, SH) centred on `centre`
    -- inside tile (1, 1), 8 pixels from its edges, so the 3 sigma rect is that tile alone -- plus
    `others` distinct gaussians whose centres lie right of x = 44 (tiles of column 2 and 3 only).
    f32 world, one SH component."""
    z = 5.0
    world = _world32(k + others)
    harm = np.zeros((k + others, 3), np.float32)
    x, y = _pixel_to_world(centre[0], centre[1], z, w, h)
    world["px"][:k], world["py"][:k], world["pz"][:k] = x, y, z
    world["sx"][:k] = world["sy"][:k] = world["sz"][:k] = _sigma_to_scale(sigma_px, z, h)
    world["opacity"][:k] = opacity
    harm[:k] = dc
    if others:
        ow, oh = scene(others, w, h, 1, 0, seed)
        rng = np.random.default_rng(seed + 1)
        ow["px"] = (rng.uniform(0.32, 0.55, others) * ow["pz"]).astype(np.float32)
        ow["py"] = (rng.uniform(-0.5, 0.5, others) * ow["pz"]).astype(np.float32)
        world[k:] = ow
        harm[k:] = oh.reshape(others, 3)
    return world, harm.reshape(-1)


def plane(n, w, h, seed, z=5.0):
    """n gaussians at one view depth: every list is one run of equal depth16 (the tie-order contract)."""
    world, harm = scene(n, w, h, 1, 0, seed, scale_px=1.5)
    rng = np.random.default_rng(seed + 7)
    world["pz"] = np.float32(z)
    world["px"] = (rng.uniform(-0.55, 0.55, n) * z * w / h).astype(np.float32)
    world["py"] = (rng.uniform(-0.55, 0.55, n) * z).astype(np.float32)
    return world, harm


def nonfinite_colour(w=64, h=64, seed=11, background=400):
    """One gaussian whose SH DC makes half(colour) +inf, centred at (17.5, 17.5): near a corner of tile
    (1, 1), so some 4x2 groups of that tile and of its neighbours see eight zero alphas (they skip the
    entry and stay finite) and others do not (inf * 0 = NaN), over an ordinary background."""
    world, harm = stack(1, w, h, centre=(17.5, 17.5), sigma_px=2.0, opacity=0.9, dc=3.0e5, others=0)
    bw, bh = scene(background, w, h, 1, 0, seed)
    world = np.concatenate([bw, world])
    harm = np.concatenate([bh, harm])
    return world, harm


@functools.lru_cache(maxsize=None)
def kat_inputs(which):
    """The per-tile sort inputs of LocalUnitTests.swift:122-235: (keys16, indices, counts, max_per_tile)."""
    import oracle as O
    if which == "full":  # testPerTileSortCorrectness: srand48(42), 4 tiles x 64, every slot used
        tiles, mpt, counts, seed, fill = 4, 64, [64] * 4, 42, 0
    else:                # testPerTileSortVariableCounts: srand48(123), 8 tiles x 128
        tiles, mpt, counts, seed, fill = 8, 128, [10, 50, 5, 100, 25, 0, 75, 30], 123, 0xFFFF
    d = O.drand48_sequence(seed, sum(counts))
    keys = np.full(tiles * mpt, fill, np.uint16)
    idx = np.zeros(tiles * mpt, np.uint32)
    p = 0
    for t, c in enumerate(counts):
        for j in range(c):
            keys[t * mpt + j] = int(d[p] * 65535.0)  # UInt16(drand48() * 65535.0)
            idx[t * mpt + j] = t * mpt + j
            p += 1
    return keys, idx, np.array(counts, np.uint32), mpt


def kat_expected(keys, counts, mpt):
    """Per tile, the local indices ascending by (key, local index); slots past the count stay 0."""
    out = np.zeros(len(counts) * mpt, np.uint16)
    for t, c in enumerate(counts.tolist()):
        k = keys[t * mpt:t * mpt + c].astype(np.uint32)
        out[t * mpt:t * mpt + c] = np.argsort((k << 16) | np.arange(c, dtype=np.uint32), kind="stable")
    return out
