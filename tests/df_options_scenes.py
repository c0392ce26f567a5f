"""Hand-built scenes of the DepthFirst create-option tests (test_depthfirst_options.py).  Test data only."""
import numpy as np

# the grid of 65,792 tiles (257 x 256): one column of tiles past 4096 pixels, 257 ids past 16 bits
BIG_W, BIG_H = 4112, 4096


def cam(w, h):
    from gsm_amd import scenes
    return scenes.make_camera(w, h, 0.0)


def cams(w, h, ipd=0.064):
    from gsm_amd import scenes
    return scenes.make_camera(w, h, -ipd / 2), scenes.make_camera(w, h, ipd / 2)


def depth_ties(n=3000, w=160, h=128, seed=31):
    """n overlapping gaussians (f32 world, one SH component) around the image centre whose view depths are
    8 + k * 2^-12, k a permutation of the ids: about 32 consecutive depths share one fp16 value (the fp16
    ulp at 8 is 2^-7), and inside such a run the ascending-id order of the 16-bit sort is not the depth
    order.  Opacities of 0.3 .. 0.6 and random colours make the blend order visible."""
    from gsm_amd import scenes
    world, harm, _ = scenes.gen_scene(n, w, h, 1, 0, seed=seed, scale_px=4.0)
    rng = np.random.default_rng(seed + 1)
    z = (np.float32(8.0) + rng.permutation(n).astype(np.float32) * np.float32(2.0 ** -12)).astype(np.float32)
    world["pz"] = z
    world["px"] = (rng.uniform(-0.25, 0.25, n) * z).astype(np.float32)
    world["py"] = (rng.uniform(-0.25, 0.25, n) * z).astype(np.float32)
    world["opacity"] = rng.uniform(0.3, 0.6, n).astype(np.float32)
    return world, harm


def big_grid(seed=17):
    """A few hundred gaussians for the BIG_W x BIG_H grid: 128 along the bottom tile row (tile ids
    65,535 + tx, every second column), 128 along the top row at the columns those ids alias to when
    truncated to 16 bits (id - 65536 = tx - 1), and 100 anywhere.  About 3 pixels of sigma at depth 5."""
    from gsm_amd.types import WORLD32
    w, h, z = BIG_W, BIG_H, 5.0
    P = cam(w, h)["proj"]
    rng = np.random.default_rng(seed)
    k = np.arange(128)
    px = np.concatenate([16.0 * (2 * k + 2) + 8.0, 16.0 * (2 * k + 1) + 8.0, rng.uniform(0, w, 100)])
    py = np.concatenate([np.full(128, h - 8.0), np.full(128, 8.0), rng.uniform(0, h, 100)])
    n = len(px)
    world = np.zeros(n, WORLD32)
    world["rot"] = np.array([0, 0, 0, 1], np.float32)
    zz = (z + rng.uniform(-0.5, 0.5, n)).astype(np.float32)
    world["pz"] = zz
    world["px"] = ((2.0 * px / w - 1.0) * zz / float(P[0])).astype(np.float32)  # ndcToScreen: no half-pixel shift
    world["py"] = ((2.0 * py / h - 1.0) * zz / float(P[5])).astype(np.float32)
    s = 3.0 * zz / (h * float(P[5]) * 0.5)
    world["sx"] = world["sy"] = world["sz"] = s.astype(np.float32)
    world["opacity"] = rng.uniform(0.5, 0.9, n).astype(np.float32)
    harm = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32).reshape(-1)
    return world, harm


# gaussian counts of big_grid_dense at which a low-digit bucket of the two-pass tile sort starts exactly on
# a block boundary of its last pass (a multiple of 4096 instances); test_ref_dense_grid_spans_blocks asserts it
DENSE_N = {"mono": 2998, "stereo": 2999}


def big_grid_dense(n, seed=23, n_max=3200):
    """The first n of n_max gaussians (f32 world, one SH component, about 6 pixels of sigma at depth 5: rects of
    3 x 3 tiles and more) for the BIG_W x BIG_H grid, in shuffled order: a third in the two bottom tile rows
    (tile ids past 16 bits), a third in the two top rows (the ids those alias to), a third anywhere.  Tens of
    thousands of instances: every sort pass of the frame spans several workgroups."""
    from gsm_amd.types import WORLD32
    w, h, z = BIG_W, BIG_H, 5.0
    P = cam(w, h)["proj"]
    rng = np.random.default_rng(seed)
    third = n_max // 3
    px = rng.uniform(0, w, n_max)
    py = np.concatenate([rng.uniform(h - 32, h, third), rng.uniform(0, 32, third), rng.uniform(0, h, n_max - 2 * third)])
    perm = rng.permutation(n_max)
    px, py = px[perm], py[perm]
    world = np.zeros(n_max, WORLD32)
    world["rot"] = np.array([0, 0, 0, 1], np.float32)
    zz = (z + rng.uniform(-0.5, 0.5, n_max)).astype(np.float32)
    world["pz"] = zz
    world["px"] = ((2.0 * px / w - 1.0) * zz / float(P[0])).astype(np.float32)
    world["py"] = ((2.0 * py / h - 1.0) * zz / float(P[5])).astype(np.float32)
    s = rng.uniform(4.0, 8.0, n_max) * zz / (h * float(P[5]) * 0.5)
    world["sx"] = world["sy"] = world["sz"] = s.astype(np.float32)
    world["opacity"] = rng.uniform(0.5, 0.9, n_max).astype(np.float32)
    harm = rng.uniform(0.0, 1.0, (n_max, 3)).astype(np.float32)
    return world[:n].copy(), harm[:n].reshape(-1).copy()
