#!/usr/bin/env python3
"""Time GlobalRenderer.transform against a device-to-device copy of the bytes it moves.

One process, one handle per case, HIP events, interleaved blocks; 5 blocks of 20 calls each by default, medians of the
per-call block times.  1M gaussians: fp16 records with 16 harmonics components (32 + 96 bytes a gaussian) and fp32
records with one (48 bytes; the harmonics are not touched), each over the whole scene ({NULL, s}) and over a keep set
of half the states.  The pose is a rotation with a scale of 1 and no translation, so that repeated calls keep the
values in range.  The yardstick is not a fixed number: a torch `copy_` (hipMemcpyAsync, device to device) of as many
bytes as the whole-scene call reads, which is also what it writes, in the same blocks.  The half keep set touches
about half the rows, scattered; it is reported against the same whole-scene copy.
Writes profiles/transform_timing.json.

    python tools/transform_timing.py [--blocks 5] [--calls 20] [--out profiles/transform_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))

N = 1_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls

    a, b = np.radians(30.0), 0.4
    rot = np.array([[np.cos(a), np.sin(a), 0.0], [-np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rot = rot @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), np.sin(b)], [0.0, -np.sin(b), np.cos(b)]])
    pose = gsm_amd.Transform.from_pose(rot, 1.0, (0.0, 0.0, 0.0))
    results = []
    for prec, sh, name in ((1, 16, "fp16_sh3"), (0, 1, "fp32_sh0")):
        world, harm, _ = scenes.gen_scene(N, 1920, 1080, sh, prec, seed=42)
        dworld = torch.from_numpy(world.view(np.uint8).reshape(-1).copy()).cuda()
        dharm = torch.from_numpy(np.asarray(harm).view(np.uint8).reshape(-1).copy()).cuda()
        record = world.dtype.itemsize
        row_bytes = 3 * sh * (2 if prec else 4) if sh > 1 else 0
        moved = N * (record + row_bytes)
        state = torch.from_numpy(np.random.default_rng(prec).integers(0, 256, N).astype(np.uint8)).cuda()
        half_keep = gsm_amd.keep_masked(0x80, 0)
        src = torch.zeros(moved, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(moved, dtype=torch.uint8, device="cuda")
        r = gsm_amd.GlobalRenderer(config=gsm_amd.RendererConfig(max_gaussians=N, max_width=64, max_height=64,
                                                                 precision=prec))
        fns = {"transform_whole_scene": lambda: r.transform(dworld, dharm, N, sh, 0, [0xFFFFFFFF] * 8, pose),
               "transform_half_keep_set": lambda: r.transform(dworld, dharm, N, sh, state, half_keep, pose),
               "copy_same_bytes": lambda: dst.copy_(src)}
        for _ in range(3):  # warm-up
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.blocks):
            for k, fn in fns.items():
                times[k].append(block(fn))
        med = {k: statistics.median(t) for k, t in times.items()}
        row = {"gaussians": N, "case": name, "record_bytes": record, "harmonics_row_bytes": row_bytes,
               "bytes_read_whole_scene": moved, "bytes_written_whole_scene": moved, "median_ms": med,
               "over_copy": {k: med[k] / med["copy_same_bytes"] for k in med if not k.startswith("copy")},
               "copy_gb_per_s": 2 * moved / (med["copy_same_bytes"] * 1e-3) / 1e9,
               "transform_gb_per_s": 2 * moved / (med["transform_whole_scene"] * 1e-3) / 1e9,
               "blocks_ms": times}
        print(json.dumps({"case": name, "median_ms": med, "over_copy": row["over_copy"]}), flush=True)
        results.append(row)
        r.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "calls_per_block": args.calls,
                   "yardstick": "one torch copy_ (device to device) of the bytes the whole-scene call reads (the "
                                "records, and the harmonics rows where they are rotated), same session",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
