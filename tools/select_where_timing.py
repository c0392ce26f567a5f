#!/usr/bin/env python3
"""Time GlobalRenderer.select_where and GlobalRenderer.state_bounds against a device-to-device copy of the bytes
each reads.

One process, one handle per precision, HIP events, interleaved blocks; 5 blocks of 40 calls each by default, medians
of the per-call block times.  1M gaussians, fp16 (32-byte records) and fp32 (48-byte records).  The select runs with
no shape and no range (the state test alone), with a rotated box, and with a box and both ranges; the bounds run over
the whole scene ({NULL, s}) and over a keep set of half the states.  The yardstick is not a fixed number: a torch
`copy_` (hipMemcpyAsync, device to device) of as many bytes as the entry reads -- the records as whole rows, since
memory moves whole lines, plus one state byte per gaussian where a state array is read -- in the same blocks.
Writes profiles/select_where_timing.json.

    python tools/select_where_timing.py [--blocks 5] [--calls 40] [--out profiles/select_where_timing.json]
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
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_where_timing.json"))
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

    a = np.radians(30.0)
    rot = np.array([[np.cos(a), np.sin(a), 0.0], [-np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    box = tuple(float(v) for v in scenes.box_to_shape((0.3, -0.2, 5.5), (1.5, 1.5, 2.0), rot))
    results = []
    for prec, name, record in ((1, "fp16", 32), (0, "fp32", 48)):
        world, _, _ = scenes.gen_scene(N, 1920, 1080, 1, prec, seed=42)
        dworld = torch.from_numpy(world.view(np.uint8).reshape(-1).copy()).cuda()
        rng = np.random.default_rng(prec)
        state = torch.from_numpy(rng.integers(0, 256, N).astype(np.uint8) & 0xFE).cuda()
        src = torch.zeros(N * (record + 1), dtype=torch.uint8, device="cuda")
        dst = torch.zeros(N * (record + 1), dtype=torch.uint8, device="cuda")
        matched = torch.zeros(1, dtype=torch.int32, device="cuda")
        bounds = torch.zeros(8, dtype=torch.int32, device="cuda")
        inp = gsm_amd.GaussianInput(dworld, None, N, 0)
        r = gsm_amd.GlobalRenderer(config=gsm_amd.RendererConfig(max_gaussians=N, max_width=64, max_height=64,
                                                                 precision=prec))
        queries = {"select_state_test_only": gsm_amd.SelectQuery(test_mask=0x80, test_value=0),
                   "select_box": gsm_amd.SelectQuery(gsm_amd.SELECT_BOX, 0, box),
                   "select_box_and_ranges": gsm_amd.SelectQuery(gsm_amd.SELECT_BOX, 0, box, opacity_min=0.6,
                                                                scale_max=0.01)}
        half_keep = gsm_amd.keep_masked(0x80, 0)
        fns = {k: (lambda q=q: r.select_where(inp, q, state, ~1, 1, matched=matched)) for k, q in queries.items()}
        # the same select without the count: no clear launch, no atomic per workgroup
        fns["select_box_no_count"] = lambda: r.select_where(inp, queries["select_box"], state, ~1, 1)
        fns["bounds_whole_scene"] = lambda: r.state_bounds(inp, 0, [0xFFFFFFFF] * 8, bounds)
        fns["bounds_keep_set"] = lambda: r.state_bounds(inp, state, half_keep, bounds)
        fns["copy_records_and_state"] = lambda: dst.copy_(src)
        fns["copy_records"] = lambda: dst[:N * record].copy_(src[:N * record])
        for _ in range(5):  # warm-up: the lazy allocations, caches
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.blocks):
            for k, fn in fns.items():
                times[k].append(block(fn))
        med = {k: statistics.median(t) for k, t in times.items()}
        row = {"gaussians": N, "precision": name, "record_bytes": record,
               "bytes_read": {"select": N * (record + 1), "bounds_whole_scene": N * record,
                              "bounds_keep_set": N * (record + 1)},
               "median_ms": med,
               "over_copy": {k: med[k] / med["copy_records" if k == "bounds_whole_scene" else "copy_records_and_state"]
                             for k in med if not k.startswith("copy")},
               "copy_gb_per_s": 2 * N * (record + 1) / (med["copy_records_and_state"] * 1e-3) / 1e9,
               "matched_last": int(matched.item()), "bounds_last": [int(v) for v in bounds.tolist()],
               "blocks_ms": times}
        print(json.dumps({"precision": name, "median_ms": med, "over_copy": row["over_copy"]}), flush=True)
        results.append(row)
        r.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "calls_per_block": args.calls,
                   "yardstick": "one torch copy_ (device to device) of the bytes the entry reads (whole records, plus "
                                "one state byte per gaussian where a state array is read), same session",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
