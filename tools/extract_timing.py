#!/usr/bin/env python3
"""Time GlobalRenderer.extract against a device-to-device copy of the bytes it moves.

One process, one handle, HIP events, interleaved blocks; 5 blocks of 40 calls each by default, medians of the
per-call block times.  1M gaussians, SH3, fp16 (32-byte records, 96-byte harmonics rows), keeping 1 %, 50 % and 99 %
at random.  The yardstick is not a fixed number: a torch `copy_` (hipMemcpyAsync, device to device) of as many bytes
as the extract reads plus writes, over the same buffers, in the same blocks; a second copy of half as many bytes --
the one whose own traffic, read plus written, equals the extract's -- is recorded beside it.  The split between the
launches comes from the same extract at capacity 0, which runs the count and the scan and skips the move.
Writes profiles/extract_timing.json.

    python tools/extract_timing.py [--blocks 5] [--calls 40] [--out profiles/extract_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))

N, SH, PREC = 1_000_000, 16, 1
RECORD, ROW = 32, 96
FRACTIONS = (0.01, 0.5, 0.99)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import gsm_amd

    rng = np.random.default_rng(42)
    # one flat source (records | harmonics) and one flat destination (records | harmonics | state | ids): the
    # extract's pointers are slices of them, and the yardstick copies run over the same two buffers
    # (both are long enough for the largest yardstick, so that every yardstick is one copy, one launch)
    span = 2 * N * (RECORD + ROW + 1 + 4) + (1 << 16)
    src = torch.zeros(span, dtype=torch.uint8, device="cuda")
    src[:N * (RECORD + ROW)] = torch.from_numpy(rng.integers(0, 256, N * (RECORD + ROW), dtype=np.uint8)).cuda()
    dst = torch.zeros(span, dtype=torch.uint8, device="cuda")
    recs, harm = src[:N * RECORD], src[N * RECORD:N * (RECORD + ROW)]
    o_recs, o_harm = dst[:N * RECORD], dst[N * RECORD:N * (RECORD + ROW)]
    o_state = dst[N * (RECORD + ROW):N * (RECORD + ROW + 1)]
    o_ids = dst[N * (RECORD + ROW + 1):N * (RECORD + ROW + 1 + 4)]
    kept = torch.zeros(1, dtype=torch.int32, device="cuda")
    keep = gsm_amd.keep_masked(1, 1)
    inp = gsm_amd.GaussianInput(recs, harm, N, SH)
    r = gsm_amd.GlobalRenderer(config=gsm_amd.RendererConfig(max_gaussians=N, max_width=64, max_height=64,
                                                             precision=PREC))

    def copy_bytes(nbytes):
        assert nbytes <= span
        dst[:nbytes].copy_(src[:nbytes])

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls

    results = []
    for p in FRACTIONS:
        state_np = (rng.integers(0, 128, N) * 2 + (rng.random(N) < p)).astype(np.uint8)
        state = torch.from_numpy(state_np).cuda()
        K = int((state_np & 1).sum())
        blocks = (N + 255) // 256
        # read: the state bytes twice (count, move), the kept rows, the block words twice; written: the kept rows with
        # their state byte and id, the block words twice, the count
        read = 2 * N + K * (RECORD + ROW) + 2 * 4 * blocks
        written = K * (RECORD + ROW + 1 + 4) + 2 * 4 * blocks + 4
        moved = read + written

        def full():
            r.extract(inp, state, keep, o_recs, o_harm, o_state, o_ids, capacity=N, kept=kept)

        def count_and_scan():
            r.extract(inp, state, keep, o_recs, o_harm, o_state, o_ids, capacity=0, kept=kept)

        def copy_moved():
            copy_bytes(moved)

        def copy_half():
            copy_bytes(moved // 2)

        fns = (full, count_and_scan, copy_moved, copy_half)
        for _ in range(5):  # warm-up: the lazy allocation, caches
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        assert int(kept.item()) == K
        times = [[] for _ in fns]
        for _ in range(args.blocks):
            for t, fn in zip(times, fns):
                t.append(block(fn))
        med = [statistics.median(t) for t in times]
        row = {"gaussians": N, "sh_components": SH, "precision": "fp16", "kept_fraction": p, "kept": K,
               "bytes_read": read, "bytes_written": written,
               "extract_ms": med[0], "count_and_scan_ms": med[1], "move_ms": med[0] - med[1],
               "copy_of_moved_bytes_ms": med[2], "copy_of_half_ms": med[3],
               "extract_over_copy_of_moved_bytes": med[0] / med[2], "extract_over_copy_of_half": med[0] / med[3],
               "extract_gb_per_s": moved / (med[0] * 1e-3) / 1e9,
               "copy_gb_per_s": 2 * moved / (med[2] * 1e-3) / 1e9,
               "blocks_ms": {fn.__name__: t for fn, t in zip(fns, times)}}
        print(json.dumps({k: row[k] for k in ("kept_fraction", "kept", "extract_ms", "count_and_scan_ms", "move_ms",
                                              "copy_of_moved_bytes_ms", "copy_of_half_ms",
                                              "extract_over_copy_of_moved_bytes", "extract_over_copy_of_half")}),
              flush=True)
        results.append(row)
    r.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "calls_per_block": args.calls,
                   "yardstick": "one torch copy_ (device to device) of bytes_read + bytes_written bytes over the same "
                                "buffers, same session; copy_of_half: half as many bytes, so equal traffic",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
