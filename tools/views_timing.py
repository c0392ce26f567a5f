#!/usr/bin/env python3
"""Time K sequential GlobalRenderer.render calls against one render_views of the same K cameras.

One process, HIP events, interleaved blocks: (a) K sequential `render` calls per frame, (b) one
`render_views` per frame; 5 blocks of 40 frames each by default, medians of the per-frame block times.
The yardstick for (b) is (a): the same build's unchanged single frame.  Stage times come from a
profiled run of each afterwards (set_profiling stage events).  Writes profiles/views_timing.json.

    python tools/views_timing.py [--blocks 5] [--frames 40] [--out profiles/views_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))

CASES = [  # (name, gaussians, sh components, width, height, precision, view counts, blend kernel to expect or None)
    ("50k_sh0_640x360_f32", 50_000, 1, 640, 360, 0, (2, 4, 8), None),
    ("1m_sh3_640x360_f16", 1_000_000, 16, 640, 360, 1, (2, 4), None),
    # 27 x 460 tiles: the batch takes the pair walk (blend_kernel_kind() 3), which no other workload reaches
    ("20k_sh0_640x360_f32", 20_000, 1, 640, 360, 0, (27,), 3),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    results = []
    for name, n, sh, w, h, prec, ks, kind in CASES:
        world_np, harm_np, _ = scenes.gen_scene(n, w, h, sh, prec, seed=42)
        world = torch.from_numpy(world_np.view(np.uint8).reshape(-1).copy()).cuda()
        harm = torch.from_numpy(harm_np.view(np.uint8).reshape(-1).copy()).cuda()
        inp = gsm_amd.GaussianInput(world, harm, n, sh)
        items = (n + 255) // 256 * 256
        for k in ks:
            cams = [gsm_amd.CameraParams.from_dict(scenes.orbit_camera(w, h, 3.0 * (i - (k - 1) / 2))) for i in range(k)]
            single = gsm_amd.GlobalRenderer(config=gsm_amd.RendererConfig(
                max_gaussians=n, max_width=w, max_height=h, precision=prec, gaussian_color_space=0))
            batch = gsm_amd.GlobalRenderer(config=gsm_amd.RendererConfig(
                max_gaussians=k * items, max_width=w, max_height=k * ((h + 15) // 16 * 16), precision=prec,
                gaussian_color_space=0))
            color = torch.zeros((k, h, w, 4), dtype=torch.float16, device="cuda")
            depth = torch.zeros((k, h, w), dtype=torch.float16, device="cuda")

            def seq():
                for v in range(k):
                    single.render(color[v], depth[v], inp, cams[v], w, h)

            def views():
                batch.render_views(color, depth, inp, cams, w, h)

            def block(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.frames):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / args.frames

            for _ in range(10):  # warm-up: schedules, caches
                seq()
                views()
            torch.cuda.synchronize()
            if kind is not None and batch.blend_kernel_kind() != kind:
                raise SystemExit(f"{name} x{k}: blend kernel {batch.blend_kernel_kind()}, expected {kind}")
            ta, tb = [], []
            for _ in range(args.blocks):
                ta.append(block(seq))
                tb.append(block(views))
            stages = {}
            for tag, r, fn in (("sequential", single, seq), ("views", batch, views)):
                r.set_profiling(stage_events=True)
                for _ in range(16):
                    fn()
                torch.cuda.synchronize()
                stages[tag] = r.stage_times_ms()
                r.set_profiling(stage_events=False)
            row = {"case": name, "views": k, "sequential_ms": statistics.median(ta), "views_ms": statistics.median(tb),
                   "sequential_blocks_ms": ta, "views_blocks_ms": tb, "blend_kernel": batch.blend_kernel_kind(),
                   "stage_ms_per_single_frame": stages["sequential"], "stage_ms_per_batch": stages["views"]}
            row["speedup"] = row["sequential_ms"] / row["views_ms"]
            print(json.dumps({k_: row[k_] for k_ in ("case", "views", "sequential_ms", "views_ms", "speedup")}), flush=True)
            results.append(row)
            single.close()
            batch.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "frames_per_block": args.frames, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
