#!/usr/bin/env python3
"""Time K GlobalRenderer.render_frame calls against one render_frames of the same K descriptors.

One process, one handle, HIP events, interleaved blocks: (a) K sequential `render_frame` calls per frame, (b) one
`render_frames` per frame; 5 blocks of 40 frames each by default, medians of the per-frame block times.  The
yardstick for (b) is (a): the same build's single-descriptor entry with the same options.  Whole-frame and blend-stage
times; the stage times come from a profiled run of each afterwards (set_profiling stage events; the sequential
figure is the sum over the K calls).  The pick-only rows are also the cost of the union kernel -- the occluded pick
walk over the whole sorted runs -- against k_blend_px_pick's walk over the half-tile lists.
Writes profiles/frames_batch_timing.json.

    python tools/frames_timing.py [--blocks 5] [--frames 40] [--out profiles/frames_batch_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))

OPTION_SETS = ("occluder+pick+styles", "pick", "styles")
CASES = [  # (name, gaussians, sh components, width, height, precision, frames, option sets)
    ("50k_sh0_640x360_f32", 50_000, 1, 640, 360, 0, 4, OPTION_SETS),
    ("1m_sh3_1920x1080_f16_stereo", 1_000_000, 16, 1920, 1080, 1, 2, ("occluder+pick",)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_batch_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    results = []
    for name, n, sh, w, h, prec, k, option_sets in CASES:
        world_np, harm_np, _ = scenes.gen_scene(n, w, h, sh, prec, seed=42)
        world = torch.from_numpy(world_np.view(np.uint8).reshape(-1).copy()).cuda()
        harm = torch.from_numpy(harm_np.view(np.uint8).reshape(-1).copy()).cuda()
        inp = gsm_amd.GaussianInput(world, harm, n, sh)
        items = (n + 255) // 256 * 256
        cams = [gsm_amd.CameraParams.from_dict(scenes.orbit_camera(w, h, 3.0 * (i - (k - 1) / 2))) for i in range(k)]
        r = gsm_amd.GlobalRenderer(config=gsm_amd.RendererConfig(
            max_gaussians=k * items, max_width=w, max_height=k * ((h + 15) // 16 * 16), precision=prec,
            gaussian_color_space=0))
        color = torch.zeros((k, h, w, 4), dtype=torch.float16, device="cuda")
        depth = torch.zeros((k, h, w), dtype=torch.float16, device="cuda")
        pick = torch.zeros((k, h, w), dtype=torch.int32, device="cuda")
        # the surface: the median of view 0's own nonzero depths, nothing occluded on the left third
        r.render(color[0], depth[0], inp, cams[0], w, h)
        torch.cuda.synchronize()
        d = depth[0].float().cpu().numpy()
        occ_np = np.full((h, w), np.median(d[np.isfinite(d) & (d > 0)]), np.float32)
        occ_np[:, : w // 3] = np.inf
        occ = torch.from_numpy(occ_np).cuda()
        state = torch.from_numpy(np.random.default_rng(1).integers(0, 4, n).astype(np.uint8)).cuda()
        styles = [gsm_amd.Style(), gsm_amd.Style((255, 40, 0), 200, 255, False), gsm_amd.Style((0, 0, 0), 0, 90, False),
                  gsm_amd.Style((0, 0, 0), 0, 255, True)]
        for opts in option_sets:
            with_pick, with_occ, with_styles = "pick" in opts, "occluder" in opts, "styles" in opts
            frames = [gsm_amd.Frame((inp, cams[v]), w, h, color[v], depth[v], pick=pick[v] if with_pick else None,
                                    occluder=occ if with_occ else None, states=state if with_styles else None,
                                    styles=styles if with_styles else None) for v in range(k)]

            def seq():
                for f in frames:
                    r.render_frame(f.color, f.depth, f.objects, w, h, pick=f.pick, occluder=f.occluder, states=f.states,
                                   styles=f.styles)

            def batch():
                r.render_frames(frames)

            def block(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.frames):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / args.frames

            for _ in range(10):  # warm-up: schedules, caches, the lazy allocations
                seq()
                batch()
            torch.cuda.synchronize()
            ta, tb = [], []
            for _ in range(args.blocks):
                ta.append(block(seq))
                tb.append(block(batch))
            stages = {}
            for tag, fn in (("sequential", seq), ("frames", batch)):
                r.set_profiling(stage_events=True)
                for _ in range(16):
                    fn()
                torch.cuda.synchronize()
                stages[tag] = r.stage_times_ms()
                r.set_profiling(stage_events=False)
            batch()
            torch.cuda.synchronize()
            row = {"case": name, "frames": k, "options": opts, "sequential_ms": statistics.median(ta),
                   "frames_ms": statistics.median(tb), "sequential_blocks_ms": ta, "frames_blocks_ms": tb,
                   "blend_kernel": r.blend_kernel_kind(), "stage_ms_per_single_frame": stages["sequential"],
                   "stage_ms_per_batch": stages["frames"],
                   "sequential_blend_ms": k * stages["sequential"].get("blend", float("nan")),
                   "frames_blend_ms": stages["frames"].get("blend", float("nan"))}
            row["speedup"] = row["sequential_ms"] / row["frames_ms"]
            print(json.dumps({k_: row[k_] for k_ in ("case", "frames", "options", "sequential_ms", "frames_ms", "speedup",
                                                     "sequential_blend_ms", "frames_blend_ms")}), flush=True)
            results.append(row)
        r.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "frames_per_block": args.frames, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
