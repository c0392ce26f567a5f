#!/usr/bin/env python3
"""Times the DepthFirst mono frame (gsm_depthfirst_render) next to the Global frame of the same scene.

The benchmark's flagship scene (1M gaussians, SH3, 1920x1080, fp16, seed 42) by default.  In one
process: HIP events around --frames frames of each renderer after --warmup frames (interleaved in
blocks, so clock and thermal drift hit both alike), then the mono frame's per-stage times from
gsm_depthfirst_stage_times over a further profiled run.  Prints one JSON object; --out writes it
to a file as well (profiles/).

    python tools/df_mono_timing.py --out profiles/df_mono_timing.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2_1m_sh3_1080p_f16")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    c = scenes.CONFIGS[a.config]
    n, W, H, sh, prec = c["count"], c["width"], c["height"], c["sh"], c["precision"]
    world_np, harm_np, cam_d = scenes.gen_scene(n, W, H, sh, prec, seed=42)
    dev = torch.device("cuda", 0)
    world = torch.from_numpy(world_np.view(np.uint8).reshape(-1).copy()).to(dev)
    harm = torch.from_numpy(harm_np.view(np.uint8).reshape(-1).copy()).to(dev)
    inp = gsm_amd.GaussianInput(world, harm, n, sh)
    cam = gsm_amd.CameraParams.from_dict(cam_d)
    # the reference's default capacity (RendererConfig.maxGaussians = 6M): no instance is clamped
    cfg = gsm_amd.RendererConfig(max_gaussians=max(n, 6_000_000), max_width=W, max_height=H, precision=prec)
    mono = gsm_amd.DepthFirstRenderer(device=0, config=cfg)
    glob = gsm_amd.GlobalRenderer(device=0, config=cfg)
    color = torch.zeros((H, W, 4), dtype=torch.float16, device=dev)
    depth = torch.zeros((H, W), dtype=torch.float16, device=dev)

    def frame(r):
        r.render(color, depth, inp, cam, W, H)

    def timed(r, frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            frame(r)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames  # ms per frame

    for r in (mono, glob):
        for _ in range(a.warmup):
            frame(r)
    torch.cuda.synchronize()
    per = max(1, a.frames // a.blocks)
    ms = {"mono": [], "global": []}
    for _ in range(a.blocks):
        ms["mono"].append(timed(mono, per))
        ms["global"].append(timed(glob, per))
    mono_counters = mono.counters()
    assignments = glob.debug_read_total_assignments()

    mono.set_profiling(True)
    for _ in range(max(per, 50)):
        frame(mono)
    torch.cuda.synchronize()
    stages = mono.stage_times_ms()

    out = {
        "config": a.config, "gaussians": n, "width": W, "height": H, "sh_components": sh,
        "device": torch.cuda.get_device_name(0), "frames_per_block": per, "blocks": a.blocks, "warmup": a.warmup,
        "mono_ms_per_frame": {"median": statistics.median(ms["mono"]), "blocks": ms["mono"]},
        "global_ms_per_frame": {"median": statistics.median(ms["global"]), "blocks": ms["global"]},
        "mono_over_global": statistics.median(ms["mono"]) / statistics.median(ms["global"]),
        "mono_visible": mono_counters["visible"], "mono_instances": mono_counters["total_instances"],
        "mono_overflow": mono_counters["overflow"], "global_assignments": assignments,
        "mono_stage_ms": stages,
    }
    mono.close()
    glob.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
