#!/usr/bin/env python3
"""Time GlobalRenderer.render_pick against `render` of the same scene on a handle of the same configuration.

Per workload one process, HIP events, interleaved blocks: (a) one `render` per frame, (b) one `render_pick` per
frame of the same input and camera on a second handle; 5 blocks of 40 frames each by default, medians of the
per-frame block times.  (a) is the floor: the pick frame does the same work up to the blend, and its blend walks
with more VALU work per entry, without compaction and without the pair walk.  Stage times come
from a profiled run of each afterwards, so the cost shows where it sits.  The driver itself never opens the GPU:
every workload runs in a fresh child process under its own time limit, and the first one that fails or runs out
of time ends the run.  Writes profiles/pick_timing.json.

    python tools/pick_timing.py [--blocks 5] [--frames 40] [--out profiles/pick_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))

# workloads: name -> (time limit in seconds, gaussians, sh components, precision, width, height, orbit angle or None)
WORKLOADS = {
    "1m_sh3_1080p_f16_fixed": (240, 1_000_000, 16, 1, 1920, 1080, None),
    "1m_sh3_1080p_f16_orbit_20deg": (240, 1_000_000, 16, 1, 1920, 1080, 20.0),
    "50k_sh0_640x360_f32_fixed": (120, 50_000, 1, 0, 640, 360, None),
}


def run_workload(name, blocks, frames):
    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    _, n, sh, prec, w, h, angle = WORKLOADS[name]
    world_np, harm_np, cam_d = scenes.gen_scene(n, w, h, sh, prec, seed=42)
    if angle is not None:
        cam_d = scenes.orbit_camera(w, h, angle)
    world = torch.from_numpy(world_np.view(np.uint8).reshape(-1).copy()).cuda()
    harm = torch.from_numpy(harm_np.view(np.uint8).reshape(-1).copy()).cuda()
    cfg = gsm_amd.RendererConfig(max_gaussians=n, max_width=w, max_height=h, precision=prec, gaussian_color_space=0)
    plain, pick = gsm_amd.GlobalRenderer(config=cfg), gsm_amd.GlobalRenderer(config=cfg)
    inp = gsm_amd.GaussianInput(world, harm, n, sh)
    cam = gsm_amd.CameraParams.from_dict(cam_d)
    tg = [(torch.zeros((h, w, 4), dtype=torch.float16, device="cuda"),
           torch.zeros((h, w), dtype=torch.float16, device="cuda")) for _ in range(2)]
    ptg = torch.zeros((h, w), dtype=torch.int32, device="cuda")

    def seq():
        plain.render(tg[0][0], tg[0][1], inp, cam, w, h)

    def one():
        pick.render_pick(tg[1][0], tg[1][1], ptg, inp, cam, w, h)

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames

    for _ in range(10):  # warm-up: schedules, caches
        seq()
        one()
    torch.cuda.synchronize()
    same = bool(torch.equal(tg[0][0], tg[1][0]) and torch.equal(tg[0][1], tg[1][1]))
    picked = float((ptg != -1).float().mean().item())
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(block(seq))
        tb.append(block(one))
    stages, kinds = {}, {}
    for tag, r, fn in (("render", plain, seq), ("render_pick", pick, one)):
        r.set_profiling(stage_events=True)
        for _ in range(16):
            fn()
        torch.cuda.synchronize()
        stages[tag] = r.stage_times_ms()
        kinds[tag] = r.blend_kernel_kind()
        r.set_profiling(stage_events=False)
    row = {"workload": name, "gaussians": n, "width": w, "height": h, "render_ms": statistics.median(ta),
           "render_pick_ms": statistics.median(tb), "render_blocks_ms": ta, "render_pick_blocks_ms": tb,
           "same_image": same, "picked_fraction": picked, "assignments": pick.debug_read_total_assignments(),
           "blend_kernel_render": kinds["render"], "blend_kernel_render_pick": kinds["render_pick"],
           "stage_ms_render": stages["render"], "stage_ms_render_pick": stages["render_pick"]}
    row["ratio"] = row["render_pick_ms"] / row["render_ms"]
    row["ratio_blocks"] = [b / a for a, b in zip(ta, tb)]
    plain.close()
    pick.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pick_timing.json"))
    ap.add_argument("--workload", help="run this one workload in this process and print its row")
    args = ap.parse_args()
    if args.workload:
        print(json.dumps(run_workload(args.workload, args.blocks, args.frames)), flush=True)
        return 0
    results = []
    for name, spec in WORKLOADS.items():
        limit = spec[0]
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", name, "--blocks",
                                str(args.blocks), "--frames", str(args.frames)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {limit} s; stopping", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{name}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        row = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps({k: row[k] for k in ("workload", "render_ms", "render_pick_ms", "ratio", "same_image")}),
              flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "frames_per_block": args.frames, "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
