#!/usr/bin/env python3
"""Time K sequential GlobalRenderer.render calls against one render_batch of the same K views.

Per workload one process, HIP events, interleaved blocks: (a) K sequential `render` calls per frame (the stereo
pair: one `render_stereo_sbs`), (b) one `render_batch` per frame; 5 blocks of 40 frames each by default, medians
of the per-frame block times.  The yardstick for (b) is (a): the same build's unchanged single frame.  Stage
times come from a profiled run of each afterwards (set_profiling stage events; for (a), of the first view's
handle).  The driver itself never opens
the GPU: every workload runs in a fresh child process under its own time limit, and the first one that fails or
runs out of time ends the run.  Writes profiles/batch_timing.json.

    python tools/batch_timing.py [--blocks 5] [--frames 40] [--out profiles/batch_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))

# scenes: name -> (gaussians, sh components, precision, the size the scene is generated for)
SCENES = {"50k": (50_000, 1, 0, (640, 360)), "1m": (1_000_000, 16, 1, (640, 360)),
          "1m_1080": (1_000_000, 16, 1, (1920, 1080)), "50k_f16": (50_000, 16, 1, (320, 180))}
# workloads: name -> (time limit in seconds, [(scene, width, height)] per view, side by side)
WORKLOADS = {
    "50k_sh0_640x360_f32_x2": (120, [("50k", 640, 360)] * 2, False),
    "50k_sh0_640x360_f32_x4": (120, [("50k", 640, 360)] * 4, False),
    "50k_sh0_640x360_f32_x8": (120, [("50k", 640, 360)] * 8, False),
    "1m_sh3_640x360_f16_x2": (240, [("1m", 640, 360)] * 2, False),
    "1m_sh3_640x360_f16_x4": (240, [("1m", 640, 360)] * 4, False),
    "mixed_1m_1080p_plus_4x50k_320x180_f16": (240, [("1m_1080", 1920, 1080)] + [("50k_f16", 320, 180)] * 4, False),
    "stereo_sbs_50k_640x360_f32": (120, [("50k", 640, 360)] * 2, True),
}


def run_workload(name, blocks, frames):
    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    _, spec, sbs = WORKLOADS[name]
    dev = {}
    for key in {s for s, _, _ in spec}:
        n, sh, prec, (gw, gh) = SCENES[key]
        world_np, harm_np, _ = scenes.gen_scene(n, gw, gh, sh, prec, seed=42)
        world = torch.from_numpy(world_np.view(np.uint8).reshape(-1).copy()).cuda()
        harm = torch.from_numpy(harm_np.view(np.uint8).reshape(-1).copy()).cuda()
        dev[key] = (gsm_amd.GaussianInput(world, harm, n, sh), n, prec)
    prec = dev[spec[0][0]][2]
    k = len(spec)
    cams = [gsm_amd.CameraParams.from_dict(scenes.orbit_camera(w, h, 3.0 * (i - (k - 1) / 2)))
            for i, (_, w, h) in enumerate(spec)]
    mw, mh = max(w for _, w, _ in spec), max(h for _, _, h in spec)
    tx = (mw + 31) // 32
    all_tiles = sum(((w + 31) // 32) * ((h + 15) // 16) for _, w, h in spec)
    # (a): one handle per distinct scene and size, as a caller of `render` would keep them (a handle that
    # alternates between sizes re-keys its blend schedule on every call)
    singles = {key: gsm_amd.GlobalRenderer(config=gsm_amd.RendererConfig(
        max_gaussians=dev[key[0]][1], max_width=key[1], max_height=key[2], precision=prec, gaussian_color_space=0))
        for key in set(spec)}
    single = singles[spec[0]]
    batch = gsm_amd.GlobalRenderer(config=gsm_amd.RendererConfig(
        max_gaussians=sum((dev[s][1] + 255) // 256 * 256 for s, _, _ in spec), max_width=mw,
        max_height=max(mh, 16 * ((all_tiles + tx - 1) // tx)), precision=prec, gaussian_color_space=0))
    if sbs:  # both eyes in one target, the right one width pixels into the rows
        w, h = spec[0][1], spec[0][2]
        color = torch.zeros((h, 2 * w, 4), dtype=torch.float16, device="cuda")
        depth = torch.zeros((h, 2 * w), dtype=torch.float16, device="cuda")
        views = [gsm_amd.BatchView(dev[spec[v][0]][0], cams[v], w, h, color.data_ptr() + v * w * 8,
                                   depth.data_ptr() + v * w * 2, color_pitch=2 * w * 8, depth_pitch=2 * w * 2)
                 for v in range(2)]

        def seq():
            single.render_stereo_sbs(color, depth, dev[spec[0][0]][0], cams[0], cams[1], w, h)
    else:
        tg = [(torch.zeros((h, w, 4), dtype=torch.float16, device="cuda"),
               torch.zeros((h, w), dtype=torch.float16, device="cuda")) for _, w, h in spec]
        views = [gsm_amd.BatchView(dev[s][0], cams[v], w, h, tg[v][0], tg[v][1]) for v, (s, w, h) in enumerate(spec)]

        def seq():
            for v, (s, w, h) in enumerate(spec):
                singles[(s, w, h)].render(tg[v][0], tg[v][1], dev[s][0], cams[v], w, h)

    def one():
        batch.render_batch(views)

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
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(block(seq))
        tb.append(block(one))
    stages = {}
    for tag, r, fn in (("sequential", single, seq), ("batch", batch, one)):
        r.set_profiling(stage_events=True)
        for _ in range(16):
            fn()
        torch.cuda.synchronize()
        stages[tag] = r.stage_times_ms()
        r.set_profiling(stage_events=False)
    row = {"workload": name, "views": k, "sequential_ms": statistics.median(ta), "batch_ms": statistics.median(tb),
           "sequential_blocks_ms": ta, "batch_blocks_ms": tb, "blend_kernel": batch.blend_kernel_kind(),
           "stage_ms_per_single_frame": stages["sequential"], "stage_ms_per_batch": stages["batch"]}
    row["speedup"] = row["sequential_ms"] / row["batch_ms"]
    for r in singles.values():
        r.close()
    batch.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_timing.json"))
    ap.add_argument("--workload", help="run this one workload in this process and print its row")
    args = ap.parse_args()
    if args.workload:
        print(json.dumps(run_workload(args.workload, args.blocks, args.frames)), flush=True)
        return 0
    results = []
    for name, (limit, _, _) in WORKLOADS.items():
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
        print(json.dumps({k: row[k] for k in ("workload", "views", "sequential_ms", "batch_ms", "speedup")}), flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "frames_per_block": args.frames, "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
