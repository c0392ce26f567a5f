#!/usr/bin/env python3
"""Time GlobalRenderer.render_occluded against `render` of the same scene on handles of the same configuration.

Per workload one process, HIP events, interleaved blocks of four legs, each on a handle of its own:
(a) `render`; (b) `render_occluded` under an occluder of all +inf -- the price of the instance: the same image
(checked), the walk without compaction and without the pair walk, plus the cut's packed operations per entry
(DESIGN.md 21); (c) a plane at the median visible depth over the left half of the image, +inf on the right;
(d) the same plane over the whole image.  The median visible depth is taken from leg (a)'s own targets: the
median, over the pixels with alpha above one half, of the blended depth divided by alpha.  5 blocks of 40 frames
each by default, medians of the per-frame block times and the blocks' range.  Stage times come from a profiled
run of each leg afterwards, so a difference shows where it sits.  The driver itself never opens the GPU: every
workload runs in a fresh child process under its own time limit, and the first one that fails or runs out of
time ends the run.  Writes profiles/occluded_timing.json.

    python tools/occluded_timing.py [--blocks 5] [--frames 40] [--out profiles/occluded_timing.json]
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
    "1m_sh3_1080p_f16_fixed": (300, 1_000_000, 16, 1, 1920, 1080, None),
    "1m_sh3_1080p_f16_orbit_20deg": (300, 1_000_000, 16, 1, 1920, 1080, 20.0),
    "50k_sh0_640x360_f32_fixed": (120, 50_000, 1, 0, 640, 360, None),
}
LEGS = ("render", "occluded_inf", "occluded_left_half", "occluded_whole")


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
    handles = {leg: gsm_amd.GlobalRenderer(config=cfg) for leg in LEGS}
    inp = gsm_amd.GaussianInput(world, harm, n, sh)
    cam = gsm_amd.CameraParams.from_dict(cam_d)
    tg = {leg: (torch.zeros((h, w, 4), dtype=torch.float16, device="cuda"),
                torch.zeros((h, w), dtype=torch.float16, device="cuda")) for leg in LEGS}

    handles["render"].render(tg["render"][0], tg["render"][1], inp, cam, w, h)
    torch.cuda.synchronize()
    alpha, dep = tg["render"][0][..., 3].float(), tg["render"][1].float()
    solid = alpha > 0.5
    plane = float((dep[solid] / alpha[solid]).median().item())
    occ = {"occluded_inf": torch.full((h, w), float("inf"), dtype=torch.float32, device="cuda"),
           "occluded_left_half": torch.full((h, w), float("inf"), dtype=torch.float32, device="cuda"),
           "occluded_whole": torch.full((h, w), plane, dtype=torch.float32, device="cuda")}
    occ["occluded_left_half"][:, :w // 2] = plane

    def frame(leg):
        if leg == "render":
            return lambda: handles[leg].render(tg[leg][0], tg[leg][1], inp, cam, w, h)
        return lambda: handles[leg].render_occluded(tg[leg][0], tg[leg][1], occ[leg], inp, cam, w, h)

    fns = {leg: frame(leg) for leg in LEGS}

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames

    for _ in range(10):  # warm-up: schedules, caches
        for leg in LEGS:
            fns[leg]()
    torch.cuda.synchronize()
    same = bool(torch.equal(tg["render"][0].view(torch.int16), tg["occluded_inf"][0].view(torch.int16)) and
                torch.equal(tg["render"][1].view(torch.int16), tg["occluded_inf"][1].view(torch.int16)))
    if not same:
        raise SystemExit(f"{name}: render_occluded under +inf differs from render")
    changed = {leg: float((tg[leg][0].view(torch.int16) != tg["render"][0].view(torch.int16)).any(dim=2)
                          .float().mean().item()) for leg in LEGS[2:]}
    times = {leg: [] for leg in LEGS}
    for _ in range(blocks):
        for leg in LEGS:
            times[leg].append(block(fns[leg]))
    stages, kinds = {}, {}
    for leg in LEGS:
        r = handles[leg]
        r.set_profiling(stage_events=True)
        for _ in range(16):
            fns[leg]()
        torch.cuda.synchronize()
        stages[leg] = r.stage_times_ms()
        kinds[leg] = r.blend_kernel_kind()
        r.set_profiling(stage_events=False)
    row = {"workload": name, "gaussians": n, "width": w, "height": h, "plane_depth": plane,
           "same_image_under_inf": same, "changed_pixel_fraction": changed,
           "assignments": handles["render"].debug_read_total_assignments(),
           "ms": {leg: statistics.median(times[leg]) for leg in LEGS},
           "blocks_ms": times,
           "blocks_range_ms": {leg: [min(times[leg]), max(times[leg])] for leg in LEGS},
           "blend_kernel": kinds, "stage_ms": stages}
    row["ratio_to_render"] = {leg: row["ms"][leg] / row["ms"]["render"] for leg in LEGS[1:]}
    for r in handles.values():
        r.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occluded_timing.json"))
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
        print(json.dumps({"workload": row["workload"], "ms": row["ms"], "ratio_to_render": row["ratio_to_render"]}),
              flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "frames_per_block": args.frames, "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
