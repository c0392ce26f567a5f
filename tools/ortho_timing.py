#!/usr/bin/env python3
"""Time the orthographic Global frame (GSM_FRAME_ORTHOGRAPHIC) against the perspective one.

Per workload one process, HIP events, interleaved blocks, each leg on a handle of its own: (a) one perspective
`render_frame` per frame; (b) one orthographic `render_frame` of the same scene, framed -- the half height of the view
volume is chosen from a scan, before anything is timed -- so that its assignment count is as close to (a)'s as the
scan gets (both counts are reported); (c) the quad view, one `render_frames` of one perspective and three orthographic
views; (d) the same four views as four `render_frame` calls on one handle.  5 blocks of 40 frames each by default,
medians of the per-frame block times.  The stage times, the projection among them, come from a profiled run of (a) and
(b) afterwards.  No number here is a target.  The driver itself never opens the GPU: every workload runs in a fresh
child process under its own time limit, and the first one that fails or runs out of time ends the run.  Writes
profiles/ortho_timing.json.

    python tools/ortho_timing.py [--blocks 5] [--frames 40] [--out profiles/ortho_timing.json]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))

# workloads: name -> (time limit in seconds, gaussians, sh components, precision, width, height)
WORKLOADS = {
    "1m_sh3_1080p_f16": (400, 1_000_000, 16, 1, 1920, 1080),
    "50k_sh0_640x360_f32": (150, 50_000, 1, 0, 640, 360),
}


def turned(scenes, w, h, half_height, angle):
    """ortho_camera turned by `angle` about the y axis through the cloud's middle (0, 0, 5.5)."""
    import numpy as np
    c, s = np.float32(math.cos(angle)), np.float32(math.sin(angle))
    V = np.eye(4, dtype=np.float32)
    V[0, 0], V[0, 2], V[2, 0], V[2, 2] = c, s, -s, c
    pivot = np.array([0, 0, 5.5], np.float32)
    V[:3, 3] = pivot - V[:3, :3] @ pivot
    return scenes.ortho_camera(w, h, half_height, view=V.T.reshape(-1))


def run_workload(name, blocks, frames):
    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    _, n, sh, prec, w, h = WORKLOADS[name]
    world_np, harm_np, cam_d = scenes.gen_scene(n, w, h, sh, prec, seed=42)
    world = torch.from_numpy(world_np.view(np.uint8).reshape(-1).copy()).cuda()
    harm = torch.from_numpy(harm_np.view(np.uint8).reshape(-1).copy()).cuda()
    cfg = gsm_amd.RendererConfig(max_gaussians=n, max_width=w, max_height=h, precision=prec, gaussian_color_space=0)
    padded = (n + 255) // 256 * 256
    # (a handle whose tile space holds four views: each view's rows round up to whole tiles)
    quad_cfg = gsm_amd.RendererConfig(max_gaussians=4 * padded, max_width=2 * ((w + 31) // 32 * 32),
                                      max_height=2 * ((h + 15) // 16 * 16), precision=prec, gaussian_color_space=0)
    inp = gsm_amd.GaussianInput(world, harm, n, sh)
    pcam = gsm_amd.CameraParams.from_dict(cam_d)

    def target():
        return (torch.zeros((h, w, 4), dtype=torch.float16, device="cuda"),
                torch.zeros((h, w), dtype=torch.float16, device="cuda"))

    # the framing of (b): the half height whose assignment count is closest to the perspective frame's
    probe = gsm_amd.GlobalRenderer(config=cfg)
    pc, pd = target()
    probe.render_frame(pc, pd, (inp, pcam), w, h)
    torch.cuda.synchronize()
    want = probe.debug_read_total_assignments()
    scan = []
    for k in range(25):
        hh = 1.0 * (8.0 ** (k / 24.0))
        probe.render_frame(pc, pd, (inp, gsm_amd.CameraParams.from_dict(scenes.ortho_camera(w, h, hh))), w, h,
                           orthographic=True)
        torch.cuda.synchronize()
        c = probe.counters()
        if not c["overflow"]:
            scan.append((abs(c["total_assignments"] - want), hh, c["total_assignments"]))
    probe.close()
    _, half_height, _ = min(scan)
    ocam = gsm_amd.CameraParams.from_dict(scenes.ortho_camera(w, h, half_height))
    quad_cams = [pcam, ocam, gsm_amd.CameraParams.from_dict(turned(scenes, w, h, half_height, math.pi / 2)),
                 gsm_amd.CameraParams.from_dict(turned(scenes, w, h, half_height, -0.4))]
    quad_ortho = [False, True, True, True]

    rs = [gsm_amd.GlobalRenderer(config=cfg), gsm_amd.GlobalRenderer(config=cfg),
          gsm_amd.GlobalRenderer(config=quad_cfg), gsm_amd.GlobalRenderer(config=quad_cfg)]
    ta, tb = target(), target()
    tq, ts = [target() for _ in range(4)], [target() for _ in range(4)]
    quad_frames = [gsm_amd.Frame((inp, c), w, h, t[0], t[1], orthographic=o)
                   for c, t, o in zip(quad_cams, tq, quad_ortho)]

    def persp():
        rs[0].render_frame(ta[0], ta[1], (inp, pcam), w, h)

    def ortho():
        rs[1].render_frame(tb[0], tb[1], (inp, ocam), w, h, orthographic=True)

    def quad():
        rs[2].render_frames(quad_frames)

    def four():
        for c, t, o in zip(quad_cams, ts, quad_ortho):
            rs[3].render_frame(t[0], t[1], (inp, c), w, h, orthographic=o)

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames

    fns = (("perspective", persp), ("orthographic", ortho), ("quad_batch", quad), ("quad_four_calls", four))
    for _ in range(10):  # warm-up: schedules, caches
        for _, fn in fns:
            fn()
    torch.cuda.synchronize()
    quad_same = all(bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])) for a, b in zip(tq, ts))
    times = {tag: [] for tag, _ in fns}
    for _ in range(blocks):
        for tag, fn in fns:
            times[tag].append(block(fn))
    row = {"workload": name, "gaussians": n, "width": w, "height": h, "half_height": half_height,
           "quad_batch_equals_four_calls": quad_same}
    for (tag, fn), r in zip(fns, rs):
        row[tag + "_ms"] = statistics.median(times[tag])
        row[tag + "_blocks_ms"] = times[tag]
        if tag in ("perspective", "orthographic", "quad_batch"):
            r.set_profiling(stage_events=True)
            for _ in range(16):
                fn()
            torch.cuda.synchronize()
            row["stage_ms_" + tag] = r.stage_times_ms()
            row["assignments_" + tag] = r.debug_read_total_assignments()
            r.set_profiling(stage_events=False)
    row["assignments_ratio"] = row["assignments_orthographic"] / max(row["assignments_perspective"], 1)
    row["ratio_orthographic"] = row["orthographic_ms"] / row["perspective_ms"]
    row["ratio_project_stage"] = row["stage_ms_orthographic"]["project"] / row["stage_ms_perspective"]["project"]
    row["ratio_quad"] = row["quad_batch_ms"] / row["quad_four_calls_ms"]
    for r in rs:
        r.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ortho_timing.json"))
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
        print(json.dumps({k: row[k] for k in ("workload", "perspective_ms", "orthographic_ms", "quad_batch_ms",
                                              "quad_four_calls_ms", "assignments_perspective",
                                              "assignments_orthographic", "ratio_project_stage",
                                              "quad_batch_equals_four_calls")}), flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "frames_per_block": args.frames, "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
