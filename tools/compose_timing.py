#!/usr/bin/env python3
"""Time GlobalRenderer.render_composite against `render` of the same gaussians pre-merged into one buffer.

Per workload one process, HIP events, interleaved blocks: (a) one `render` per frame of the merged buffer under
the frame's camera, (b) one `render_composite` per frame of the same buffer cut into K objects (contiguous id
ranges), each under its own pose; 5 blocks of 40 frames each by default, medians of the per-frame block times.
(a) is the floor: the composite does the same work plus the padding of every object to whole 256-item blocks and
one lookup per block.  With identity poses the two frames are the same image; with distinct poses (small
similarity transforms about the scene's centre) the composite shows moved objects, so its visible set differs a
little from (a)'s.  Stage times come from a profiled run of each afterwards.  The driver itself never opens the
GPU: every workload runs in a fresh child process under its own time limit, and the first one that fails or runs
out of time ends the run.  Writes profiles/compose_timing.json.

    python tools/compose_timing.py [--blocks 5] [--frames 40] [--out profiles/compose_timing.json]
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

# workloads: name -> (time limit in seconds, gaussians, sh components, precision, width, height, objects, posed)
WORKLOADS = {}
for _k in (1, 4, 16):
    WORKLOADS[f"1m_sh3_1080p_f16_{_k}_objects_identity"] = (240, 1_000_000, 16, 1, 1920, 1080, _k, False)
for _k in (1, 4, 16):
    WORKLOADS[f"1m_sh3_1080p_f16_{_k}_objects_posed"] = (240, 1_000_000, 16, 1, 1920, 1080, _k, True)
WORKLOADS["4x50k_sh0_640x360_f32_identity"] = (120, 200_000, 1, 0, 640, 360, 4, False)
WORKLOADS["4x50k_sh0_640x360_f32_posed"] = (120, 200_000, 1, 0, 640, 360, 4, True)


def pose(i, pivot=(0.0, 0.0, 5.5)):
    """Object i's model matrix, 4x4 column-major flat: a few degrees about an axis through the pivot, a uniform
    scale within 10 % and a shift of up to 0.2, all fixed functions of i."""
    import numpy as np
    a = math.radians(2.0 + 6.0 * ((i * 5) % 7) / 6.0) * (1 if i % 2 else -1)
    k = np.array([math.sin(1.0 + i), math.cos(2.0 + 3 * i), math.sin(0.5 + 7 * i)])
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    s = 0.9 + 0.2 * ((i * 3) % 5) / 4.0
    t = 0.2 * np.array([math.sin(3.0 * i), math.cos(5.0 * i), math.sin(11.0 * i)])
    p = np.asarray(pivot)
    M = np.eye(4)
    M[:3, :3] = s * R
    M[:3, 3] = p - s * R @ p + t
    return M.T.reshape(-1)


def run_workload(name, blocks, frames):
    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    _, n, sh, prec, w, h, k, posed = WORKLOADS[name]
    world_np, harm_np, cam_d = scenes.gen_scene(n, w, h, sh, prec, seed=42)
    world = torch.from_numpy(world_np.view(np.uint8).reshape(-1).copy()).cuda()
    harm = torch.from_numpy(harm_np.view(np.uint8).reshape(-1).copy()).cuda()
    wbytes, hbytes = world_np.dtype.itemsize, harm_np.dtype.itemsize * 3 * sh
    cuts = [n * i // k for i in range(k + 1)]
    objects = []
    for i in range(k):
        cam = scenes.object_camera(cam_d, pose(i)) if posed else cam_d
        inp = gsm_amd.GaussianInput(world.data_ptr() + cuts[i] * wbytes, harm.data_ptr() + cuts[i] * hbytes,
                                    cuts[i + 1] - cuts[i], sh)
        objects.append(gsm_amd.SceneObject(inp, gsm_amd.CameraParams.from_dict(cam)))
    items = sum((cuts[i + 1] - cuts[i] + 255) // 256 * 256 for i in range(k))
    cfg = gsm_amd.RendererConfig(max_gaussians=items, max_width=w, max_height=h, precision=prec,
                                 gaussian_color_space=0)
    merged, comp = gsm_amd.GlobalRenderer(config=cfg), gsm_amd.GlobalRenderer(config=cfg)
    whole = gsm_amd.GaussianInput(world, harm, n, sh)
    cam = gsm_amd.CameraParams.from_dict(cam_d)
    tg = [(torch.zeros((h, w, 4), dtype=torch.float16, device="cuda"),
           torch.zeros((h, w), dtype=torch.float16, device="cuda")) for _ in range(2)]

    def seq():
        merged.render(tg[0][0], tg[0][1], whole, cam, w, h)

    def one():
        comp.render_composite(tg[1][0], tg[1][1], objects, w, h)

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
    ta, tb = [], []
    for _ in range(blocks):
        ta.append(block(seq))
        tb.append(block(one))
    stages, totals = {}, {}
    for tag, r, fn in (("merged", merged, seq), ("composite", comp, one)):
        r.set_profiling(stage_events=True)
        for _ in range(16):
            fn()
        torch.cuda.synchronize()
        stages[tag] = r.stage_times_ms()
        totals[tag] = r.debug_read_total_assignments()
        r.set_profiling(stage_events=False)
    row = {"workload": name, "objects": k, "posed": posed, "gaussians": n, "items": items,
           "merged_ms": statistics.median(ta), "composite_ms": statistics.median(tb),
           "merged_blocks_ms": ta, "composite_blocks_ms": tb, "same_image": same,
           "assignments_merged": totals["merged"], "assignments_composite": totals["composite"],
           "blend_kernel": comp.blend_kernel_kind(), "stage_ms_merged": stages["merged"],
           "stage_ms_composite": stages["composite"]}
    row["ratio"] = row["composite_ms"] / row["merged_ms"]
    row["ratio_blocks"] = [b / a for a, b in zip(ta, tb)]
    merged.close()
    comp.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose_timing.json"))
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
        print(json.dumps({k: row[k] for k in ("workload", "objects", "merged_ms", "composite_ms", "ratio",
                                              "same_image")}), flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "frames_per_block": args.frames, "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
