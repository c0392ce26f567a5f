#!/usr/bin/env python3
"""Time GlobalRenderer.render_styled against `render` of the same scene, and select_mask alone.

Per workload one process, HIP events, interleaved blocks: (a) one `render` per frame; (b) one `render_styled` per
frame with the identity table (the same image: the cost of the state byte, the table entry and the integer rule);
(c) one `render_styled` per frame with 10 % of the gaussians hidden and 10 % tinted (a smaller frame: hidden
gaussians leave the lists).  Three handles of one configuration; 5 blocks of 40 frames each by default, medians of
the per-frame block times.  Stage times come from a profiled run of each afterwards.  At 1M the select is timed as
well: one select_mask per frame with a rectangle mask (toggle, so every frame does the same work).  The driver
itself never opens the GPU: every workload runs in a fresh child process under its own time limit, and the first one
that fails or runs out of time ends the run.  Writes profiles/style_timing.json.

    python tools/style_timing.py [--blocks 5] [--frames 40] [--out profiles/style_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))

# workloads: name -> (time limit in seconds, gaussians, sh components, precision, width, height, time the select)
WORKLOADS = {
    "1m_sh3_1080p_f16": (300, 1_000_000, 16, 1, 1920, 1080, True),
    "50k_sh0_640x360_f32": (120, 50_000, 1, 0, 640, 360, False),
}


def run_workload(name, blocks, frames):
    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    _, n, sh, prec, w, h, with_select = WORKLOADS[name]
    world_np, harm_np, cam_d = scenes.gen_scene(n, w, h, sh, prec, seed=42)
    world = torch.from_numpy(world_np.view(np.uint8).reshape(-1).copy()).cuda()
    harm = torch.from_numpy(harm_np.view(np.uint8).reshape(-1).copy()).cuda()
    cfg = gsm_amd.RendererConfig(max_gaussians=n, max_width=w, max_height=h, precision=prec, gaussian_color_space=0)
    rs = [gsm_amd.GlobalRenderer(config=cfg) for _ in range(3)]
    inp = gsm_amd.GaussianInput(world, harm, n, sh)
    cam = gsm_amd.CameraParams.from_dict(cam_d)
    tg = [(torch.zeros((h, w, 4), dtype=torch.float16, device="cuda"),
           torch.zeros((h, w), dtype=torch.float16, device="cuda")) for _ in range(3)]
    rng = np.random.default_rng(1)
    u = rng.random(n)
    mixed = np.where(u < 0.1, 1, np.where(u < 0.2, 2, 0)).astype(np.uint8)   # 10 % hidden, 10 % tinted
    st_id = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st_mix = torch.from_numpy(mixed).cuda()
    identity = [gsm_amd.Style()]
    table = [gsm_amd.Style(), gsm_amd.Style(hidden=True), gsm_amd.Style((255, 200, 0), 160, 255)]

    def plain():
        rs[0].render(tg[0][0], tg[0][1], inp, cam, w, h)

    def ident():
        rs[1].render_styled(tg[1][0], tg[1][1], None, inp, cam, w, h, st_id, identity)

    def mix():
        rs[2].render_styled(tg[2][0], tg[2][1], None, inp, cam, w, h, st_mix, table)

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames

    fns = (("render", plain), ("styled_identity", ident), ("styled_mixed", mix))
    for _ in range(10):  # warm-up: schedules, caches
        for _, fn in fns:
            fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(tg[0][0], tg[1][0]) and torch.equal(tg[0][1], tg[1][1]))
    times = {tag: [] for tag, _ in fns}
    for _ in range(blocks):
        for tag, fn in fns:
            times[tag].append(block(fn))
    row = {"workload": name, "gaussians": n, "width": w, "height": h, "identity_same_image": same}
    for (tag, fn), r in zip(fns, rs):
        r.set_profiling(stage_events=True)
        for _ in range(16):
            fn()
        torch.cuda.synchronize()
        row[tag + "_ms"] = statistics.median(times[tag])
        row[tag + "_blocks_ms"] = times[tag]
        row["stage_ms_" + tag] = r.stage_times_ms()
        row["assignments_" + tag] = r.debug_read_total_assignments()
        r.set_profiling(stage_events=False)
    row["ratio_identity"] = row["styled_identity_ms"] / row["render_ms"]
    row["ratio_mixed"] = row["styled_mixed_ms"] / row["render_ms"]
    if with_select:
        mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        mask[h // 4:3 * h // 4, w // 4:3 * w // 4] = 1
        matched = torch.zeros(1, dtype=torch.int32, device="cuda")
        state = torch.zeros(n, dtype=torch.uint8, device="cuda")

        def select():
            rs[0].select_mask(inp, cam, w, h, mask, state, 0xFF, 1, matched=matched)

        for _ in range(10):
            select()
        torch.cuda.synchronize()
        ts = [block(select) for _ in range(blocks)]
        row["select_mask_ms"] = statistics.median(ts)
        row["select_mask_blocks_ms"] = ts
        row["select_matched"] = int(matched.item())
    for r in rs:
        r.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "style_timing.json"))
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
        print(json.dumps({k: row[k] for k in ("workload", "render_ms", "styled_identity_ms", "styled_mixed_ms",
                                              "ratio_identity", "ratio_mixed", "identity_same_image")}), flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"blocks": args.blocks, "frames_per_block": args.frames, "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
