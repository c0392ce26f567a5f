#!/usr/bin/env python3
"""Times the LocalRenderer frame (gsm_local_render) for one seeded scene, next to the Global frame and the
DepthFirst mono frame of the same scene and size from the same build.

The small benchmark scene (50k gaussians, SH0, 640x360, fp32, seed 42) by default: LocalRenderer is the
small-scene path (2048 slots per 16x16 tile).  Three GPU steps -- local, global, mono -- each a fresh
child process under its own time limit, chained: a step that fails or runs out of time ends the run and
the later steps are not started.  A step renders --warmup frames, then --blocks blocks of frames between
HIP events; the local step also reports the per-stage times of gsm_local_stage_times and the frame's
counters.  Prints one JSON object; --out writes it to a file as well (profiles/).

    python tools/local_timing.py --out profiles/local_timing.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gsm-renderer_amd"))
STEPS = ("local", "global", "mono")


def step(a):
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
    cfg = gsm_amd.RendererConfig(max_gaussians=n, max_width=W, max_height=H, precision=prec)
    cls = {"local": gsm_amd.LocalRenderer, "global": gsm_amd.GlobalRenderer, "mono": gsm_amd.DepthFirstRenderer}
    r = cls[a.step](device=0, config=cfg)
    color = torch.zeros((H, W, 4), dtype=torch.float16, device=dev)
    depth = torch.zeros((H, W), dtype=torch.float16, device=dev)

    def timed(frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            r.render(color, depth, inp, cam, W, H)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames  # ms per frame

    timed(a.warmup)
    per = max(1, a.frames // a.blocks)
    ms = [timed(per) for _ in range(a.blocks)]
    out = {"ms_per_frame": {"median": statistics.median(ms), "blocks": ms}, "frames_per_block": per,
           "device": torch.cuda.get_device_name(0)}
    if a.step == "local":
        out["counters"] = r.counters()
        r.set_profiling(True)
        for _ in range(max(per, 50)):
            r.render(color, depth, inp, cam, W, H)
        torch.cuda.synchronize()
        out["stage_ms"] = r.stage_times_ms()
    r.close()
    print("STEP_RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg1_50k_sh0_640x360_f32")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds for each GPU step")
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one step in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return 0

    from gsm_amd import scenes
    c = scenes.CONFIGS[a.config]
    out = {"config": a.config, "gaussians": c["count"], "width": c["width"], "height": c["height"],
           "sh_components": c["sh"], "warmup": a.warmup, "blocks": a.blocks}
    for s in STEPS:  # chained: the first failure ends the run
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", s,
               "--config", a.config, "--frames", str(a.frames), "--warmup", str(a.warmup), "--blocks", str(a.blocks)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
        if p.returncode != 0 or not res:
            print(f"step {s} failed (exit {p.returncode}); later steps not started", file=sys.stderr)
            return p.returncode or 1
        out[s] = json.loads(res[-1][len("STEP_RESULT "):])
    out["local_over_global"] = out["local"]["ms_per_frame"]["median"] / out["global"]["ms_per_frame"]["median"]
    out["local_over_mono"] = out["local"]["ms_per_frame"]["median"] / out["mono"]["ms_per_frame"]["median"]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
