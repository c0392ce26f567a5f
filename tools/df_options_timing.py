#!/usr/bin/env python3
"""Times the DepthFirst frames under the create options (gsm_depthfirst_create_with_options): depth key
bits x tile id bits = (32,16) the default, (16,16) and (32,32).

Two seeded scenes (seed 42): the config-5 stereo scene (1M gaussians, SH2, 2 x 1440x1600, fp16) through
gsm_depthfirst_render_stereo_sbs and the 1M mono scene at 1080p (config 2: SH3, fp16) through
gsm_depthfirst_render.  Every (scene, mode) is one GPU step: a fresh child process under its own time
limit, chained -- a step that fails or runs out of time ends the run and the later steps are not started.
A step renders --warmup frames, then --blocks blocks of frames between HIP events, then a profiled run for
gsm_depthfirst_stage_times.  --repeats runs the whole series that many times, one after another, so the
spread between repeated runs of one mode is on record next to the differences between modes.
--baseline-tree DIR (another built checkout of this project, e.g. the parent commit) adds a default-mode
step of that tree in front of every repeat -- alternating builds on one machine in one session.
Prints one JSON object; --out writes it to a file as well (profiles/).

    python tools/df_options_timing.py --out profiles/df_options_timing.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"stereo_cfg5": "cfg5_1m_sh2_stereo_2x1440x1600_f16", "mono_1080p": "cfg2_1m_sh3_1080p_f16"}
MODES = ((32, 16), (16, 16), (32, 32))


def step(a):
    tree = a.tree or ROOT
    sys.path.insert(0, os.path.join(tree, "gsm-renderer_amd"))
    import numpy as np
    import torch
    import gsm_amd
    from gsm_amd import scenes

    c = scenes.CONFIGS[SCENES[a.scene]]
    n, W, H, sh, prec = c["count"], c["width"], c["height"], c["sh"], c["precision"]
    world_np, harm_np, cam_d = scenes.gen_scene(n, W, H, sh, prec, seed=42)
    dev = torch.device("cuda", 0)
    world = torch.from_numpy(world_np.view(np.uint8).reshape(-1).copy()).to(dev)
    harm = torch.from_numpy(harm_np.view(np.uint8).reshape(-1).copy()).to(dev)
    inp = gsm_amd.GaussianInput(world, harm, n, sh)
    # the reference's default capacity (RendererConfig.maxGaussians = 6M): no instance is clamped
    cfg = gsm_amd.RendererConfig(max_gaussians=max(n, 6_000_000), max_width=W, max_height=H, precision=prec)
    dk, ti = a.depth_key_bits, a.tile_id_bits
    if a.tree:  # a tree that may predate the options: its default create
        assert (dk, ti) == (32, 16)
        r = gsm_amd.DepthFirstRenderer(device=0, config=cfg)
    else:
        r = gsm_amd.DepthFirstRenderer(device=0, config=cfg, depth_key_bits=dk, tile_id_bits=ti)
    stereo = "stereo" in c
    if stereo:
        L = gsm_amd.CameraParams.from_dict(scenes.make_camera(W, H, -c["stereo"]))
        R = gsm_amd.CameraParams.from_dict(scenes.make_camera(W, H, c["stereo"]))
        color = torch.zeros((H, 2 * W, 4), dtype=torch.float16, device=dev)

        def frame():
            r.render_stereo_sbs(color, inp, L, R, W, H)
    else:
        cam = gsm_amd.CameraParams.from_dict(cam_d)
        color = torch.zeros((H, W, 4), dtype=torch.float16, device=dev)
        depth = torch.zeros((H, W), dtype=torch.float16, device=dev)

        def frame():
            r.render(color, depth, inp, cam, W, H)

    def timed(frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            frame()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames  # ms per frame

    timed(a.warmup)
    per = max(1, a.frames // a.blocks)
    ms = [timed(per) for _ in range(a.blocks)]
    out = {"ms_per_frame": {"median": statistics.median(ms), "blocks": ms}, "frames_per_block": per,
           "device": torch.cuda.get_device_name(0), "counters": r.counters()}
    r.set_profiling(True)
    for _ in range(max(per, 50)):
        frame()
    torch.cuda.synchronize()
    out["stage_ms"] = r.stage_times_ms()
    r.close()
    print("STEP_RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-tree", default=None, help="another built checkout: its default mode, every repeat")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds for each GPU step")
    ap.add_argument("--out", default=None)
    # (internal) one step in this process
    ap.add_argument("--scene", choices=sorted(SCENES), default=None)
    ap.add_argument("--depth-key-bits", type=int, default=32)
    ap.add_argument("--tile-id-bits", type=int, default=16)
    ap.add_argument("--tree", default=None)
    a = ap.parse_args()
    if a.scene:
        step(a)
        return 0

    out = {"scenes": SCENES, "frames": a.frames, "warmup": a.warmup, "blocks": a.blocks, "repeats": a.repeats,
           "baseline_tree": bool(a.baseline_tree), "runs": []}
    for scene in SCENES:
        for rep in range(a.repeats):  # chained: the first failure ends the run
            series = ([("baseline", 32, 16)] if a.baseline_tree else []) + [("this", d, t) for d, t in MODES]
            for build, d, t in series:
                cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
                       "--scene", scene, "--depth-key-bits", str(d), "--tile-id-bits", str(t),
                       "--frames", str(a.frames), "--warmup", str(a.warmup), "--blocks", str(a.blocks)]
                if build == "baseline":
                    cmd += ["--tree", os.path.abspath(a.baseline_tree)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                res = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP_RESULT ")]
                if p.returncode != 0 or not res:
                    print(f"step {scene} {build} ({d},{t}) failed (exit {p.returncode}); later steps not started",
                          file=sys.stderr)
                    return p.returncode or 1
                r = json.loads(res[-1][len("STEP_RESULT "):])
                r.update({"scene": scene, "build": build, "mode": [d, t], "repeat": rep})
                out["runs"].append(r)
    # per (scene, build, mode): the repeats' medians and stage times side by side
    summary = {}
    for r in out["runs"]:
        k = f"{r['scene']} {r['build']} ({r['mode'][0]},{r['mode'][1]})"
        s = summary.setdefault(k, {"frame_ms": [], "depth_sort_ms": [], "tile_sort_ms": []})
        s["frame_ms"].append(round(r["ms_per_frame"]["median"], 4))
        s["depth_sort_ms"].append(round(r["stage_ms"]["depth_sort"], 4))
        s["tile_sort_ms"].append(round(r["stage_ms"]["tile_sort"], 4))
    out["summary"] = summary
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
