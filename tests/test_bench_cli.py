"""bench.py's command line: a plain run keeps only the headline leg, --full keeps every leg's own
switch, and --dump-outputs writes float32 arrays within its budget, the same elements every run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_every_extra_leg_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--parity", "1", "--orbit-steps", "9")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert (a.cpu_baseline, a.cpu_one_thread, a.parity, a.orbit_steps, a.inflight_steps, a.virtual_ranks) == (0,) * 6
    assert a.multi_extra_config == "none"


def test_full_keeps_the_legs_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and a.cpu_baseline == 1 and a.parity == 1 and a.orbit_steps == 50 and a.inflight_steps == 50
    assert a.virtual_ranks == 8 and a.multi_extra_config == "cfg3_5m_sh3_4k_f16"
    a = _parse(monkeypatch, "--full", "--parity", "0", "--orbit-steps", "3", "--dump-outputs", "d")
    assert (a.parity, a.orbit_steps, a.cpu_baseline, a.dump_outputs) == (0, 3, 1, "d")


def test_dump_outputs_whole_arrays(tmp_path):
    color = np.arange(5 * 7 * 4, dtype=np.float16).reshape(5, 7, 4)
    depth = np.array([[0.5, np.inf], [np.nan, -2.0]], dtype=np.float16)
    bench.dump_outputs(str(tmp_path / "d"), {"color": color, "depth": depth})
    c, d = np.load(tmp_path / "d" / "color.npy"), np.load(tmp_path / "d" / "depth.npy")
    assert c.dtype == np.float32 and d.dtype == np.float32
    assert np.array_equal(c, color.astype(np.float32)) and np.array_equal(d, depth.astype(np.float32), equal_nan=True)


def test_dump_outputs_samples_a_large_frame_the_same_way_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    rng = np.random.default_rng(0)
    color = rng.random((33, 21, 4)).astype(np.float16)  # 11088 B as float32
    depth = rng.random((33, 21)).astype(np.float16)  # 2772 B
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"color": color, "depth": depth})
    size = 0
    for name, src in (("color", color), ("depth", depth)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < src.size and np.array_equal(a, b)
        idx = np.sort(np.random.default_rng(1234).choice(src.size, size=a.size, replace=False))
        assert np.array_equal(a, src.reshape(-1)[idx].astype(np.float32))  # elements of the frame, in row-major order
        size += a.nbytes
    assert size <= 4000
