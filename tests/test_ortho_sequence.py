"""tests/c/ortho_sequence.c: the C call sequence for one orthographic frame and one orthographic select, against the
checker (tests/ortho/ortho_ref.c) and the select's numpy contract."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def test_c_program_uses_only_declared_entry_points():
    src = open(os.path.join(HERE, "c", "ortho_sequence.c")).read()
    hdr = open(os.path.join(HERE, "..", "include", "gsm_renderer.h")).read()
    names = set(re.findall(r"\b(gsm_\w+)\(", src))
    assert {"gsm_global_render_frame", "gsm_global_select_mask_ortho"} <= names and "GSM_FRAME_ORTHOGRAPHIC" in src
    for name in names:
        assert re.search(rf"\b{name}\(", hdr), name


@pytest.mark.gpu
def test_c_program_renders_and_selects_an_orthographic_view(tmp_path):
    import ortho_ref
    import style_ref
    sys.path.insert(0, os.path.join(HERE, "..", "gsm-renderer_amd"))
    from gsm_amd import scenes
    exe = os.path.join(HERE, "c", "ortho_sequence")
    assert os.path.exists(exe), "tests/c/ortho_sequence not built (__graft_entry__.build)"
    n, W, H, sh = 3001, 203, 77, 16
    world, harm, _ = scenes.gen_scene(n, W, H, sh, 0, seed=3)
    cam = scenes.ortho_camera(W, H, 3.0)
    with ortho_ref.frame([(world, np.asarray(harm).reshape(-1), cam)], sh, W, H) as fr:
        ref, res = fr.data(), fr.walk()
    (tmp_path / "w.bin").write_bytes(world.tobytes())
    (tmp_path / "h.bin").write_bytes(np.asarray(harm).tobytes())
    cf = np.concatenate([cam["view"], cam["proj"], cam["position"],
                         np.array([cam["focal_x"], cam["focal_y"], cam["near"], cam["far"]], np.float32)])
    (tmp_path / "c.bin").write_bytes(cf.astype(np.float32).tobytes())
    out = tmp_path / "out.bin"
    p = subprocess.run([exe, str(tmp_path / "w.bin"), str(tmp_path / "h.bin"), str(n), str(sh), str(W), str(H),
                        str(tmp_path / "c.bin"), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr + p.stdout
    raw = out.read_bytes()
    px = W * H
    color = np.frombuffer(raw[:px * 8], np.uint16).reshape(H, W, 4)
    pick = np.frombuffer(raw[px * 8:px * 12], np.uint32).reshape(H, W)
    state = np.frombuffer(raw[px * 12:px * 12 + n], np.uint8)
    matched = int(np.frombuffer(raw[px * 12 + n:], np.uint32)[0])
    assert np.array_equal(color, res["color"]) and np.array_equal(pick, res["items"])
    want, m = style_ref.select_mask(ref["render_data"], ref["mask"], W, H, np.ones((H, W), np.uint8),
                                    np.zeros(n, np.uint8), 0xFF, 4)
    assert np.array_equal(state, want) and matched == m > 0
