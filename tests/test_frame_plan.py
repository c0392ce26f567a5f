"""The Global frame entries' admission rows and layouts (gsm-renderer_amd/csrc/gsm_frame_plan.h) on the CPU.

tests/host/frame_plan_test.cpp is a stand-alone program over that header (and the two plain headers it includes): it
is compiled here with the host compiler (no HIP), rebuilt whenever it or a header is newer, and run.
__graft_entry__.build() builds it too.
"""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "gsm-renderer_amd", "csrc")
_SRC = os.path.join(_HERE, "host", "frame_plan_test.cpp")
_EXE = os.path.join(_HERE, "host", "frame_plan_test")
_DEPS = [_SRC] + [os.path.join(_CSRC, h) for h in ("gsm_frame_plan.h", "gsm_blend_plan.h", "gsm_types.h",
                                                   "gsm_schedule_key.h")] + \
    [os.path.join(_ROOT, "include", h) for h in ("gsm_renderer.h", "gsm_debug.h")]
_CXXFLAGS = ["-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


def build(force: bool = False) -> str:
    if force or not os.path.exists(_EXE) or os.path.getmtime(_EXE) < max(map(os.path.getmtime, _DEPS)):
        tmp = _EXE + f".{os.getpid()}.tmp"
        subprocess.run([os.environ.get("CXX", "g++")] + _CXXFLAGS + ["-I" + _CSRC, "-o", tmp, _SRC], check=True)
        os.replace(tmp, _EXE)
    return _EXE


def test_header_compiles_alone(tmp_path):
    """g++ compiles the header by itself: plain C++17, no HIP include."""
    tu = tmp_path / "only_header.cpp"
    tu.write_text('#include "gsm_frame_plan.h"\nint main() { return 0; }\n')
    subprocess.run([os.environ.get("CXX", "g++")] + _CXXFLAGS + ["-I" + _CSRC, "-fsyntax-only", str(tu)], check=True)


def test_frame_plan_program():
    """Every status row of the single frame, views, batch, frames, composite, select_mask, select_pick and partition
    checks alone, adjacent rows failing together, the offending view or object last, items and tiles at and one past
    the handle's, the 65535 bound, the 32-bit overflow of a views call, pitches and pointers off by one and two, the
    style-table agreement of a batch, more frames than a handle holds, and the batch, composite and views layouts:
    every result equals the hand-written row."""
    r = subprocess.run([build()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout
