"""The Global blend's launch plan (gsm-renderer_amd/csrc/gsm_blend_plan.h) on the CPU.

tests/host/blend_plan_test.cpp is a stand-alone program over that header alone: it is compiled here with the host
compiler (no HIP), rebuilt whenever it or a header is newer, and run.  __graft_entry__.build() builds it too.
"""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "gsm-renderer_amd", "csrc")
_SRC = os.path.join(_HERE, "host", "blend_plan_test.cpp")
_EXE = os.path.join(_HERE, "host", "blend_plan_test")
_DEPS = [_SRC, os.path.join(_CSRC, "gsm_blend_plan.h"), os.path.join(_CSRC, "gsm_schedule_key.h")]
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
    tu.write_text('#include "gsm_blend_plan.h"\nint main() { return 0; }\n')
    subprocess.run([os.environ.get("CXX", "g++")] + _CXXFLAGS + ["-I" + _CSRC, "-fsyntax-only", str(tu)], check=True)


def test_blend_plan_program():
    """Every kernel family, each side of the quadrant / half-tile rule, of both wave thresholds and of the grid's
    clamps at 4 and at 256 CUs, a waves override, the pair walk taken and refused for each of its conditions, the
    walks over the sorted values without them, and every flag bit set and clear: the plan equals the hand-written
    row."""
    r = subprocess.run([build()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout
