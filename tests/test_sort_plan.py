"""The radix sorts' pass plans (gsm-renderer_amd/csrc/gsm_sort_plan.h) on the CPU.

tests/host/sort_plan_test.cpp is a stand-alone program over that header alone: it is compiled here with the host
compiler (no HIP), rebuilt whenever it or a header is newer, and run.  __graft_entry__.build() builds it too.
"""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "gsm-renderer_amd", "csrc")
_SRC = os.path.join(_HERE, "host", "sort_plan_test.cpp")
_EXE = os.path.join(_HERE, "host", "sort_plan_test")
_DEPS = [_SRC, os.path.join(_CSRC, "gsm_sort_plan.h"), os.path.join(_ROOT, "include", "gsm_debug.h")]
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
    tu.write_text('#include "gsm_sort_plan.h"\nint main() { return 0; }\n')
    subprocess.run([os.environ.get("CXX", "g++")] + _CXXFLAGS + ["-I" + _CSRC, "-fsyntax-only", str(tu)], check=True)


def test_sort_plan_program():
    """Every tile plan of tests/test_frame_sort.py's PLANS table and every tile field of 9 to 16 bits, the one wide
    pass taken and refused, the wide-then-narrow plan at each width and past the widest, the bits and pairs plans with
    each switch, the plan a frame sort reports, and the fit against a workspace of sort_workspace_bytes and one a word
    short: every pass equals the hand-written row."""
    r = subprocess.run([build()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout
