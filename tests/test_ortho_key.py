"""The schedule key's orthographic word (gsm-renderer_amd/csrc/gsm_schedule_key.h) on the CPU.

tests/host/ortho_key_test.cpp is a stand-alone program over that header alone: it is compiled here with the host
compiler (no HIP), rebuilt whenever it or the header is newer, and run; __graft_entry__.build() builds it too.  The
same program is the stand-alone target of a host-side AddressSanitizer / UndefinedBehaviorSanitizer run of the key
code: a second build with -fsanitize=address,undefined is run as a program of its own.
"""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "gsm-renderer_amd", "csrc")
_SRC = os.path.join(_HERE, "host", "ortho_key_test.cpp")
_EXE = os.path.join(_HERE, "host", "ortho_key_test")
_DEPS = [_SRC, os.path.join(_CSRC, "gsm_schedule_key.h")]
_CXXFLAGS = ["-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


def build(force: bool = False) -> str:
    if force or not os.path.exists(_EXE) or os.path.getmtime(_EXE) < max(map(os.path.getmtime, _DEPS)):
        tmp = _EXE + f".{os.getpid()}.tmp"
        subprocess.run([os.environ.get("CXX", "g++")] + _CXXFLAGS + ["-I" + _CSRC, "-o", tmp, _SRC], check=True)
        os.replace(tmp, _EXE)
    return _EXE


def test_ortho_key_program():
    """An orthographic frame and a perspective one clear each other's costs in every kind of frame; a batch is marked
    by any orthographic view; perspective keys keep their words; nothing allocates within the reservations."""
    r = subprocess.run([build()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout


def test_ortho_key_program_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run on its own: no report, exit 0."""
    exe = tmp_path / "ortho_key_test_san"
    subprocess.run([os.environ.get("CXX", "g++")] + _CXXFLAGS +
                   ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + _CSRC, "-o", str(exe),
                    _SRC], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout and "ERROR" not in r.stdout and "runtime error" not in r.stdout
