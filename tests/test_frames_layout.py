"""gsm_global_render_frames adds no public struct: it takes an array of the gsm_global_frame the
project already has.  CPU only: the descriptor is still 112 bytes -- the array's stride -- through the new signature,
in C and in the ctypes mirror."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_render_frames_takes_an_array_of_the_unchanged_descriptor(gsm, tmp_path):
    root = os.path.dirname(HERE)
    prog = tmp_path / "layout.c"
    prog.write_text(
        '#include "gsm_renderer.h"\n#include <stdio.h>\n#include <stddef.h>\n'
        "_Static_assert(__builtin_types_compatible_p(__typeof__(&gsm_global_render_frames),\n"
        "    gsm_status (*)(gsm_renderer *, void *, const gsm_global_frame *, uint32_t)), \"render_frames' signature\");\n"
        "_Static_assert(__builtin_types_compatible_p(__typeof__(&gsm_global_select_pick_ids),\n"
        "    gsm_status (*)(gsm_renderer *, void *, const void *, size_t, uint32_t, uint32_t, const void *, size_t,\n"
        "                   uint8_t *, uint32_t, uint32_t, uint32_t, uint32_t *)), \"select_pick_ids' signature\");\n"
        "int main(void) {\n"
        "    gsm_global_frame two[2];\n"
        '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(gsm_global_frame), (size_t)((char *)&two[1] - (char *)&two[0]),\n'
        "           offsetof(gsm_global_frame, color), offsetof(gsm_global_frame, pick_r32u),\n"
        "           offsetof(gsm_global_frame, occluder_r32f), offsetof(gsm_global_frame, states),\n"
        "           offsetof(gsm_global_frame, flags));\n"
        "    return 0;\n}\n")
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(prog), "-o",
                    str(tmp_path / "layout")], check=True)
    sizes = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                            check=True).stdout.split()]
    F = gsm._GlobalFrame
    assert sizes[0] == sizes[1] == 112 == gsm.GLOBAL_FRAME_BYTES == C.sizeof(F) == C.sizeof(F * 2) // 2
    assert sizes[2:] == [F.color.offset, F.pick_r32u.offset, F.occluder_r32f.offset, F.states.offset, F.flags.offset]
    args, res = gsm._SIGNATURES["gsm_global_render_frames"]
    assert args[2] is C.POINTER(F) and args[3] is C.c_uint32 and res is C.c_int
