"""Host check of csrc/vrt_line_block.h, the owner of one wavelength block of a line Λ-iteration session (S and J, B_0 in the
store's order, I_0 and the native α, and the iterate up to the update), and of csrc/vrt_multi_members.h, the per-device worker
protocol of the multi-device object: a stand-alone program, tests/probes/line_block_main.cpp, drives them against a fake of
the HIP calls and launches behind them -- which buffers a block holds after create in all three forms (odd and even n·nb, one
wavelength, none), an allocation that fails at every position in turn, the launches of a step in order with and without Λ*,
the plan checks of a line session, and every way a member's work can end: failing on one member, on two, throwing, skipped,
a device that cannot be made current, with and without the plan mutex.  No GPU, no Python-loaded library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_line_block_failed_allocations_and_member_protocol(tmp_path, sanitizer):
    """built with ASan + UBSan, and again with TSan (on_members is the one threaded piece); the runtimes are linked in
    (nothing is preloaded) and the program runs as a child process"""
    exe = tmp_path / "line_block_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    static = ["-static-libasan", "-static-libubsan"] if sanitizer != "thread" else ["-static-libtsan"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={sanitizer}", *static, "-fno-omit-frame-pointer",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voronoirt_amd", "csrc"), "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "probes", "line_block_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1",
                                TSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    for form in ("rows", "planes", "planes f32"):
        for block in ("[1, 4)", "[2, 6)", "[6, 7)", "[3, 3)"):
            assert f"ok block {block} {form}" in out
    assert "ok plan checks" in out and "ok members" in out
    assert "no allocation outlived a failed create" in out[-1]
