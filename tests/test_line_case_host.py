"""Host check of csrc/vrt_line_case.h, the owner of the line case a Λ-iteration session uploads: a stand-alone program,
tests/probes/line_case_main.cpp, drives it against a fake of the HIP calls behind upload() and DevBuf -- the argument checks
of a vrt_line_case (each array NULL in turn, nlam, the bounds and lengths of the three blocks, λ_0 and c_0, their order and
their four texts), the one writer and the one reader of the lambda | planck2 | sigma_bf1 | sigma_bf2 vector with unequal
continuum blocks, which buffers exist after create and how long they are, an allocation that fails at every position in turn,
and what the two launches the owner forwards to are handed.  No GPU, no Python-loaded library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_line_case_checks_layout_and_failed_allocations(tmp_path):
    """built with ASan + UBSan (runtimes linked in: nothing is preloaded) and run as a child process"""
    exe = tmp_path / "line_case_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voronoirt_amd", "csrc"), "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "probes", "line_case_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    assert out[:3] == ["ok checks", "ok small", "ok owner, 14 allocations"]
    assert "no allocation outlived a failed create" in out[-1]
