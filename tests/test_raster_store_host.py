"""Host check of csrc/vrt_raster_store.h, the owner of a raster Λ-iteration session's S and J (rows and plane-major, the
I_0 planes, the zero plane), and of the two shared pieces of csrc/vrt_internal.h that follow every single-device update
(read_criterion, ng_after_update): a stand-alone program, tests/probes/raster_store_main.cpp, drives them against a fake of
the HIP calls and layout launches behind them -- which buffers exist after create and how large (odd and even n nlam), the
planes as the transpose of the rows, S_written and download, an allocation that fails at every position in turn during create
and during stage, adopt as pointer swaps with every old buffer released exactly once, what Ng acceleration is handed, and the
epilogue's refresh and synchronise on recorded, incomplete, accepted and rejected steps.  No GPU, no Python-loaded library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_raster_store_failed_allocations_and_shared_epilogue(tmp_path):
    """built with ASan + UBSan (runtimes linked in: nothing is preloaded) and run as a child process"""
    exe = tmp_path / "raster_store_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voronoirt_amd", "csrc"), "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "probes", "raster_store_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    assert "ok raster 5 x 3 x 3, nlam 3" in out and "ok raster 4 x 2 x 3, nlam 4" in out
    assert "ok epilogue" in out and "ok criterion" in out
    assert "no allocation outlived a failed create or stage" in out[-1]
