"""Host check of csrc/vrt_source_store.h, the owner of a Λ-iteration session's S and J in its three storage forms (rows,
sweep-order planes, float sweep-order planes): a stand-alone program, tests/probes/source_store_main.cpp, drives the store
against a fake of the HIP calls and layout launches behind it -- which buffers exist after create and how large (odd and even
nlam), an allocation that fails at every position in turn during create and during stage, adopt as pointer swaps with every
old buffer released exactly once, and what Ng acceleration is handed.  No GPU, no Python-loaded library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_source_store_forms_and_failed_allocations(tmp_path):
    """built with ASan + UBSan (runtimes linked in: nothing is preloaded) and run as a child process"""
    exe = tmp_path / "source_store_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voronoirt_amd", "csrc"), "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "probes", "source_store_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    for form in ("rows", "planes", "planes f32"):
        for nlam in (3, 4):
            assert "ok %s, nlam %d" % (form, nlam) in out
    assert "no allocation outlived a failed create or stage" in out[-1]
