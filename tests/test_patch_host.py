"""Host check of the host side of the fused patch path: a stand-alone program, tests/probes/patch_host_main.cpp, compiled
together with csrc/vrt_patch.cpp, drives patch_shape (the one decision of a patch launch's kernel shape) over the tuning
fields, build_chain_items and build_patch_work (the chained launch's items and the per-layer work lists) on a hand-made
patch index of three angles and four layers with 0, 1, 9 and 17 patches per (angle, layer), and ChainLaunch::select (the
plan's four item sets, least recently used out first) against a fake of the HIP calls behind DevBuf, with an allocation
that fails at every position in turn.  No GPU, no Python-loaded library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_patch_shape_item_builders_and_item_set_cache(tmp_path):
    """built with ASan + UBSan (runtimes linked in: nothing is preloaded) and run as a child process"""
    exe = tmp_path / "patch_host_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer", "-pthread",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "voronoirt_amd", "csrc"), "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "probes", "patch_host_main.cpp"),
                           os.path.join(ROOT, "voronoirt_amd", "csrc", "vrt_patch.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    assert out[:4] == ["ok chain items", "ok work lists", "ok shapes", "ok cache"]
    assert "no allocation outlived its owner" in out[-1]
