"""Builds libvrt_hip.so (the C-ABI product library) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so is
git-ignored but travels with the tree to the GPU box.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libvrt_hip.so")
SOURCES = ["vrt_api.cpp", "vrt_grid.cpp", "vrt_schedule.cpp", "vrt_patch.cpp", "vrt_lambda.cpp", "vrt_multi.cpp", "vrt_tessellate.cpp", "vrt_tessellate.hip", "vrt_kernels.hip", "vrt_tables.hip", "vrt_layers.hip", "vrt_patch.hip", "vrt_regular.hip", "vrt_regular_lambda.hip", "vrt_physics.hip", "vrt_raster.hip", "vrt_synth.hip", "vrt_accel.hip", "vrt_continuum.hip", "vrt_line_ali.hip"]
HEADERS = [os.path.join(CSRC, h) for h in ("vrt_internal.h", "vrt_source_store.h", "vrt_raster_store.h", "vrt_line_case.h", "vrt_line_block.h", "vrt_multi_members.h", "vrt_device.h", "vrt_weights.h", "vrt_regular.h", "vrt_voigt.h", "vrt_layout_kernels.h", "vrt_tile_kernels.h", "vrt_step_kernels.h")] + [os.path.join(ROOT, "include", h) for h in ("voronoirt.h", "voronoirt_multi_accel.h")]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def is_stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force: bool = False, verbose: bool = False, diag: bool = False) -> str:
    """Compile every HIP/C++ source of the product into voronoirt_amd/libvrt_hip.so.

    diag=True builds voronoirt_amd/libvrt_hip_diag.so with -DVRT_DIAG instead: the timing diagnostics
    that switch pieces of the memory traffic off (VRT_DEBUG_FLAGS, VRT_DEBUG_SKIP_LEVELS,
    VRT_TILE_DEBUG; wrong results) exist only there.  tools/flags_sweep.sh selects it with
    VRT_LIB_PATH; nothing else loads it."""
    if diag:
        return _build(os.path.join(HERE, "libvrt_hip_diag.so"), ["-DVRT_DIAG"], verbose)
    if force or is_stale():
        _build(LIB, [], verbose)
    build_multi_accel(force, verbose)
    return LIB


ACCEL_SRC = os.path.join(CSRC, "vrt_multi_accel.cpp")
ACCEL_LIB = os.path.join(HERE, "libvrt_hip_multi_accel.so")


def build_multi_accel(force: bool = False, verbose: bool = False) -> str:
    """The companion library of include/voronoirt_multi_accel.h: csrc/vrt_multi_accel.cpp, two C entries that forward into
    libvrt_hip.so, which it links (found beside it at run time).  Rebuilt when its source, a header or libvrt_hip.so is
    newer."""
    deps = [ACCEL_SRC, LIB] + HEADERS
    if not force and os.path.exists(ACCEL_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(ACCEL_LIB) for d in deps):
        return ACCEL_LIB
    return _build(ACCEL_LIB, ["-L", HERE, "-Wl,-rpath,$ORIGIN"], verbose, sources=[ACCEL_SRC], libs=["-lvrt_hip"])


def _build(out: str, extra, verbose: bool, sources=None, libs=()) -> str:
    cmd = [
        _hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
        # build-wide floating-point contract: no FMA contraction on host or device, so neighbour
        # choices match the CPU oracle bit for bit
        "-ffp-contract=off", "-fno-fast-math",
        "-Wall", "-Wno-unused-result",
        "-I", os.path.join(ROOT, "include"), "-I", CSRC,
        "-o", out,
    ] + list(extra) + (sources or [os.path.join(CSRC, s) for s in SOURCES]) + list(libs) + ["-lpthread", "-ldl"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


PROBE_SRC = os.path.join(ROOT, "tests", "probes", "weights_probe.hip")
PROBE_LIB = os.path.join(HERE, "libvrt_weights_probe.so")


def build_probe(force: bool = False, verbose: bool = False) -> str:
    """Test infrastructure only: compile tests/probes/weights_probe.hip -- direct calls of every function of
    csrc/vrt_weights.h, for tests/test_weights_domain.py -- into voronoirt_amd/libvrt_weights_probe.so with exactly
    the flags of the product library.  Rebuilt when the probe source or vrt_weights.h is newer; the product
    library does not link it and no other module of the package names it."""
    deps = [PROBE_SRC, os.path.join(CSRC, "vrt_weights.h")]
    if not force and os.path.exists(PROBE_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(PROBE_LIB) for d in deps):
        return PROBE_LIB
    return _build(PROBE_LIB, [], verbose, sources=[PROBE_SRC])


TESS_SRC = os.path.join(CSRC, "vrt_tessellate.hip")
TESS_VARIANT_LIB = os.path.join(HERE, "libvrt_tess_faces16.so")


def build_tess_variant(force: bool = False) -> str:
    """Test infrastructure only: csrc/vrt_tessellate.hip with the face capacity lowered to 16 (-DVRT_TESS_FACES=16), so that
    tests/test_tessellate_device.py sees sites fall back to the host code.  Built by tools/build_variant.sh into
    voronoirt_amd/libvrt_tess_faces16.so, which links the libvrt_hip.so beside it for everything else; the package
    never loads it."""
    deps = [TESS_SRC, LIB] + HEADERS
    if not force and os.path.exists(TESS_VARIANT_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(TESS_VARIANT_LIB) for d in deps):
        return TESS_VARIANT_LIB
    env = dict(os.environ, VRT_VARIANT_UNITS="vrt_tessellate.hip", HIPCC=_hipcc())
    subprocess.check_call(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), os.path.basename(TESS_VARIANT_LIB),
                           "-DVRT_TESS_FACES=16"], env=env)
    return TESS_VARIANT_LIB


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True, diag="--diag" in sys.argv))
