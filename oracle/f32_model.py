"""Test infrastructure (like everything under oracle/): what tests/test_f32_model_host.py (CPU) and
tests/test_f32_storage.py (GPU) share -- which storage model (vrt_oracle.c: orc_delaunay_model) each device path of
the fp32 storage path implies, the inputs both files run, and the comparison of two float32 arrays by the share
of bit-identical elements and the largest distance in float ulps.

Where each path rounds, read off the kernels (voronoirt_amd/csrc):
  patches  k_patch_solve / lean_pairs / quad_pairs (vrt_patch.hip): inputs widened, c and g in double registers, the
           levels on a double2 LDS tile, ONE from_d2<float> / (float) cast when the owned sites are stored
           -> store "layer", coef "f64".  J: patch_reduce_role / chain_reduce round Σ_a w_a I_a per direction to
           float, k_combine_J[_narrow] (vrt_layout_kernels.h) rounds J_up + J_down -> jsum "dir".
  steps    run_steps (vrt_layers.hip) takes the single-wavelength level kernel for EVERY float run
           (`single = kF32 || ...`): k_step_coeffs<float, true> stores c, g1, g2 as float
           (vrt_step_kernels.h, the SPLIT branch), k_step_levels1<float, K> keeps them and its tile as float and
           rounds every visit -> store "visit", coef "f32".  J as for patches (k_reduce_dir, k_combine_J) -> "dir".
           (The pair level kernel k_step_levels, double2 tile, exists for fp64 storage only.)
  levels   k_sweep_level<float> (vrt_kernels.hip): one launch per dependency level, every visit re-evaluates the
           reference's expression from float I in memory and stores a float -> store "visit", coef "f64".
           J: k_reduce_J<float>, one sum over every angle rounded once -> jsum "single".
"""
import numpy as np

PATH_MODEL = {
    "patches": dict(store="layer", coef="f64", jsum="dir"),
    "steps": dict(store="visit", coef="f32", jsum="dir"),
    "levels": dict(store="visit", coef="f64", jsum="single"),
}

# The conditions of both files.  A correct kernel differs from its model only where the ~1e-15 difference between the
# device's and libm's exponential straddles a float rounding boundary; the CPU file shows that a model against a copy
# of itself with every exp changed by 2e-13 relative stays within both, and that two different models do not.
MIN_IDENTICAL_SHARE = 0.999
MAX_ULPS = 2
EXP_EPS = 2e-13                 # the coarsest device exponential ever quoted


def draw_case(so, nlam, n_angles=0, seed=12):
    """float32 S, α (n, nlam), I_0 of both directions, drawn as in test_fp32_value_path_against_fp64_oracle (the down
    boundary and the per-angle factor of α are further draws of the same generator); n_angles > 0: α per angle.
    α is per box width, so that Δτ spans the three branches of linear_weights on the metre-sized lattice too (the
    Voronoi grid of the tests is one unit wide: its numbers are those of that test)."""
    rng = np.random.default_rng(seed)
    n = so.n
    S = (1 + rng.random((n, nlam))).astype(np.float32)
    al = (5 * 10 ** rng.uniform(-3, 3, (n, 1)) * (1 + rng.random((n, nlam))) / (so.bounds[3] - so.bounds[2])).astype(np.float32)
    I0u = rng.random((so.layers_up[1] - 1, nlam)).astype(np.float32)
    I0d = rng.random((so.layers_down[1] - 1, nlam)).astype(np.float32)
    if n_angles:
        al = (al[None].astype(np.float64) * (1 + 0.1 * rng.random((n_angles, n, nlam)))).astype(np.float32)
    return S, al, I0u, I0d


def _ordered(a):
    """float32 bit patterns as integers that count representable values in order (-0 and +0 coincide)"""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def float_compare(got, want):
    """(number of elements whose float32 values differ, largest distance in float ulps) of two arrays that hold
    float32 values (as float32, or exactly representable in float64).  A NaN counts as infinitely far."""
    g64, w64 = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    g, w = g64.astype(np.float32), w64.astype(np.float32)
    assert np.array_equal(g.astype(np.float64), g64, equal_nan=True) and np.array_equal(w.astype(np.float64), w64, equal_nan=True), \
        "float_compare takes float32 values"
    d = np.abs(_ordered(g) - _ordered(w)).astype(np.float64)
    d[np.isnan(g) | np.isnan(w)] = np.inf
    return int((d > 0).sum()), float(d.max()) if d.size else 0.0


def within_conditions(got, want):
    """(ok, differing, size, largest ulp distance): at least MIN_IDENTICAL_SHARE of the elements bit-identical and
    every other one within MAX_ULPS"""
    ndiff, ulps = float_compare(got, want)
    size = int(np.asarray(want).size)
    return (size - ndiff) >= MIN_IDENTICAL_SHARE * size and ulps <= MAX_ULPS, ndiff, size, ulps
