"""CPU tests of the float-storage line Λ-iteration: the model loop (tests/f32_lambda_model.py) exists and is well posed,
and the figures that tests/test_f32_lambda.py (GPU) takes its bounds from are those of the oracle alone -- the model loop
against the fp64 oracle loop, and against a copy of itself whose exponentials and opacities carry the coarsest device
errors the project quotes."""
import numpy as np

from f32_lambda_model import ALPHA_EPS, deviations, f32, oracle_runs, update_model
from oracle.f32_model import EXP_EPS, float_compare, within_conditions

ITERATES = 6


def test_model_loop_is_well_posed_and_stays_beside_the_fp64_loop(voro_small):
    """Six iterates on the 1500-site, 33-wavelength case: finite fields, positive populations that sum to the atom
    density, every J and S a float; the deviations from the fp64 oracle loop are those of float storage (a few 1e-7)
    and do not grow with the iterate.  Printed per iterate: J (of max |J|), S and the populations (relative)."""
    r = oracle_runs(*voro_small, ITERATES)
    case, worst = r["case"], []
    for k, (m, d) in enumerate(zip(r["model"], r["f64"])):
        J, S, pops = m
        assert np.isfinite(J).all() and np.isfinite(S).all() and (pops > 0).all()
        assert np.allclose(pops.sum(axis=0), case.atom_density, rtol=1e-12)
        assert np.array_equal(f32(J), J) and np.array_equal(f32(S), S)
        worst.append(deviations(m, d))
        print(f"iterate {k + 1}: model loop against the fp64 loop: J {worst[-1][0]:.2e} of max|J|, S {worst[-1][1]:.2e}, "
              f"populations {worst[-1][2]:.2e}")
    # float storage: half an ulp (6e-8) per rounding, a handful of roundings in a row; and no drift
    assert max(w[0] for w in worst) < 1e-6 and max(w[1] for w in worst) < 1e-6 and max(w[2] for w in worst) < 1e-6
    for q in range(3):
        assert worst[-1][q] < 2 * worst[0][q]
    assert r["hist"][2] < r["hist"][1] < r["hist"][0]


def test_reference_alone_meets_the_conditions_of_the_gpu_file(voro_small):
    """The model loop against its perturbed copy (every exponential changed by EXP_EPS, every α by ALPHA_EPS): the first
    iterate is bit-identical in 99.9 % of J and of S and within 2 float ulps in the rest (GPU test 4); over four iterates
    the two stay within 2 ulps, half of the 4 the GPU file allows (GPU test 5); the populations' deviation is printed --
    the GPU file allows four times it."""
    r = oracle_runs(*voro_small, ITERATES)
    for name, q in (("J", 0), ("S", 1)):
        ok, ndiff, size, ulps = within_conditions(r["perturbed"][0][q], r["model"][0][q])
        print(f"first iterate, {name}: the perturbed copy differs in {ndiff} of {size} elements, largest distance {ulps:g} ulp")
        assert ok, (name, ndiff, size, ulps)
    for k in range(ITERATES):
        figs = [float_compare(r["perturbed"][k][q], r["model"][k][q]) for q in range(2)]
        dp = deviations(r["perturbed"][k], r["model"][k])[2]
        print(f"iterate {k + 1}: perturbed copy: J differs in {figs[0][0]} ({figs[0][1]:g} ulp), S in {figs[1][0]} ({figs[1][1]:g} ulp), "
              f"populations {dp:.2e} (exp {EXP_EPS:g}, alpha {ALPHA_EPS:g})")
        if k < 4:
            assert figs[0][1] <= 2 and figs[1][1] <= 2, (k, figs)


def test_update_model_rounds_where_the_header_says():
    """The numpy model of the update step on a handful of values worked by hand: J is the float sum, S the float of the
    double expression, the scalar is taken from the stored floats, NaN spreads, S_old = 0 gives 1."""
    one = np.float32(1.0)
    tiny = np.float32(2.0 ** -24)                              # half an ulp of 1: 1 + tiny rounds to even, to 1
    J, S, d = update_model(np.array([[one]]), np.array([[tiny]]), np.array([[one]], dtype=np.float32), np.array([[one]]), [0.0])
    assert J[0, 0] == one and S[0, 0] == one and d == 0.0
    J, S, d = update_model(np.array([[one]]), None, np.array([[np.float32(3.0)]]), np.array([[np.float32(0.0)]]), [1.0])
    assert S[0, 0] == np.float32(3.0) and d == 1.0
    J, S, d = update_model(None, np.array([[np.float32("nan")]]), np.array([[one]]), np.array([[one]]), [0.5])
    assert np.isnan(S[0, 0]) and np.isnan(d)
    e = 0.3
    J, S, d = update_model(np.array([[np.float32(0.7)]]), np.array([[np.float32(0.2)]]), np.array([[np.float32(1.1)]]),
                           np.array([[np.float32(0.9)]]), [e])
    j = np.float32(np.float64(np.float32(0.7)) + np.float64(np.float32(0.2)))
    s = np.float32((1.0 - e) * np.float64(j) + e * np.float64(np.float32(1.1)))
    assert J[0, 0] == j and S[0, 0] == s and d == abs(1.0 - np.float64(np.float32(0.9)) / np.float64(s))
