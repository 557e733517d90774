"""CPU tests of the storage-model oracle (oracle/vrt_oracle.c: orc_delaunay_model, orc_J_voronoi_model), the reference
of tests/test_f32_storage.py: the C model against an independent second transcription (oracle/pyref.py, numpy for
J) bit for bit, the default model against the existing oracle bit for bit, the share / ulp conditions of the GPU
file met by the reference alone under a changed exponential, and the models far enough apart on the GPU file's
inputs that a kernel which rounds in the wrong place cannot pass."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle import pyref
from oracle.f32_model import EXP_EPS, PATH_MODEL, draw_case, float_compare, within_conditions
from voronoirt_amd.api import read_quadrature

STORES = ("f64", "layer", "visit")
COEFS = ("f64", "f32")


def _one_based(a):
    return [0] + [float(v) for v in a]


@pytest.fixture(scope="module")
def small_grids(bcc_small, golden):
    """bcc_small and the committed voro2k grid as (oracle sites, the 1-based lists oracle/pyref.py takes)."""
    out = {}
    pos, nbr, bounds = bcc_small
    out["bcc_small"] = (orc.make_sites(pos, nbr, bounds), bounds)
    out["voro2k"] = (orc.read_cell(golden["nbr_file"], golden["meta"]["n"], golden["pos"], golden["bounds"]),
                     golden["bounds"])
    for name, (s, bounds) in list(out.items()):
        n = s.n
        P = [None] + [[0.0] + list(map(float, s.positions[i])) for i in range(n)]
        N = [None] + [[0] + [int(v) for v in s.neighbours[:, i]] for i in range(n)]
        lines = pyref.calc_delaunay_lines(P, N, n, *bounds[2:])
        out[name] = (s, P, N, lines)
    return out


@pytest.mark.parametrize("name", ["bcc_small", "voro2k"])
def test_c_model_equals_second_transcription_bit_for_bit(small_grids, name):
    """Every (store, coef), up and down, n_sweeps 1 and 3, float32 inputs: oracle/pyref.py's delaunay_model --
    pure-Python loops, its own neighbour search, geometry hoisted per layer, float32 through struct -- gives the C
    model's intensities bit for bit."""
    s, P, N, lines = small_grids[name]
    S, al, I0u, I0d = (a.astype(np.float64) for a in draw_case(s, 1, seed=7))
    for up, theta, phi, I0, layers, perm in ((True, 152.7, 315.5, I0u, s.layers_up, s.perm_up),
                                             (False, 70.3, 346.4, I0d, s.layers_down, s.perm_down)):
        k = orc.direction(theta, phi)
        lay1, perm1 = [0] + layers.tolist(), [0] + perm.tolist()
        for n_sweeps in (1, 3):
            seen = {}
            for store in STORES:
                for coef in COEFS:
                    I_c = orc.Delaunay_model(1 if up else -1, k, S[:, 0], I0[:, 0], al[:, 0], s, n_sweeps, store, coef)
                    I_py = pyref.delaunay_model(up, _one_based(k), _one_based(S[:, 0]), _one_based(I0[:, 0]),
                                                _one_based(al[:, 0]), P, N, lines, lay1, perm1, n_sweeps, store, coef)
                    assert np.array_equal(I_c, np.array(I_py[1:])), (up, n_sweeps, store, coef)
                    if store != "f64":
                        assert np.array_equal(I_c, I_c.astype(np.float32).astype(np.float64))   # stored values are floats
                    seen[store, coef] = I_c
            assert not np.array_equal(seen["layer", "f64"], seen["visit", "f64"])
            assert not np.array_equal(seen["visit", "f64"], seen["visit", "f32"])
            # a changed exponential reaches both transcriptions the same way
            I_c = orc.Delaunay_model(1 if up else -1, k, S[:, 0], I0[:, 0], al[:, 0], s, n_sweeps, "f64", "f32", 1e-3)
            I_py = pyref.delaunay_model(up, _one_based(k), _one_based(S[:, 0]), _one_based(I0[:, 0]), _one_based(al[:, 0]),
                                        P, N, lines, lay1, perm1, n_sweeps, "f64", "f32", 1e-3)
            assert np.array_equal(I_c, np.array(I_py[1:])) and not np.array_equal(I_c, seen["f64", "f32"])


@pytest.mark.parametrize("name", ["bcc_small", "voro2k"])
def test_default_model_is_the_existing_oracle_bit_for_bit(small_grids, name):
    s = small_grids[name][0]
    w, th, ph, nq = read_quadrature("ul7n12.dat")
    rng = np.random.default_rng(3)
    nlam = 2
    S = 1 + rng.random((s.n, nlam))
    al = 10 ** rng.uniform(-3, 3, (s.n, nlam))
    I0u, I0d = rng.random((s.layers_up[1] - 1, nlam)), rng.random((s.layers_down[1] - 1, nlam))
    for n_sweeps in (1, 3):
        for a in (1, 6):
            k = orc.direction(th[a], ph[a])
            if th[a] > 90:
                old = orc.Delaunay_upII(k, S[:, 0], I0u[:, 0], al[:, 0], s, n_sweeps)
                new = orc.Delaunay_model(+1, k, S[:, 0], I0u[:, 0], al[:, 0], s, n_sweeps)
            else:
                old = orc.Delaunay_downII(k, S[:, 0], I0d[:, 0], al[:, 0], s, n_sweeps)
                new = orc.Delaunay_model(-1, k, S[:, 0], I0d[:, 0], al[:, 0], s, n_sweeps)
            assert np.array_equal(old, new)
        for alpha in (al[:, 0].copy(), al, np.stack([al * (1 + 0.1 * i) for i in range(nq)])):
            old = orc.J_voronoi(w, th, ph, S, alpha, s, I0_up=I0u, I0_down=I0d, n_sweeps=n_sweeps, nthreads=4)
            J, I, Ju, Jd = orc.J_voronoi_model(w, th, ph, S, alpha, s, I0_up=I0u, I0_down=I0d, n_sweeps=n_sweeps, nthreads=4)
            assert np.array_equal(old, J)


def test_J_of_the_model_against_a_numpy_transcription(small_grids):
    """J from the model's own per-angle intensities, in numpy: the double sum of every angle in the reference's
    order ("f64"), that sum rounded to float once ("single": k_reduce_J<float>), and a float sum per direction in
    the reference's order inside the direction, then float(J_up + J_down) ("dir": patch_reduce_role / k_reduce_dir,
    then k_combine_J).  A θ = 90 angle is skipped and contributes nothing."""
    s = small_grids["voro2k"][0]
    w, th, ph, nq = read_quadrature("ul7n12.dat")
    w, th, ph = np.append(w, 0.25), np.append(th, 90.0), np.append(ph, 10.0)
    S, al, I0u, I0d = (a.astype(np.float64) for a in draw_case(s, 3))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    for store, coef in (("layer", "f64"), ("visit", "f32")):
        got = {j: orc.J_voronoi_model(w, th, ph, S, al, s, I0_up=I0u, I0_down=I0d, nthreads=4, store=store, coef=coef, jsum=j)
               for j in ("f64", "single", "dir")}
        I = got["f64"][1]
        assert np.array_equal(I, got["dir"][1]) and not I[12].any()
        for a in range(12):
            k = orc.direction(th[a], ph[a])
            I0 = I0u if th[a] > 90 else I0d
            assert np.array_equal(I[a, :, 1], orc.Delaunay_model(1 if th[a] > 90 else -1, k, S[:, 1], I0[:, 1], al[:, 1], s, 3, store, coef))
        total, Ju, Jd = np.zeros_like(S), np.zeros_like(S), np.zeros_like(S)
        for a in range(13):
            if th[a] == 90:
                continue
            total += w[a] * I[a]
            if th[a] > 90:
                Ju += w[a] * I[a]
            else:
                Jd += w[a] * I[a]
        assert np.array_equal(got["f64"][0], total)
        assert np.array_equal(got["single"][0], f32(total))
        assert np.array_equal(got["dir"][2], f32(Ju)) and np.array_equal(got["dir"][3], f32(Jd))
        assert np.array_equal(got["dir"][0], f32(f32(Ju) + f32(Jd)))
        assert not np.array_equal(got["dir"][0], got["single"][0])


@pytest.fixture(scope="module")
def gpu_inputs(bcc_small, voro_small):
    """The grids, quadrature and fields of tests/test_f32_storage.py (7 wavelengths), and each path's model on them."""
    w, th, ph, nq = read_quadrature("ul7n12.dat")
    out = {}
    for name, (pos, nbr, bounds) in (("bcc", bcc_small), ("voronoi", voro_small)):
        so = orc.make_sites(pos, nbr, bounds)
        S, al, I0u, I0d = (a.astype(np.float64) for a in draw_case(so, 7))

        def run(store, coef, jsum, exp_eps=0.0, so=so, S=S, al=al, I0u=I0u, I0d=I0d):
            J, I, _, _ = orc.J_voronoi_model(w, th, ph, S, al, so, I0_up=I0u, I0_down=I0d, nthreads=8, store=store, coef=coef,
                                             jsum=jsum, exp_eps=exp_eps)
            return J, I
        out[name] = run
    return out


@pytest.mark.parametrize("grid", ["bcc", "voronoi"])
@pytest.mark.parametrize("path", sorted(PATH_MODEL))
def test_reference_alone_meets_the_conditions_of_the_gpu_tests(gpu_inputs, grid, path):
    """Each path's model against a copy of itself whose every exp(-Δτ) is changed by 2e-13 relative -- the coarsest
    device exponential ever quoted, a hundred times the difference of the exponentials in use (3e-15) -- on the GPU
    file's inputs: I of every angle and J stay at >= 99.9 % bit-identical floats, the rest within 2 ulps.  So the
    conditions of tests/test_f32_storage.py are ones a correct kernel meets.  Also: how far each model is from the fp64
    oracle -- the float rounding that the 5e-6 of the large fp32 tests is a margin over."""
    run = gpu_inputs[grid]
    m = PATH_MODEL[path]
    J, I = run(**m)
    Jp, Ip = run(**m, exp_eps=EXP_EPS)
    worst, far = 0, 0.0
    for a in range(I.shape[0]):
        ok, ndiff, size, ulps = within_conditions(Ip[a], I[a])
        worst, far = max(worst, ndiff), max(far, ulps)
        assert ok, (a, ndiff, size, ulps)
    ok, ndiff, size, ulps = within_conditions(Jp, J)
    print(f"{grid} {path}: exp changed by {EXP_EPS:g}: at most {worst} of {I[0].size} elements of an angle's I differ, "
          f"{ndiff} of {size} of J, largest distance {max(far, ulps):g} ulp")
    assert ok, (ndiff, size, ulps)
    J64, I64 = run("f64", "f64", "f64")
    dI = np.abs(I - I64)[I64 != 0] / np.abs(I64)[I64 != 0]
    dJ = np.abs(J / J64 - 1)
    print(f"{grid} {path}: model against the fp64 oracle: I {dI.max():.2e}, J {dJ.max():.2e} (max relative)")
    assert 1e-9 < dI.max() < 2.5e-7 and dJ.max() < 2.5e-7       # a few float roundings (2^-24 = 6e-8 each), nowhere near 5e-6


@pytest.mark.parametrize("grid", ["bcc", "voronoi"])
def test_models_are_distinguishable_on_the_inputs_of_the_gpu_tests(gpu_inputs, grid):
    """Rounding a layer when it is complete against rounding every visit, float against double coefficients, and each
    pair of the paths' models: more than 1 % of the elements of every angle's I and of J differ -- ten times what
    the GPU file lets a kernel differ from its model -- so a kernel that rounds in another place than its model says
    fails there."""
    run = gpu_inputs[grid]
    pm = {k: tuple(v.values()) for k, v in PATH_MODEL.items()}
    for name, m1, m2 in (("layer | visit", ("layer", "f64", "dir"), ("visit", "f64", "dir")),
                         ("coef f64 | f32", ("visit", "f64", "dir"), ("visit", "f32", "dir")),
                         ("coef f64 | f32 (store layer)", ("layer", "f64", "dir"), ("layer", "f32", "dir")),
                         ("patches | steps", pm["patches"], pm["steps"]), ("levels | steps", pm["levels"], pm["steps"]),
                         ("levels | patches", pm["levels"], pm["patches"])):
        (J1, I1), (J2, I2) = run(*m1), run(*m2)
        shares = [float_compare(I1[a], I2[a])[0] / I1[a].size for a in range(I1.shape[0])]
        jshare = float_compare(J1, J2)[0] / J1.size
        print(f"{grid} {name}: I differs in {min(shares):.1%} .. {max(shares):.1%} of an angle's elements, J in {jshare:.1%}")
        assert min(shares) > 0.01 and jshare > 0.01, name
