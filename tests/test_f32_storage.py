"""GPU tests (-m gpu) of the fp32 storage path (S, α, I_0, I, J held as float, arithmetic fp64) against the
storage-model oracle (oracle/vrt_oracle.c: orc_delaunay_model; oracle/f32_model.py says which model each device path
implies and names the kernels it was read off): the per-angle intensities and J of every path must be the model's floats BIT FOR
BIT in at least 99.9 % of the elements and within 2 float ulps in the rest.  tests/test_f32_model_host.py shows that
the model alone meets both under an exponential changed by 2e-13, and that a model that rounds in another place
misses the first by a factor of 25 or more -- which the 5e-6 of the older fp32 tests cannot see.
Also: scaling S and I_0 by 2^-100 and 2^+100 scales the float results bit for bit (no absolute threshold, clamp or
flush in the conversions), 2^-140 puts every stored value among the float subnormals, and the float form of the
opacity prologue writes the float rounding of what its double form writes."""
import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from oracle.f32_model import PATH_MODEL, draw_case, within_conditions
from voronoirt_amd import _lib

pytestmark = pytest.mark.gpu

W, TH, PH, NQ = vrt.read_quadrature("ul7n12.dat")
DIRS = [1 if t > 90 else -1 for t in TH]


@pytest.fixture(scope="module")
def grids(bcc_small, voro_small):
    out = {}
    for name, (pos, nbr, bounds) in (("bcc", bcc_small), ("voronoi", voro_small)):
        out[name] = (vrt.VoronoiSites(pos, nbr, bounds, device=0), orc.make_sites(pos, nbr, bounds))
    yield out
    for hs, _ in out.values():
        hs.close()


_model_runs = {}


def _model(so, key, path, S, al, I0u, I0d, n_sweeps=3):
    """(J, I, J_up, J_down) of the path's model, computed once per `key` and shared"""
    if key not in _model_runs:
        f = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
        _model_runs[key] = orc.J_voronoi_model(W, TH, PH, f(S), f(al), so, I0_up=f(I0u), I0_down=f(I0d), n_sweeps=n_sweeps,
                                               nthreads=8, **PATH_MODEL[path])
        for a in _model_runs[key]:
            a.setflags(write=False)
    return _model_runs[key]


def _device(hs, monkeypatch, path, S, al, amode, I0u, I0d, n_sweeps=3, chain=None, env=None):
    """J (n, nlam) and the per-angle I (angles, n, nlam) of vrt_plan_execute_dev_f32 on `path`, and the plan's launches"""
    import torch
    monkeypatch.setenv("VRT_PATH", path)                   # read when the plan is created
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    plan = vrt.FormalPlan(hs, vrt.quadrature_directions(TH, PH), n_sweeps, dirs=DIRS)
    if chain is not None:
        plan.set_option("VRT_PATCH_CHAIN", chain)
    dev = torch.device("cuda", 0)
    n, nlam = S.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    Sd, Ad, Ud, Dd = t(S), t(al), t(I0u), t(I0d)
    Jd = torch.full((n, nlam), float("nan"), dtype=torch.float32, device=dev)
    Id = torch.full((NQ, n, nlam), float("nan"), dtype=torch.float32, device=dev)
    plan.execute_dev(nlam, nlam, Sd.data_ptr(), Ad.data_ptr(), amode, W, dJ=Jd.data_ptr(), dI0_up=Ud.data_ptr(),
                     dI0_down=Dd.data_ptr(), dI_out=Id.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, f32=True)
    torch.cuda.synchronize()
    plan.check()
    assert plan.last_path == path
    launches = plan.last_launches
    plan.close()
    return Jd.cpu().numpy(), Id.cpu().numpy(), launches


def _assert_is_the_model(label, J, I, ref):
    """the two conditions for I of every angle and for J; prints the differing count and the largest ulp distance"""
    Jm, Im = ref[0], ref[1]
    results = [within_conditions(I[a], Im[a]) for a in range(NQ)] + [within_conditions(J, Jm)]
    print(f"{label}: I differs in at most {max(r[1] for r in results[:-1])} of {results[0][2]} elements of an angle "
          f"({sum(r[1] for r in results[:-1])} of {NQ * results[0][2]} in all), largest distance {max(r[3] for r in results[:-1]):g} ulp; "
          f"J in {results[-1][1]} of {results[-1][2]}, {results[-1][3]:g} ulp")
    for a, r in enumerate(results):
        assert r[0], (label, "J" if a == NQ else f"angle {a}", r[1:])


# patches: nλ = 4 and 7 (padded last pair) have an even pair count -> k_patch_quad / quad_pairs; 6 (three pairs) -> the
# pair kernel (k_patch_lean / lean_pairs); 1 (a single pair) -> k_patch_solve; chain 1: every layer in one launch, 0: one launch per layer (the J
# reduction then rides in patch_reduce_role instead of chain_reduce).  steps: k_step_coeffs<float, true> +
# k_step_levels1<float, K> for every float run.  levels: k_sweep_level<float> + k_reduce_J<float>.
@pytest.mark.parametrize("grid", ["voronoi", "bcc"])
@pytest.mark.parametrize("path, nlam, chain", [("patches", 4, None), ("patches", 7, 1), ("patches", 7, 0), ("patches", 6, None),
                                               ("patches", 1, None), ("steps", 7, None), ("steps", 1, None),
                                               ("levels", 7, None), ("levels", 1, None)])
def test_every_path_is_its_storage_model(grids, monkeypatch, grid, path, nlam, chain):
    """I of every angle and J of each device path against the model its code implies (oracle/f32_model.py), with
    boundary intensities for up AND down rays, α per (site, wavelength)."""
    hs, so = grids[grid]
    S, al, I0u, I0d = draw_case(so, nlam)
    J, I, launches = _device(hs, monkeypatch, path, S, al, _lib.ALPHA_SITE_LAM, I0u, I0d, chain=chain)
    if chain is not None:
        assert (launches == 1) == bool(chain)
    _assert_is_the_model(f"{grid} {path} nlam {nlam}" + ("" if chain is None else f" chain {chain}"), J, I,
                         _model(so, (grid, path, nlam), path, S, al, I0u, I0d))
    for a in range(NQ):                   # the never-visited last site of the direction keeps I = 0
        assert not I[a, (so.perm_up if TH[a] > 90 else so.perm_down)[-1] - 1].any()


@pytest.mark.parametrize("K, Q", [(2, 1), (1, 2)])
def test_generic_patch_kernel_is_the_same_model(grids, monkeypatch, K, Q):
    """k_patch_solve<float, AM, K, Q, NT> (several entries per thread / pairs per workgroup; the launches above take the
    one-entry kernels), patches of ~90 sites so that every layer is split and most entries are halo: its from_d2<float>
    store is the same single rounding."""
    hs, so = grids["voronoi"]
    S, al, I0u, I0d = draw_case(so, 6)
    env = {"VRT_PATCH_K": str(K), "VRT_PATCH_Q": str(Q), "VRT_PATCH_NT": "256", "VRT_PATCH_LEAN": "0", "VRT_PATCH_CHAIN": "0",
           "VRT_PATCH_QUAD": "0", "VRT_PATCH_OWN": "90", "VRT_PATCH_TARGET": "4096"}
    J, I, launches = _device(hs, monkeypatch, "patches", S, al, _lib.ALPHA_SITE_LAM, I0u, I0d, env=env)
    assert launches > 1
    _assert_is_the_model(f"voronoi patches k_patch_solve K {K} Q {Q}", J, I, _model(so, ("voronoi", "patches", 6), "patches", S, al, I0u, I0d))


@pytest.mark.parametrize("layout", ["site", "angle"])
def test_default_path_alpha_layouts(grids, monkeypatch, layout):
    """ALPHA_SITE and ALPHA_ANGLE_SITE_LAM on the default path (ALPHA_SITE_LAM: the test above)."""
    hs, so = grids["voronoi"]
    nlam = 7
    S, al, I0u, I0d = draw_case(so, nlam, n_angles=NQ if layout == "angle" else 0)
    if layout == "site":
        al = np.ascontiguousarray(al[:, 0])
    amode = _lib.ALPHA_SITE if layout == "site" else _lib.ALPHA_ANGLE_SITE_LAM
    J, I, _ = _device(hs, monkeypatch, "patches", S, al, amode, I0u, I0d)
    _assert_is_the_model(f"voronoi patches alpha per {layout}", J, I, _model(so, ("voronoi", layout), "patches", S, al, I0u, I0d))


@pytest.mark.parametrize("path", ["patches", "steps"])
def test_one_sweep(grids, monkeypatch, path):
    """n_sweeps = 1 (3: everywhere else): one visit per site, in the direction's order."""
    hs, so = grids["voronoi"]
    S, al, I0u, I0d = draw_case(so, 7)
    J, I, _ = _device(hs, monkeypatch, path, S, al, _lib.ALPHA_SITE_LAM, I0u, I0d, n_sweeps=1)
    _assert_is_the_model(f"voronoi {path} one sweep", J, I, _model(so, ("voronoi", path, "one sweep"), path, S, al, I0u, I0d, n_sweeps=1))


def test_sweep_order_float_planes(grids, monkeypatch):
    """vrt_plan_execute_native_dev_f32: S read from and J reduced into sweep-order float planes.  J_up and J_down are
    the model's per-direction float sums, and vrt_plan_j_from_native_dev_f32 combines them as the model does."""
    import torch
    monkeypatch.delenv("VRT_PATH", raising=False)
    hs, so = grids["voronoi"]
    n, nlam = so.n, 7
    S, al, I0u, I0d = draw_case(so, nlam)
    plan = vrt.FormalPlan(hs, vrt.quadrature_directions(TH, PH), 3, dirs=DIRS)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    dS, dA, dU, dD = t(S), t(al), t(I0u), t(I0d)
    count = plan.native_plane_count(nlam)
    S_up, S_dn, J_up, J_dn = (torch.full((count,), float("nan"), dtype=torch.float32, device=dev) for _ in range(4))
    dal = torch.full((2 * count,), float("nan"), dtype=torch.float32, device=dev)
    plan.to_native_dev(nlam, nlam, dS.data_ptr(), S_up.data_ptr(), S_dn.data_ptr(), stream=st, f32=True)
    plan.to_native_dev(nlam, nlam, dA.data_ptr(), dal.data_ptr(), dal.data_ptr() + 4 * count, stream=st, f32=True)
    plan.execute_native_dev(nlam, S_up.data_ptr(), S_dn.data_ptr(), dal.data_ptr(), _lib.ALPHA_SITE_LAM_NATIVE, W,
                            dJ_up=J_up.data_ptr(), dJ_down=J_dn.data_ptr(), dI0_up=dU.data_ptr(), dI0_down=dD.data_ptr(),
                            stream=st, f32=True)
    assert plan.last_path == "patches"
    out = {}
    for name, d, buf in (("J_up", 1, J_up), ("J_down", -1, J_dn)):
        out[name] = torch.full((n, nlam), float("nan"), dtype=torch.float32, device=dev)
        plan.from_native_dev(d, nlam, nlam, buf.data_ptr(), out[name].data_ptr(), stream=st, f32=True)
    out["J"] = torch.full((n, nlam), float("nan"), dtype=torch.float32, device=dev)
    plan.J_from_native_dev(nlam, nlam, J_up.data_ptr(), J_dn.data_ptr(), out["J"].data_ptr(), stream=st, f32=True)
    torch.cuda.synchronize()
    plan.check()
    plan.close()
    Jm, _, Jum, Jdm = _model(so, ("voronoi", "patches", nlam), "patches", S, al, I0u, I0d)
    for name, want in (("J_up", Jum), ("J_down", Jdm), ("J", Jm)):
        ok, ndiff, size, ulps = within_conditions(out[name].cpu().numpy(), want)
        print(f"voronoi sweep-order float planes {name}: differs in {ndiff} of {size}, largest distance {ulps:g} ulp")
        assert ok, (name, ndiff, size, ulps)


@pytest.mark.parametrize("path", ["patches", "steps"])
def test_scaling_by_powers_of_two_is_exact(grids, monkeypatch, path):
    """Everything between the loads and the stores is fp64 and linear in (S, I_0), so S and I_0 times 2^-100 or 2^+100
    -- both inside float's normal range -- give the unscaled float I and J times that power bit for bit: there is no
    absolute threshold, clamp or flush in the float conversions."""
    hs, so = grids["voronoi"]
    S, al, I0u, I0d = draw_case(so, 7)
    J, I, _ = _device(hs, monkeypatch, path, S, al, _lib.ALPHA_SITE_LAM, I0u, I0d)
    for e in (-100, 100):
        f = np.float32(2.0) ** np.float32(e)
        assert np.isfinite(I * f).all() and (np.abs(I[I != 0] * f) >= np.finfo(np.float32).tiny).all()
        Js, Is, _ = _device(hs, monkeypatch, path, S * f, al, _lib.ALPHA_SITE_LAM, I0u * f, I0d * f)
        assert np.array_equal(Is, I * f) and np.array_equal(Js, J * f), (path, e)


@pytest.mark.parametrize("path", ["patches", "steps"])
def test_float_subnormals_underflow_gradually(grids, monkeypatch, path):
    """S and I_0 times 2^-140: every stored intensity is a float subnormal (9 to 10 significant bits).  The device keeps
    them -- conversions in both directions, the float coefficients of the step path -- as IEEE gradual underflow does,
    which is what the model's casts do: the same conditions hold against the model fed the same subnormal inputs."""
    hs, so = grids["voronoi"]
    S, al, I0u, I0d = draw_case(so, 7)
    f = 2.0 ** -140
    sub = lambda a: (a.astype(np.float64) * f).astype(np.float32)
    S, I0u, I0d = sub(S), sub(I0u), sub(I0d)
    assert 0 < S.min() and S.max() < np.finfo(np.float32).tiny
    J, I, _ = _device(hs, monkeypatch, path, S, al, _lib.ALPHA_SITE_LAM, I0u, I0d)
    assert np.abs(I).max() < np.finfo(np.float32).tiny and (I != 0).mean() > 0.99 and (J != 0).mean() > 0.99
    _assert_is_the_model(f"voronoi {path} subnormal", J, I, _model(so, ("voronoi", path, "subnormal"), path, S, al, I0u, I0d))


def test_float_opacity_is_the_rounded_double_opacity(grids):
    """vrt_line_opacity_dev_f32 on the 51-wavelength case of test_gpu_f32_storage_accepts_native_per_angle_alpha: the
    same kernel with a float store, so its native buffer is the float rounding of what vrt_line_opacity_dev writes
    (the pad wavelength of the last pair is unspecified and not compared)."""
    import torch
    from test_physics import C0, _line_case
    hs, so = grids["voronoi"]
    c = _line_case(hs.n, 3)
    nlam = 51
    lam = c["lam"][:nlam]
    scale = 3e4 / c["strength"].max() * c["doppler"].mean()
    strength, alpha_cont = c["strength"] * scale, c["alpha_cont"] * 1e5
    plan = vrt.FormalPlan(hs, vrt.quadrature_directions(TH, PH), 3, dirs=DIRS)
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_vel, d_dop, d_gam, d_str, d_ac = t(c["velocity"]), t(c["doppler"]), t(c["gamma"]), t(strength), t(alpha_cont)
    st = torch.cuda.current_stream().cuda_stream
    count = plan.native_alpha_count(nlam)
    got = {}
    for f32, dt in ((False, torch.float64), (True, torch.float32)):
        native = torch.full((count,), float("nan"), dtype=dt, device=dev)
        plan.line_opacity_dev(lam, c["lambda0"], C0, d_vel.data_ptr(), d_dop.data_ptr(), d_gam.data_ptr(), d_str.data_ptr(),
                              d_ac.data_ptr(), native.data_ptr(), stream=st, f32=f32)
        torch.cuda.synchronize()
        got[f32] = plan.native_to_site_major(native.cpu().numpy(), nlam, NQ)
    plan.close()
    assert np.isfinite(got[False]).all() and (got[False] > 0).all()
    ok, ndiff, size, ulps = within_conditions(got[True], got[False].astype(np.float32))
    print(f"float opacity against the rounded double opacity: differs in {ndiff} of {size}, largest distance {ulps:g} ulp")
    assert ok, (ndiff, size, ulps)
