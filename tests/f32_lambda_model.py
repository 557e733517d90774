"""What tests/test_f32_lambda_host.py (CPU) and tests/test_f32_lambda.py (GPU) share: the line Λ-iteration restated with
the storage model of the fp32 value path, the numpy model of the float update step, and the oracle-only figures the GPU
file takes its bounds from.  Nothing here touches the device.

Where the float loop rounds (include/voronoirt.h, vrt_lambda_create_f32):
  B_0 and I_0         rounded to float once, at create
  α                   the double opacity rounded to float (k_line_opacity<float2>)
  J                   the patch path's storage model (oracle/f32_model.py: PATH_MODEL["patches"])
  S_new               f32((1 - ε) J + ε B) with the float J and B widened (k_lambda_update_native_f32)
  rates, populations  double arithmetic on the widened float J (k_rates_populations<true, float>)
"""
import numpy as np

import voronoirt_amd as vrt
from oracle import oracle as orc
from oracle import update_ref
from oracle.f32_model import EXP_EPS, PATH_MODEL
from oracle.update_ref import f32

QUADRATURE = "ul7n12.dat"
ALPHA_EPS = 1e-13               # the coarsest error of the device opacity the project quotes (EXP_EPS: of its exponential)


def update_model(J_up, J_down, B, S_old, eps, nlam=None):
    """numpy model of vrt_lambda_update_native_dev_f32 on caller-layout float32 arrays (n, nlam) (either J may be None):
    (J, S_new as float32, the criterion's scalar).  It is the "line_f32" kind of oracle/update_ref.py, which holds the
    operations."""
    u = update_ref.update_model("line_f32", J_up, B, eps, S_old, J_down=J_down, nlam=nlam)
    return u.parts["J"].astype(np.float32), u.S_new.astype(np.float32), u.scalar


def model_lambda_iteration(case, so, maxiter, exp_eps=0.0, alpha_eps=0.0):
    """_oracle_lambda_iteration (tests/test_physics.py) with the storage model: the state after EVERY iterate as a list of
    (J, S_new, populations) and the history.  exp_eps, alpha_eps: every exponential of the solve and every α changed by
    that relative amount (the perturbed copy that stands for a device whose roundings differ from libm's)."""
    w, th, ph, nq = vrt.read_quadrature(QUADRATURE)
    B0 = f32(case.B0)
    pops, S_new = case.lte.copy(), B0.copy()
    bottom = so.perm_up[: so.layers_up[1] - 1] - 1
    eps = np.asarray(case.eps)[:, None]
    states, hist = [], []
    for _ in range(maxiter):
        S_old = S_new
        gamma, strength = orc.line_terms(case.gamma_static, case.gamma_unsold, pops, case.strength_const, case.Bij, case.Bji)
        alpha = np.stack([orc.line_opacity(orc.direction(th[a], ph[a]), case.lam, case.lambda0, case.c0, case.velocity,
                                           case.doppler, gamma, strength, case.alpha_cont) for a in range(nq)])
        alpha = f32(alpha * (1.0 + alpha_eps))
        J = orc.J_voronoi_model(w, th, ph, S_old, alpha, so, I0_up=B0[bottom], nthreads=8, exp_eps=exp_eps,
                                **PATH_MODEL["patches"])[0]
        S_new = f32((1.0 - eps) * J + eps * B0)
        hist.append(float(np.abs(1.0 - S_old / S_new).max()))
        R = orc.calculate_R(case.lam, case.blocks, J, case.planck2, case.lambda0, case.c0, case.doppler, gamma,
                            case.sigma_bb_const, case.sigma_bf1, case.sigma_bf2, case.temperature, case.lte,
                            case.hc_over_kB, case.pref_ij, case.pref_ji)
        pops = orc.revised_populations(R, case.C, case.atom_density)
        states.append((J, S_new, pops))
    return states, hist


def f64_lambda_iteration(case, so, maxiter):
    """the fp64 oracle loop (_oracle_lambda_iteration), keeping the state after every iterate"""
    w, th, ph, nq = vrt.read_quadrature(QUADRATURE)
    pops, S_new = case.lte.copy(), case.B0.copy()
    bottom = so.perm_up[: so.layers_up[1] - 1] - 1
    eps = np.asarray(case.eps)[:, None]
    states = []
    for _ in range(maxiter):
        S_old = S_new
        gamma, strength = orc.line_terms(case.gamma_static, case.gamma_unsold, pops, case.strength_const, case.Bij, case.Bji)
        alpha = np.stack([orc.line_opacity(orc.direction(th[a], ph[a]), case.lam, case.lambda0, case.c0, case.velocity,
                                           case.doppler, gamma, strength, case.alpha_cont) for a in range(nq)])
        J = orc.J_voronoi(w, th, ph, S_old, alpha, so, I0_up=case.B0[bottom], nthreads=8)
        S_new = (1 - eps) * J + eps * case.B0
        R = orc.calculate_R(case.lam, case.blocks, J, case.planck2, case.lambda0, case.c0, case.doppler, gamma,
                            case.sigma_bb_const, case.sigma_bf1, case.sigma_bf2, case.temperature, case.lte,
                            case.hc_over_kB, case.pref_ij, case.pref_ji)
        pops = orc.revised_populations(R, case.C, case.atom_density)
        states.append((J, S_new, pops))
    return states


def deviations(a, b):
    """(J: max |ΔJ| / max |J|, S: max relative, populations: max relative) of two states (J, S, populations); J is 0 at the
    never-solved site perm_up[n], hence its absolute measure"""
    (Ja, Sa, pa), (Jb, Sb, pb) = a, b
    return (float(np.abs(Ja - Jb).max() / np.abs(Jb).max()), float(np.abs(Sa / Sb - 1).max()), float(np.abs(pa / pb - 1).max()))


_runs = {}


def oracle_runs(pos, nbr, bounds, maxiter):
    """{"case", "so", "model", "hist", "perturbed", "f64"}: the model loop, its perturbed copy and the fp64 oracle loop on
    _lambda_case(pos, bounds, 11), `maxiter` iterates each, computed once per process and left unchanged"""
    from test_physics import _lambda_case
    if maxiter not in _runs:
        so = orc.make_sites(pos, nbr, bounds)
        case = _lambda_case(pos, bounds, 11)
        model, hist = model_lambda_iteration(case, so, maxiter)
        perturbed, _ = model_lambda_iteration(case, so, maxiter, exp_eps=EXP_EPS, alpha_eps=ALPHA_EPS)
        out = dict(case=case, so=so, model=model, hist=hist, perturbed=perturbed, f64=f64_lambda_iteration(case, so, maxiter))
        for key in ("model", "perturbed", "f64"):
            for state in out[key]:
                for a in state:
                    a.setflags(write=False)
        _runs[maxiter] = out
    return _runs[maxiter]
