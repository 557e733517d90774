#!/usr/bin/env python3
"""diagnostics: every bit a Λ-iteration session hands back, as text, to compare two builds of the library byte for byte.

For the raster line session (vrt_regular_lambda_*), the raster continuum session (vrt_regular_continuum_*) and -- with
--voronoi -- the Voronoi line and continuum sessions (vrt_lambda_*, vrt_continuum_*, in sweep-order planes and in rows) it
runs eight iterates each of: plain, diagonal operator, Ng (4, 4), diagonal + Ng, and resumed (three iterates, then the
state through *_set_state / *_set_source into a FRESH session, five more there).  Per iterate it prints the criterion as a
hex double, Ng's (applied, sums, coeffs), the line sessions' fallback count and the SHA-256 of every array *_get returns.
The raster has 7 x 6 x 5 ghosted points and 3 wavelengths; the Voronoi grid is tests/golden/voro2k (9 line, 3 continuum
wavelengths).  With --multi it runs the multi-device line session (vrt_multi_lambda_*) instead, over 1, 2 and 3 handles of
device 0 (9 wavelengths in blocks of 9; 5, 4; 3, 3, 3) on the 1500-site grid of the tests: double storage in sweep order and
in rows, float storage, and double storage in sweep order with Ng (4, 4); plain and resumed each.

    python tools/session_bits.py [--voronoi | --multi] > branch.txt
    VRT_LIB_PATH=/path/to/parent/libvrt_hip.so python tools/session_bits.py [--voronoi | --multi] > parent.txt
    diff parent.txt branch.txt          # must be empty (profiles/raster_store/INDEX.md, profiles/multi_members/INDEX.md)
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import voronoirt_amd as vrt                     # noqa: E402
from voronoirt_amd import _lib, api, synth      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--voronoi", action="store_true", help="the Voronoi line and continuum sessions on voro2k instead")
ap.add_argument("--multi", action="store_true", help="the multi-device line session over 1, 2 and 3 handles of device 0 instead")
args = ap.parse_args()

QUAD = "ul7n12.dat"
ITERATES, RESUME_AT = 8, 3
MODES = [("plain", 0, None), ("diagonal", 1, None), ("ng", 0, (4, 4)), ("diagonal+ng", 1, (4, 4))]
L = _lib.load()
d = lambda a: a.ctypes.data_as(_lib.p_dbl)
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
hexes = lambda xs: " ".join(float(x).hex() for x in xs)


class Session:
    """one of the four sessions through the C entries; `line`: five arrays come home and the state has populations"""

    def __init__(self, prefix, create, n, nlam, line, has_operator=None):
        self.prefix, self.n, self.nlam, self.line = prefix, n, nlam, line
        self.has_operator = line if has_operator is None else has_operator      # (the multi-device session has none)
        self.h = ctypes.c_void_p()
        api.check(create(ctypes.byref(self.h)))

    def fn(self, name):
        return getattr(L, f"{self.prefix}_{name}")

    def operator(self, op):
        name = "use_operator" if self.line else "select_operator" if self.prefix == "vrt_regular_continuum" else "set_operator"
        api.check(self.fn(name)(self.h, op))

    def get(self):
        n, nlam = self.n, self.nlam
        out = [np.zeros((n, nlam)), np.zeros((n, nlam))]
        if self.line:
            out += [np.zeros((3, n)), np.zeros((n, 3, 3)), np.zeros(n)]
        api.check(self.fn("get")(self.h, *(d(a) for a in out)))
        return out                                  # J, S (, populations, R, gamma)

    def set_state(self, arrays):
        S = np.ascontiguousarray(arrays[1])
        if self.line:
            api.check(self.fn("set_state")(self.h, d(S), d(np.ascontiguousarray(arrays[2]))))
        else:
            api.check(self.fn("set_source")(self.h, d(S)))

    def iterate(self, it):
        """one iterate, and everything the session can say about it as one line"""
        crit = ctypes.c_double()
        api.check(self.fn("iterate")(self.h, ctypes.byref(crit)))
        applied, sums, coeffs = ctypes.c_int(9), np.zeros(5), np.zeros(2)
        api.check(self.fn("last_acceleration")(self.h, ctypes.byref(applied), d(sums), d(coeffs)))
        words = [f"{it}", crit.value.hex(), f"ng {applied.value} [{hexes(sums)}] [{hexes(coeffs)}]"]
        if self.has_operator:
            op, fallback = ctypes.c_int(), ctypes.c_int64(-1)
            api.check(self.fn("get_operator")(self.h, ctypes.byref(op), ctypes.byref(fallback)))
            words.append(f"op {op.value} fallback {fallback.value}")
        words += [sha(a) for a in self.get()]
        return "  ".join(words)

    def close(self):
        self.fn("destroy")(self.h)


def run_all(label, make, modes=MODES):
    for name, op, ng in modes:
        s = make()
        if op:
            s.operator(op)
        if ng:
            api.check(s.fn("set_acceleration")(s.h, 2, *ng))
        print(f"== {label}: {name}")
        for it in range(1, ITERATES + 1):
            print(s.iterate(it))
        s.close()
    first = make()
    print(f"== {label}: resumed after {RESUME_AT}")
    for it in range(1, RESUME_AT + 1):
        print(first.iterate(it))
    state = first.get()
    first.close()                                   # (a regular handle serves one session at a time)
    fresh = make()
    fresh.set_state(state)
    for it in range(RESUME_AT + 1, ITERATES + 1):
        print(fresh.iterate(it))
    fresh.close()


def raster_sessions():
    w, k, dirs = api._regular_directions(QUAD)
    kd, wd = np.ascontiguousarray(k, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
    z, x, y, kw = synth.three_wavelength_line_case(5, 5, 4, seed=7)            # 5 x 7 x 6 ghosted points, 3 wavelengths
    lc, keep = vrt.LineCase(**kw).c_struct()
    n = int(keep["doppler"].size)
    solver = api._regular_solver(z, x, y, n, 0)
    create = lambda out: L.vrt_regular_lambda_create(solver._h, kd.shape[0], d(kd), dirs.ctypes.data_as(_lib.p_int), d(wd),
                                                     ctypes.byref(lc), 3, out)
    run_all("raster line 7x6x5 x 3", lambda: Session("vrt_regular_lambda", create, n, 3, True))
    solver.close()
    z, x, y, kw = synth.regular_continuum_case(5, 5, 4, 7, 3)
    case = vrt.ContinuumCase(**kw)
    cc = case.c_struct()
    solver = api._regular_solver(z, x, y, case.n, 0)
    create = lambda out: L.vrt_regular_continuum_create(solver._h, kd.shape[0], d(kd), dirs.ctypes.data_as(_lib.p_int), d(wd),
                                                        ctypes.byref(cc), 3, out)
    run_all("raster continuum 7x6x5 x 3", lambda: Session("vrt_regular_continuum", create, case.n, 3, False))
    solver.close()


def voronoi_line_case(pos, bounds, nbb=5, nbf=2, seed=11):
    """a two-level atom with continuum on the sites (the magnitudes of synth.regular_line_case)"""
    c0, kB, h_pl = 2.99792458e8, 1.380649e-23, 6.62607015e-34
    n, rng, lambda0 = pos.shape[0], np.random.default_rng(seed), 121.567e-9
    q = np.concatenate([-np.geomspace(600, 0.05, nbb // 2), [0.0], np.geomspace(0.05, 600, nbb // 2)])
    lam = np.concatenate([lambda0 * (1 + q * 2.5e3 / c0), np.linspace(22.8e-9, 91.17e-9, nbf), np.linspace(91.2e-9, 364.7e-9, nbf)])
    nlam = lam.size
    zeta, box = (pos[:, 0] - bounds[0]) / (bounds[1] - bounds[0]), bounds[1] - bounds[0]
    T = 6e3 + 6e3 * zeta + 200 * rng.random(n)
    doppler = lambda0 / c0 * np.sqrt(2 * kB * T / 1.6735575e-27)
    n1 = 1e16 * np.exp(-3 * zeta) * (1 + 0.1 * rng.random(n))
    lte = np.stack([n1, n1 * 1e-3 * (1 + rng.random(n)), n1 * 1e-2 * (1 + rng.random(n))])
    Cm = 10 ** rng.uniform(-1, 1, (n, 3, 3))
    for k in range(3):
        Cm[:, k, k] = 0.0
    return vrt.LineCase(
        lam=lam, blocks=np.array([0, nbb, nbb, nbb + nbf, nbb + nbf, nlam], dtype=np.int64), lambda0=lambda0, c0=c0,
        velocity=rng.normal(0, 3e3, (n, 3)), doppler=doppler, gamma_static=4.702e8 + 10 ** rng.uniform(7, 8.7, n),
        gamma_unsold=10 ** rng.uniform(-8.5, -7.5, n), alpha_cont=0.05 / box * np.exp(-2 * zeta),
        eps=10 ** rng.uniform(-2.5, -0.5, n), temperature=T, atom_density=lte.sum(axis=0),
        B0=(1.0 + zeta)[:, None] * (1 + 0.05 * rng.random((n, nlam))), lte=lte, C=Cm, planck2=2.0 * (lambda0 / lam) ** 5,
        sigma_bf1=1e-21 * (lam[nbb:nbb + nbf] / lam[nbb + nbf - 1]) ** 3, sigma_bf2=2e-21 * (lam[nbb + nbf:] / lam[-1]) ** 3,
        strength_const=60.0 / box * doppler.mean() / n1.mean(), Bij=1.0, Bji=0.25, sigma_bb_const=2e-32,
        hc_over_kB=h_pl * c0 / kB, pref_ij=2e36, pref_ji=2e37)


def voronoi_sessions():
    golden = os.path.join(ROOT, "tests", "golden")
    meta = json.load(open(os.path.join(golden, "voro2k_meta.json")))
    pos = np.ascontiguousarray(np.loadtxt(os.path.join(golden, "voro2k_sites.txt"))[:, [3, 1, 2]])    # file: id x y z
    bounds = tuple(meta["bounds"])
    lc, keep = voronoi_line_case(pos, bounds).c_struct()
    case = vrt.ContinuumCase(**synth.continuum_case(pos, bounds, 3, seed=5))
    cc = case.c_struct()
    w, th, ph, _ = vrt.read_quadrature(QUAD)
    wd = np.ascontiguousarray(w, dtype=np.float64)
    for form, native in (("planes", "1"), ("rows", "0")):
        os.environ["VRT_LAMBDA_NATIVE"] = native               # read when a plan is made
        sites = vrt.read_cell(os.path.join(golden, "voro2k_neighbours.txt"), meta["n"], pos, bounds)
        plan = vrt.FormalPlan(sites, vrt.quadrature_directions(th, ph), 3, dirs=[1 if t > 90 else (-1 if t < 90 else 0) for t in th])
        create = lambda out: L.vrt_lambda_create(plan._h, ctypes.byref(lc), d(wd), out)
        run_all(f"voro2k line x 9, {form}", lambda: Session("vrt_lambda", create, sites.n, 9, True))
        create = lambda out: L.vrt_continuum_create(plan._h, ctypes.byref(cc), d(wd), out)
        run_all(f"voro2k continuum x 3, {form}", lambda: Session("vrt_continuum", create, sites.n, 3, False))
        plan.close()
        sites.close()


def multi_sessions():
    pos, nbr, bounds = synth.voronoi_grid(1500, seed=5, bounds=(0.0, 2.0, 0.0, 1.0, 0.0, 1.0), scale_height=0.7)
    lc, keep = voronoi_line_case(pos, bounds).c_struct()
    w, th, ph, _ = vrt.read_quadrature(QUAD)
    wd = np.ascontiguousarray(w, dtype=np.float64)
    k, dirs = vrt.quadrature_directions(th, ph), [1 if t > 90 else -1 for t in th]
    variants = (("planes", "1", L.vrt_multi_lambda_create, MODES[:1]), ("rows", "0", L.vrt_multi_lambda_create, MODES[:1]),
                ("float planes", "1", L.vrt_multi_lambda_create_f32, MODES[:1]), ("planes", "1", L.vrt_multi_lambda_create, MODES[2:3]))
    for W in (1, 2, 3):
        for form, native, entry, modes in variants:
            os.environ["VRT_LAMBDA_NATIVE"] = native               # read when the members' plans are made
            mp = vrt.MultiDevicePlan(pos, nbr, bounds, k, dirs=dirs, devices=(0,) * W)
            create = lambda out: entry(mp._h, ctypes.byref(lc), d(wd), out)
            run_all(f"multi W={W} line x 9, {form}", lambda: Session("vrt_multi_lambda", create, pos.shape[0], 9, True, has_operator=False), modes)
            mp.close()


if args.multi:
    multi_sessions()
elif args.voronoi:
    voronoi_sessions()
else:
    raster_sessions()
