"""Reference of the Λ-iteration's "update + criterion" kernels: numpy and mpmath only, no device.

  update_model    the fp64 (and float-storage) update, operation for operation, with its scalar and third word
  min_den_model   what k_ali_min_den reduces
  update_mp       the same update in mpmath from the fp64 inputs (the ALI forms also as S_old + (S_fs - S_old) / den)
  forward_bound   a per-entry bound on |update_model - update_mp| from counting operations
  thread_map      which workgroup, wave, lane, grid-stride trip and unroll slot handles an entry
  seam_cases      the positions at which a planted extreme must be seen
  value_grid      the values at which the formulas change character, and classify() their classes
  MUTANTS         named wrong models of the reduction and the tail (update_model(..., mutant=name))

Arrays are in the caller's layout (n, ld) with nlam physical columns.  The ROW index is the kernel's own index: the
site for the row kernels (thread t = site * nlam + l), the up storage position for the sweep-order kernels (one thread
per position): a test that plants at a seam of a sweep-order kernel maps the position to its site first.
"""
from collections import namedtuple

import numpy as np

# ---- the launch constants, stated once, each with the kernel line it restates -----------------------------------------
THREADS = 256                   # hipLaunchKernelGGL(..., dim3(256), ...) and __launch_bounds__(256) of every update kernel
WAVE = 64                       # __shfl_xor(d, off, 64), wave = threadIdx.x >> 6, four LDS slots wmax[4]
MAX_WORKGROUPS = 256 * 16       # std::min<int64_t>((total + 255) / 256, 256 * 16) of every launch_*update*
UNROLL = {                      # pairs (float: units) in flight per trip of the wavelength loop
    "line": 4, "line_ali": 4,   # k_lambda_update_native:      constexpr int U = 4
    "continuum": 2, "continuum_ali": 2,     # k_continuum_update_native:   constexpr int U = 2
    "line_f32": 4,              # update_units_f32:            constexpr int U = 4, units of W = 2 pairs (a quad) or W = 1
}
SECOND_TRIP = THREADS * MAX_WORKGROUPS      # 2^20: the first entry (position) of the second grid-stride trip

KINDS = ("line", "line_ali", "line_f32", "continuum", "continuum_ali")
ALI = ("line_ali", "continuum_ali")
CONTINUUM = ("continuum", "continuum_ali")

# form "rows": one thread per entry, grid-stride (k_lambda_update, k_continuum_update, k_ali_min_den); "planes": one
# thread per up position walking the wavelength pairs (k_*_update_native*); pair_block: the float plan's pairs per block
Launch = namedtuple("Launch", "form U pair_block", defaults=(0, None))


def launch_of(kind, form, pair_block=None):
    if form == "rows":
        return Launch("rows")
    return Launch("planes", UNROLL[kind], pair_block if kind == "line_f32" else None)


def f32(a):
    """the float rounding of a float64 array, as float64"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- which thread handles an entry ----------------------------------------------------------------------------------------
def _unit_of_pair(q, npair, launch):
    """(trip of the unroll, slot in it, the trip is a tail -- it has clamped slots) of pair q"""
    U = launch.U
    if launch.pair_block is None:                               # double: units of one pair, U per trip
        trips = -(-npair // U)
        return q // U, q % U, (q // U == trips - 1) & (npair % U != 0)
    # float: the quads [0, 2 nquad) as units of two pairs, then one-pair units; each run has trips (and a tail) of its own
    nquad = npair >> 1 if launch.pair_block >= 2 else 0
    in_quads = q < 2 * nquad
    unit = np.where(in_quads, q // 2, q - 2 * nquad)
    units = np.where(in_quads, nquad, npair - 2 * nquad)
    first_trip = np.where(in_quads, 0, -(-nquad // U))         # (the trips of the single pairs come after the quads')
    trips = -(-units // U)
    return first_trip + unit // U, unit % U, (unit // U == trips - 1) & (units % U != 0)


def thread_map(n, nlam, launch):
    """per entry (row, l) of an (n, nlam) array, as int arrays of that shape: workgroup, wave, lane, trip (grid-stride),
    partial (its workgroup has idle threads in that trip), utrip, slot, tail (sweep-order forms: the unroll), pad_nb (the
    last physical wavelength of an odd nlam on planes: its pair's other half is the padding wavelength)"""
    row, l = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(nlam, dtype=np.int64), indexing="ij")
    if launch.form == "rows":
        t, total = row * nlam + l, n * nlam
    else:
        t, total = row, n
    blocks = max(min(-(-total // THREADS), MAX_WORKGROUPS), 1)
    stride = blocks * THREADS
    trip, r = t // stride, t % stride
    m = dict(workgroup=r // THREADS, wave=r % THREADS // WAVE, lane=r % WAVE, trip=trip,
             partial=(trip * stride + r // THREADS * THREADS + THREADS > total))
    zero = np.zeros_like(t)
    if launch.form == "rows":
        m.update(utrip=zero, slot=zero, tail=zero.astype(bool), pad_nb=zero.astype(bool))
    else:
        npair = (nlam + 1) // 2
        utrip, slot, tail = _unit_of_pair(l // 2, npair, launch)
        m.update(utrip=utrip + zero, slot=slot + zero, tail=tail | zero.astype(bool),
                 pad_nb=(l == nlam - 1) & bool(nlam & 1))
    return m


def clamped_slots(npair, launch):
    """pairs that a tail trip loads again for its slots past the end (the clamped index), with multiplicity: a list of
    pair numbers.  Double: slot u of the last trip reads pair npair - 1; float: the last unit of its run."""
    U, out = launch.U, []
    if launch.pair_block is None:
        if npair % U:
            out += [npair - 1] * (U - npair % U)
        return out
    nquad = npair >> 1 if launch.pair_block >= 2 else 0
    if nquad % U:
        out += [2 * nquad - 2, 2 * nquad - 1] * (U - nquad % U)
    singles = npair - 2 * nquad
    if singles % U:
        out += [npair - 1] * (U - singles % U)
    return out


# ---- the update, operation for operation ---------------------------------------------------------------------------------
def _entries(kind, J, B, e, S_old, L):
    """(S_new, num, den, plain, fallback) of every entry: separate multiplies and adds in the order of line_update_entry
    (vrt_kernels.hip), update_entry (vrt_continuum.hip) and update_units_f32.  num, den: None for the plain forms."""
    with np.errstate(all="ignore"):
        plain = (1.0 - e) * J + e * B
        if kind == "line_f32":
            return f32(plain), None, None, plain, np.zeros(plain.shape, bool)
        if kind not in ALI:
            return plain, None, None, plain, np.zeros(plain.shape, bool)
        t = 1.0 - e
        num = t * (J - L * S_old) + e * B
        den = np.broadcast_to(1.0 - t * L, num.shape)
        q = num / den
        if kind == "continuum_ali":                             # no fallback rule: whatever the quotient is
            return q, num, den, plain, np.zeros(plain.shape, bool)
        ok = den > 0.0
        return np.where(ok, q, plain), num, den, plain, ~ok


def _terms(S_old, S_new):
    with np.errstate(all="ignore"):
        return np.abs(1.0 - S_old / S_new)


def _scalar(terms):
    """NaN if any counted term is NaN, otherwise the maximum (0 over nothing: the kernels start from d = 0)"""
    if np.isnan(terms).any():
        return float("nan")
    return float(terms.max()) if terms.size else 0.0


Update = namedtuple("Update", "S_new scalar third parts")


def update_model(kind, J, B, eps, S_old, diag=None, eps_thick=None, nlam=None, J_down=None, launch=None, mutant=None,
                 previous_third=0, pad=None):
    """(S_new, scalar, third_word, parts) of one update call.

    kind            "line", "line_ali", "line_f32" (eps (n,), third word: None, the fallback count, None) or "continuum",
                    "continuum_ali" (eps (n, ld), third word: the thick count, eps > eps_thick)
    J, J_down       J, or J_up and J_down: the sweep-order kernels form J = J_up + J_down (float: rounded to float); either
                    may be None (the NULL pointer of a direction without angles)
    S_new           (n, ld) with the first nlam columns updated and the others NaN (what the device leaves untouched is
                    the caller's); float kind: the float values widened
    parts           dict(num, den, plain, term, fallback, seen, J): what a test that has to compare num and den apart needs
    launch, mutant  a Launch and a name of MUTANTS: a WRONG model, for the proof that the cases suffice
    previous_third  the third word of the call before (only the mutant stale_third_word reads it)
    pad             the (n,) values (J, B, S_old, Λ*, ε) of the padding wavelength as a dict; default zeros (only the mutant
                    pad_counted reads it)
    """
    assert kind in KINDS and (mutant is None or mutant in MUTANTS)
    B = np.asarray(B, dtype=np.float64)
    n, ld = B.shape
    nlam = ld if nlam is None else nlam
    with np.errstate(all="ignore"):
        Jv = np.zeros(B.shape) if J is None else np.asarray(J, dtype=np.float64)
        if J_down is not None:
            Jv = Jv + np.asarray(J_down, dtype=np.float64)
        if kind == "line_f32":
            Jv = f32(Jv)
    e = np.asarray(eps, dtype=np.float64)
    e = e if kind in CONTINUUM else e[:, None]
    S_old = np.asarray(S_old, dtype=np.float64)
    L = None if diag is None else np.asarray(diag, dtype=np.float64)
    assert (L is not None) == (kind in ALI)
    S_new, num, den, plain, fb = _entries(kind, Jv, B, e, S_old, L)
    term = _terms(S_old, S_new)
    seen = (e > eps_thick) & np.ones(B.shape, bool) if kind in CONTINUUM else np.ones(B.shape, bool)
    phys = np.zeros(B.shape, bool)
    phys[:, :nlam] = True
    S_out = np.where(phys, S_new, np.nan)
    parts = dict(num=num, den=den, plain=plain, term=np.where(phys, term, np.nan), fallback=fb & phys, seen=seen & phys, J=Jv)
    sl = (slice(None), slice(0, nlam))
    term, seen, fb = term[sl], seen[sl], fb[sl]

    # ---- the reduction (and, by name, its wrong models) ----
    extra_terms, extra_third = [], 0
    if mutant in ("drop_wave_3", "drop_partial_block", "drop_second_trip"):
        m = thread_map(n, nlam, launch)
        lost = {"drop_wave_3": m["wave"] == 3, "drop_partial_block": m["partial"], "drop_second_trip": m["trip"] >= 1}[mutant]
        seen, fb = seen & ~lost, fb & ~lost
    if mutant == "thin_seen":
        seen = np.ones(term.shape, bool)
    if mutant == "tail_repeats_last_pair" and launch.form == "planes":
        for q in clamped_slots((nlam + 1) // 2, launch):       # the clamped slot's pair is counted once more
            for l in (2 * q, 2 * q + 1):
                if l < nlam:
                    extra_terms.append(term[:, l][seen[:, l]])
                    extra_third += int((fb[:, l] if kind == "line_ali" else seen[:, l]).sum())
    if mutant == "pad_counted" and launch.form == "planes" and nlam & 1:
        p = dict(J=0.0, B=0.0, S_old=0.0, diag=0.0, eps=0.0)
        p.update(pad or {})
        z = lambda v: np.zeros(n) + v
        pe = z(p["eps"]) if kind in CONTINUUM else e[:, 0]
        pJ = f32(z(p["J"])) if kind == "line_f32" else z(p["J"])
        pS, _, _, _, pfb = _entries(kind, pJ, z(p["B"]), pe, z(p["S_old"]), z(p["diag"]))
        pseen = pe > eps_thick if kind in CONTINUUM else np.ones(n, bool)
        extra_terms.append(_terms(z(p["S_old"]), pS)[pseen])
        extra_third += int((pfb if kind == "line_ali" else pseen).sum())
    counted = np.concatenate([term[seen]] + extra_terms)
    if mutant == "nan_through_fmax":
        counted = counted[~np.isnan(counted)]
    if mutant == "inf_as_nan" and np.isinf(counted).any():
        counted = np.append(counted, np.nan)
    scalar = _scalar(counted)
    if kind == "line_ali":
        third = int(fb.sum()) + extra_third
        if mutant == "fallback_per_pair" and launch.form == "planes":
            npair = (nlam + 1) // 2
            padded = np.zeros((n, 2 * npair), bool)
            padded[:, :nlam] = fb
            third = int(padded.reshape(n, npair, 2).any(axis=2).sum())
    elif kind in CONTINUUM:
        third = int(seen.sum()) + extra_third
    else:
        third = None
    if mutant == "stale_third_word" and third is not None:
        third += int(previous_third)
    return Update(S_out, scalar, third, parts)


# name -> (the kinds it applies to, the forms it applies to, what is wrong)
_ALL, _COUNTING = KINDS, ("line_ali", "continuum", "continuum_ali")
MUTANTS = {
    "drop_wave_3": (_ALL, ("rows", "planes"), "lanes 192-255 of every workgroup are ignored"),
    "drop_partial_block": (_ALL, ("rows", "planes"), "a workgroup with idle threads is ignored"),
    "drop_second_trip": (("line", "line_ali", "continuum", "continuum_ali"), ("rows",), "the grid-stride loop runs once"),
    "tail_repeats_last_pair": (_COUNTING, ("planes",), "the clamped index of the unroll tail is counted"),
    "pad_counted": (_ALL, ("planes",), "the padding wavelength of an odd nlam enters the scalar and the counter"),
    "nan_through_fmax": (_ALL, ("rows", "planes"), "a NaN term is dropped, as fmax alone would"),
    "inf_as_nan": (_ALL, ("rows", "planes"), "an infinite term makes the scalar NaN"),
    "thin_seen": (CONTINUUM, ("rows", "planes"), "thin entries enter the scalar and the count"),
    "fallback_per_pair": (("line_ali",), ("planes",), "one count per wavelength pair with a fallback entry"),
    "stale_third_word": (_COUNTING, ("rows", "planes"), "the third word is not cleared between calls"),
}


def min_den_model(eps, diag):
    """(min over den > 0 of den = 1 - (1 - ε) Λ* -- +Inf over nothing --, any den not > 0): k_ali_min_den"""
    with np.errstate(all="ignore"):
        den = 1.0 - (1.0 - np.asarray(eps, dtype=np.float64)) * np.asarray(diag, dtype=np.float64)
    ok = den > 0.0
    return (float(den[ok].min()) if ok.any() else float("inf")), bool((~ok).any())


# ---- the same in mpmath, and the bound between the two -------------------------------------------------------------------
MP_DIGITS = 700                 # sums and products of doubles are exact at this width (2^-1074 ... 2^1024 is 2100 bits); only the divide rounds
U64, U32 = 2.0 ** -53, 2.0 ** -24
ETA64, ETA32 = 2.0 ** -1074, 2.0 ** -149        # one unit of the subnormal range: what an underflowing operation may lose


def _flat(kind, J, B, eps, S_old, diag):
    B = np.asarray(B, dtype=np.float64)
    e = np.asarray(eps, dtype=np.float64)
    e = np.broadcast_to(e if e.ndim == B.ndim else e[:, None], B.shape)
    L = np.zeros(B.shape) if diag is None else np.asarray(diag, dtype=np.float64)
    return [np.broadcast_to(np.asarray(a, dtype=np.float64), B.shape).ravel() for a in (J, B, e, S_old, L)], B.shape


_ctx = None


def _mp():
    """an mpmath context of MP_DIGITS digits of its own (the global one is left as it is)"""
    global _ctx
    if _ctx is None:
        import mpmath
        _ctx = mpmath.mp.clone()
        _ctx.dps = MP_DIGITS
    return _ctx


def _gamma(k, u=U64):
    return k * u / (1.0 - k * u)


def mp_reference(kind, J, B, eps, S_old, diag=None, want=("S", "alt", "bound")):
    """update_mp, its alt form and forward_bound in one pass over the entries: dict of arrays of the entries' shape (S, alt:
    objects -- mpf, or None where an input is not finite or the exact den is 0 --; bound: float64, Inf where there is none)"""
    ctx = _mp()
    mpf, one = ctx.mpf, ctx.mpf(1)
    (Jf, Bf, ef, Sf, Lf), shape = _flat(kind, J, B, eps, S_old, diag)
    finite = np.isfinite(Jf) & np.isfinite(Bf) & np.isfinite(ef) & np.isfinite(Sf) & np.isfinite(Lf)
    S, alt, bound = np.full(Jf.size, None, dtype=object), np.full(Jf.size, None, dtype=object), np.full(Jf.size, np.inf)
    g1, g2, g3, g4, g5 = (mpf(_gamma(k)) for k in (1, 2, 3, 4, 5))
    u64, u32, eta64, eta32 = mpf(U64), mpf(U32), mpf(ETA64), mpf(ETA32)
    w_alt, w_bound = "alt" in want, "bound" in want
    for i in np.flatnonzero(finite).tolist():
        j, b, e, s, l = mpf(Jf[i]), mpf(Bf[i]), mpf(ef[i]), mpf(Sf[i]), mpf(Lf[i])
        t = one - e
        tj, eb = t * j, e * b
        plain = tj + eb
        E_plain = g3 * abs(tj) + g2 * abs(eb) + 2 * eta64
        if kind == "line_f32":
            S[i] = alt[i] = plain
            before = E_plain + abs(t) * (1 + g3) * (u32 * abs(j) + eta32)
            bound[i] = float(before + u32 * (abs(plain) + before) + eta32)
            continue
        if kind not in ALI:
            S[i] = alt[i] = plain
            bound[i] = float(E_plain)
            continue
        tl = t * l
        den = one - tl
        if kind == "line_ali" and not den > 0:
            S[i] = alt[i] = plain
            if w_bound and -den > g1 + g3 * abs(tl) + eta64:
                bound[i] = float(E_plain)
            continue
        if den == 0:
            continue
        num = tj - tl * s + eb
        q = num / den
        S[i] = q
        if w_alt:
            alt[i] = s + (plain - s) / den
        if w_bound:
            E_n = g4 * abs(tj) + g5 * abs(tl * s) + g2 * abs(eb) + 3 * eta64
            E_d = g1 + g3 * abs(tl) + eta64
            if abs(den) > E_d:
                Q = (E_n * abs(den) + abs(num) * E_d) / (abs(den) * (abs(den) - E_d))
                bound[i] = float(Q + u64 * (abs(q) + Q) + eta64)
    return dict(S=S.reshape(shape), alt=alt.reshape(shape), bound=bound.reshape(shape))


def update_mp(kind, J, B, eps, S_old, diag=None, alt=False):
    """S_new of every entry in mpmath at MP_DIGITS digits from the fp64 inputs (float kind: J is the double J_up + J_down;
    nothing is rounded on the way), as an object array of mpf (None where an input is not finite or the exact den is 0).
    The line ALI takes the plain value where the EXACT den is not > 0.  alt: the ALI forms as S_old + (S_fs - S_old) / den,
    S_fs the plain value."""
    return mp_reference(kind, J, B, eps, S_old, diag, want=("alt",) if alt else ("S",))["alt" if alt else "S"]


def forward_bound(kind, J, B, eps, S_old, diag=None):
    """A per-entry bound on |update_model(...).S_new - update_mp(...)| (float64 array; Inf where the analysis gives none).

    Standard forward analysis: every operation returns its exact result times (1 + δ), |δ| <= u = 2^-53; a product of k such
    factors is (1 + θ_k) with |θ_k| <= γ_k = k u / (1 - k u); a multiply or divide that underflows adds at most η = 2^-1074
    absolutely (an add or subtract that lands in the subnormal range is exact).  With t = 1 - ε:

    plain   S = fl(fl(fl(1 - ε) J) + fl(ε B)).  The t J term carries the roundings of t, of the multiply and of the add
            (3), the ε B term those of its multiply and of the add (2), two multiplies may underflow:
                |Ŝ - S| <= γ_3 |t J| + γ_2 |ε B| + 2 η
    num     fl(fl(t̂ fl(J - fl(L s))) + fl(ε B)), t̂ = fl(1 - ε).  t J carries t̂, the subtract, the multiply, the add (4);
            t L s one more, the multiply L s (5); ε B two (2); three multiplies may underflow:
                E_n = γ_4 |t J| + γ_5 |t L s| + γ_2 |ε B| + 3 η
    den     fl(1 - fl(t̂ L)): the 1 carries the subtract (1), t L carries t̂, the multiply and the subtract (3); one multiply:
                E_d = γ_1 + γ_3 |t L| + η
    quot    q̂ = fl(n̂ / d̂).  n̂ / d̂ - n / d = ((n̂ - n) d - n (d̂ - d)) / (d d̂) and |d̂| >= |d| - E_d, so for E_d < |d|
                |n̂ / d̂ - n / d| <= Q = (E_n |d| + |n| E_d) / (|d| (|d| - E_d)),
                |q̂ - q| <= Q + u (|q| + Q) + η          (the divide's own rounding and underflow)
            and no bound (Inf) where E_d >= |d|: there the computed den may have either sign.  The line ALI is bounded by
            this where the exact den is > E_d (both take the quotient), by the plain bound where it is < -E_d.
    float   The header's two float roundings.  J here is the double sum J_up + J_down as the kernel forms it, and update_mp
            is fed that J UNROUNDED; the kernel rounds it to float: E_J = u32 |J| + η32 (u32 = 2^-24, η32 = 2^-149 where the
            float underflows), which enters S through t (1 + γ_3) E_J; the final rounding of S to float adds
            u32 (|S| + everything before) + η32.

    Every magnitude on the right is evaluated in mpmath from the inputs, never from a run of the model."""
    return mp_reference(kind, J, B, eps, S_old, diag, want=("bound",))["bound"]


# ---- the seams ---------------------------------------------------------------------------------------------------------------
def _thread_seams(total):
    """thread indices at the launch seams of `total` threads' worth of work, name -> index: the first and the last entry,
    and, in the first and the last workgroup of every grid-stride trip, both sides of every wave edge and of the workgroup's
    own edges (the last workgroup is the partial one when there is one: its last lane is the last entry of the trip)"""
    s = {"first": 0}
    blocks = max(min(-(-total // THREADS), MAX_WORKGROUPS), 1)
    stride = blocks * THREADS
    for trip in range(-(-total // stride)):
        end = min((trip + 1) * stride, total)                   # (one past the trip's last entry)
        for which, base in (("first", trip * stride), ("next", trip * stride + THREADS),
                            ("last", (end - 1) // THREADS * THREADS)):
            for w in range(THREADS // WAVE):
                lo, hi = base + w * WAVE, min(base + (w + 1) * WAVE, end) - 1
                if lo < end and not (which == "next" and w):    # (of the second workgroup only its first lane: the edge)
                    s.setdefault(f"trip{trip}_{which}_workgroup_wave{w}_first_lane", lo)
                    if which != "next":
                        s.setdefault(f"trip{trip}_{which}_workgroup_wave{w}_last_lane", hi)
    s["last"] = total - 1
    seen, out = set(), {}
    for k, v in s.items():
        if 0 <= v < total and v not in seen:
            seen.add(v)
            out[k] = v
    return out


def _unroll_wavelengths(nlam, launch):
    """name -> wavelength: both halves of the first and last pair of every trip of the unroll (its tail included), and the
    last physical wavelength"""
    npair = (nlam + 1) // 2
    q = np.arange(npair)
    utrip, slot, tail = (np.broadcast_to(a, q.shape) for a in _unit_of_pair(q, npair, launch))
    out = {}
    for k in np.unique(utrip):
        pairs = q[utrip == k]
        name = f"{'tail' if tail[pairs[0]] else 'trip'}{k}"
        for which, p in (("first_pair", pairs[0]), ("last_pair", pairs[-1])):
            for half in (0, 1):
                if 2 * p + half < nlam:
                    out[f"{name}_{which}_{'xy'[half]}"] = int(2 * p + half)
    out["last_physical" + ("_next_to_pad" if nlam & 1 else "")] = nlam - 1
    return out


def seam_cases(n, nlam, launch, every_slot=True):
    """[(name, row, l)]: where a planted extreme must be seen, from the launch constants above.  Rows form: the thread
    seams of the n nlam entries (with the second grid-stride trip when there is one).  Sweep-order forms: the thread seams
    of the n positions at every wavelength (every_slot: every unroll slot at every lane seam; otherwise only at the
    wavelengths of _unroll_wavelengths)."""
    cases = []
    if launch.form == "rows":
        for name, t in _thread_seams(n * nlam).items():
            cases.append((name, t // nlam, t % nlam))
        return cases
    special = _unroll_wavelengths(nlam, launch)
    label = {}
    for name, l in special.items():
        label.setdefault(l, name)
    for name, pos in _thread_seams(n).items():
        for l in (range(nlam) if every_slot else sorted(label)):
            cases.append((f"{name}/{label.get(l, f'lam{l}')}", pos, l))
    return cases


# ---- the values at which the formulas change character ------------------------------------------------------------------
TINY = 2.0 ** -1074
EPS_VALUES = (0.0, TINY, 1e-300, 1e-7, 0.5, 1.0 - 2.0 ** -53, 1.0)
LSTAR_VALUES = (0.0, TINY, 0.5, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 2.0)
FIELD_VALUES = (0.0, TINY, 1e-300, 1.0, 1e300, np.inf, np.nan)
# float kind (its inputs ARE floats): the smallest float subnormal, a larger subnormal, the largest float -- J_up + J_down of
# two of those overflows as a float and not as a double; ε B of a subnormal B underflows as a float and not as a double
FIELD_VALUES_F32 = (0.0, 2.0 ** -149, float(np.float32(1e-40)), 1.0, float(np.finfo(np.float32).max), np.inf, np.nan)
CLASSES = ("thin", "nan", "fallback", "den_zero", "inf_term", "ordinary")
VALUE_EPS_THICK = 1e-4


def value_grid(kind):
    """dict(J, B, S_old, diag, eps): the edge set as one small array.  Rows are the (ε, Λ*) combinations -- ε is per site
    in the line kinds --, columns the (J, B, S_old) combinations; eps is (rows,) for the line kinds, (rows, columns) for
    the continuum; diag is None for the plain kinds (their rows are the ε values alone)."""
    F = FIELD_VALUES_F32 if kind == "line_f32" else FIELD_VALUES
    rows = [(e, l) for e in EPS_VALUES for l in (LSTAR_VALUES if kind in ALI else (0.0,))]
    cols = [(j, b, s) for j in F for b in F for s in F]
    col = lambda k: np.broadcast_to(np.array([c[k] for c in cols]), (len(rows), len(cols))).copy()
    e = np.array([r[0] for r in rows])
    g = dict(J=col(0), B=col(1), S_old=col(2), diag=None, eps=e)
    if kind in ALI:
        g["diag"] = np.broadcast_to(np.array([r[1] for r in rows])[:, None], g["J"].shape).copy()
    if kind in CONTINUUM:
        g["eps"] = np.broadcast_to(e[:, None], g["J"].shape).copy()
    return g


def classify(kind, upd):
    """the class of every entry of an Update, as an array of indices into CLASSES (every entry has exactly one: the
    first of CLASSES whose rule holds)

      thin       continuum: ε not > eps_thick -- written, invisible to the scalar and the count
      nan        the criterion's term is NaN (0/0 in the quotient or in S_old / S_new, a NaN input, Inf - Inf)
      fallback   line ALI: den not > 0, the plain value taken and counted
      den_zero   continuum ALI: den = 0 under a nonzero num, S_new = ±Inf
      inf_term   the term is +Inf and not NaN: S_new = 0 under S_old != 0, or a quotient past the largest double
      ordinary   everything else: a finite term
    """
    p = upd.parts
    term = p["term"]
    out = np.full(term.shape, CLASSES.index("ordinary"))
    out[np.isinf(term)] = CLASSES.index("inf_term")
    if kind == "continuum_ali":
        out[(p["den"] == 0.0) & np.isinf(upd.S_new)] = CLASSES.index("den_zero")
    if kind == "line_ali":
        out[p["fallback"]] = CLASSES.index("fallback")
    out[np.isnan(term)] = CLASSES.index("nan")
    if kind in CONTINUUM:
        out[~p["seen"]] = CLASSES.index("thin")
    return out


def class_case(kind, g, filler, mask):
    """the value grid with every entry outside `mask` replaced by the benign filler's (ε is per row in the line kinds and
    stays the grid's: the filler's J, B, S_old and Λ* are benign under every ε of the grid but the ALI rows whose den is
    not > 0 or tiny -- the model says what those give)"""
    c = dict(g)
    for key in ("J", "B", "S_old", "diag"):
        if g[key] is not None:
            c[key] = np.where(mask, g[key], filler[key])
    if kind in CONTINUUM:
        c["eps"] = np.where(mask, g["eps"], filler["eps"])
    return c


# ---- the benign case and what is planted into it -----------------------------------------------------------------------
BENIGN_BOUND, PLANT_FLOOR = 0.1, 0.3            # every term of benign_case is below the first, a planted term above the second
ONLY_THICK = 0.5                                # eps_thick of plant "only_thick": benign ε stays below it


def benign_case(kind, n, nlam, seed=0):
    """dict(J, B, S_old, diag, eps, eps_thick) whose criterion terms are all below BENIGN_BOUND: j0, B, S_old in [1, 1.05],
    Λ* in [0, 0.05] and J = j0 + Λ* S_old, so num = (1 - ε) j0 + ε B in [1, 1.05], den in [0.95, 1], S_new in [1, 1.106] and
    |1 - S_old / S_new| <= 0.096; ε in [1e-3, 0.3], per site in the line kinds; the float kind: float values"""
    rng = np.random.default_rng(seed)
    j0, B, S_old = (1.0 + 0.05 * rng.random((n, nlam)) for _ in range(3))
    eps = 10.0 ** rng.uniform(-3.0, np.log10(0.3), (n, nlam) if kind in CONTINUUM else n)
    diag = 0.05 * rng.random((n, nlam)) if kind in ALI else None
    J = j0 + diag * S_old if kind in ALI else j0
    if kind == "line_f32":
        J, B, S_old = f32(J), f32(B), f32(S_old)
    return dict(J=J, B=B, S_old=S_old, diag=diag, eps=eps, eps_thick=1e-4 if kind in CONTINUUM else None)


PLANTS = ("term", "nan", "inf", "fallback", "fallback_site", "only_thick")


def plant(kind, case, what, row, l):
    """a copy of `case` with one entry changed, and what the call must then return: (case, scalar, third, where S_new is
    NaN).  The scalar is the planted entry's own term, formed from that entry alone; third is None where the kind has none.

      term           S_old × 1.5 there: a term in [PLANT_FLOOR, 0.7], the largest
      nan            B = NaN there: the scalar is NaN and S_new is NaN there only
      inf            J = B = Λ* = 0 there: S_new = 0 under S_old != 0, a term of +Inf that is no NaN
      fallback       line ALI: ε = 0 at the row and Λ* = 1 there: the plain value, counted once
      fallback_site  line ALI: ε = 0 at the row and Λ* = 1 at all its wavelengths: counted nlam times (both halves of a pair)
      only_thick     continuum: eps_thick = ONLY_THICK, ε = 0.9 and S_old × 1.5 there -- the only thick entry --, and
                     S_old × 3 at a thin neighbour (a larger term that must stay unseen)
    """
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    n, nlam = c["B"].shape
    at = (row, l)
    if what in ("term", "only_thick"):
        c["S_old"][at] = c["S_old"][at] * 1.5
    if what == "nan":
        c["B"][at] = np.nan
    if what == "inf":
        c["J"][at] = c["B"][at] = 0.0
        if kind in ALI:
            c["diag"][at] = 0.0
    if what in ("fallback", "fallback_site"):
        assert kind == "line_ali"
        c["eps"][row] = 0.0
        c["diag"][row, slice(None) if what == "fallback_site" else l] = 1.0
    if what == "only_thick":
        assert kind in CONTINUUM
        c["eps_thick"] = ONLY_THICK
        c["eps"][at] = 0.9
        other = ((row + 1) % n, l) if n > 1 else (row, (l + 1) % nlam)
        if other != at:
            c["S_old"][other] = c["S_old"][other] * 3.0
    if kind == "line_f32":                                      # (the float kind's inputs are floats)
        for key in ("J", "B", "S_old"):
            c[key] = f32(c[key])
    # the planted entry alone, as a 1 x 1 call
    one = lambda a: None if a is None else a[row:row + 1, l:l + 1]
    e1 = c["eps"][row:row + 1, l:l + 1] if kind in CONTINUUM else c["eps"][row:row + 1]
    u = update_model(kind, one(c["J"]), one(c["B"]), e1, one(c["S_old"]), diag=one(c["diag"]), eps_thick=c["eps_thick"])
    scalar = u.scalar
    third = None
    if kind == "line_ali":
        third = {"fallback": 1, "fallback_site": nlam}.get(what, 0)
    if kind in CONTINUUM:
        third = 1 if what == "only_thick" else n * nlam
    if what in ("fallback", "fallback_site"):
        scalar = None                                           # (the other entries of the row changed too: not stated here)
    return c, scalar, third, (at if what == "nan" else None)


def run_case(kind, c, nlam=None, **kw):
    """update_model on a case dict"""
    return update_model(kind, c["J"], c["B"], c["eps"], c["S_old"], diag=c["diag"], eps_thick=c["eps_thick"], nlam=nlam, **kw)
