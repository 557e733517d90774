"""Host-side mirror of the reference's interface for the formal-solve path, over the C ABI.

Same names and argument meaning as the Julia originals so that tests read like the reference's
drivers:

  read_quadrature      src/functions.jl:33-63
  VoronoiSites         src/voronoi_utils.jl:7-28      (ray-tracing fields; grid lives on the GPU)
  read_cell            src/voronoi_utils.jl:36-85
  Delaunay_upII        src/irregular_ray_tracing.jl:15-82
  Delaunay_downII      src/irregular_ray_tracing.jl:96-163
  J_lambda_voronoi     src/lambda_iteration.jl:60-113 / src/lambda_continuum.jl:27-56 (J_λ_voronoi)
  Lambda_voronoi       src/lambda_iteration.jl:205-300 (Λ_voronoi; device-resident loop)

Arrays are numpy with the reference's memory layout (see voronoirt_amd/synth.py): positions
(n, 3) [z, x, y], neighbours (D+1, n) with 1-based ids, S / alpha / J (n, nlam) wavelength
fastest.  Nothing here computes intensities on the CPU: every call goes through libvrt_hip.so
and raises `VrtError` when no HIP device is present.
"""
from __future__ import annotations

import ctypes
import os
import re
import weakref

import numpy as np

from . import _lib
from ._lib import VrtError, check

QUADRATURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "quadratures")


def _d(a):
    return a.ctypes.data_as(_lib.p_dbl) if a is not None else None


def _i(a):
    return a.ctypes.data_as(_lib.p_i64) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def read_quadrature(fname: str):
    """weights, θ (deg), ϕ (deg), n_points -- src/functions.jl:33-63.

    The reference derives the point count from the digits after the first 'n' of the PATH
    (functions.jl:36-48), which breaks on directories containing an 'n'; here the rule is applied
    to the file's base name, and a count that disagrees with the file is an error (the reference
    would raise BoundsError or silently keep zero weights)."""
    path = fname
    if not os.path.exists(path):
        cand = os.path.join(QUADRATURE_DIR, os.path.basename(fname))
        if os.path.exists(cand):
            path = cand
    base = os.path.basename(path)
    m = re.search(r"n(\d+)", base)
    if not m:
        raise ValueError(f"cannot derive the number of quadrature points from {base!r}")
    n_points = int(m.group(1))
    rows = [ln.split() for ln in open(path) if ln.strip()]
    if len(rows) != n_points:
        raise ValueError(f"{base}: name says {n_points} points, file has {len(rows)}")
    arr = np.array([[float(v) for v in r[:3]] for r in rows])
    return arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy(), n_points


def direction(theta_deg: float, phi_deg: float) -> np.ndarray:
    """k = [cos θ, cos ϕ sin θ, sin ϕ sin θ] -- src/lambda_iteration.jl:87"""
    k = np.zeros(3)
    _lib.load().vrt_direction(float(theta_deg), float(phi_deg), _d(k))
    return k


class VoronoiSites:
    """The reference's `VoronoiSites` (src/voronoi_utils.jl:7-28) backed by a device-resident
    grid handle (`vrt_grid`).  `device=-1` builds a host-only handle (layers / permutations /
    schedule introspection, no compute)."""

    def __init__(self, positions, neighbours, bounds, device: int = 0, _from_file: str | None = None):
        L = _lib.load()
        self.positions = _f64(positions)
        if self.positions.ndim != 2 or self.positions.shape[1] != 3:
            raise ValueError("positions must have shape (n, 3) with columns (z, x, y)")
        self.n = self.positions.shape[0]
        self.bounds = tuple(float(b) for b in bounds)
        self.z_min, self.z_max, self.x_min, self.x_max, self.y_min, self.y_max = self.bounds
        self.device = device
        b = np.array(self.bounds, dtype=np.float64)
        h = ctypes.c_void_p()
        if _from_file is not None:
            check(L.vrt_grid_create_from_file(_from_file.encode(), self.n, _d(self.positions),
                                              _d(b), device, ctypes.byref(h)))
            self.neighbours = None
        else:
            self.neighbours = np.ascontiguousarray(neighbours, dtype=np.int64)
            if self.neighbours.ndim != 2 or self.neighbours.shape[1] != self.n:
                raise ValueError("neighbours must have shape (D+1, n)")
            check(L.vrt_grid_create(self.n, _d(self.positions), _i(self.neighbours),
                                    self.neighbours.shape[0], _d(b), device, ctypes.byref(h)))
        self._h = h
        self.max_neighbours = int(L.vrt_grid_max_neighbours(h))
        self.layers_up = self._layers(+1)
        self.layers_down = self._layers(-1)
        self.perm_up = self._perm(+1)
        self.perm_down = self._perm(-1)
        self._plans = {}
        self._live_plans = weakref.WeakSet()    # every FormalPlan built on this grid (closed with it)
        self._options = {}                      # tuning options set on this grid (set_option)

    # -- introspection ------------------------------------------------------------------------
    def _layers(self, d):
        L = _lib.load()
        out = np.zeros(int(L.vrt_grid_num_layer_offsets(self._h, d)), dtype=np.int64)
        check(L.vrt_grid_get_layers(self._h, d, _i(out)))
        return out

    def _perm(self, d):
        out = np.zeros(self.n, dtype=np.int64)
        check(_lib.load().vrt_grid_get_perm(self._h, d, _i(out)))
        return out

    def set_option(self, name: str, value) -> None:
        """Tuning option (`vrt_grid_set_option` / `vrt_plan_set_option`, e.g. VRT_PATH = auto | levels | tiles |
        steps | patches) for every plan of this grid: the single-solve plans cached inside the handle, the
        live FormalPlans and those created later.  Environment variables of the same names are read once, at
        plan creation."""
        check(_lib.load().vrt_grid_set_option(self._h, name.encode(), str(value).encode()))
        self._options[name] = str(value)
        for p in list(self._live_plans):
            try:
                p.set_option(name, value)
            except VrtError:
                pass          # an option that shapes what plan creation builds: it holds for the plans created from now on

    def storage_order(self, d: int) -> np.ndarray:
        """1-based site id at every storage position of direction d (> 0 up, < 0 down): the site
        order of the library's native layouts (VRT_ALPHA_ANGLE_NATIVE)."""
        out = np.zeros(self.n, dtype=np.int64)
        check(_lib.load().vrt_grid_get_storage_order(self._h, d, _i(out)))
        return out

    @property
    def Delaunay_lines(self) -> np.ndarray:
        """(n, D, 3) == Julia (3, D, n); computed on the device at construction."""
        out = np.zeros((self.n, self.max_neighbours, 3))
        check(_lib.load().vrt_grid_get_delaunay_lines(self._h, _d(out)))
        return out

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            # a plan holds a pointer to the grid: close every plan still alive before the grid goes,
            # also those the caller created (a later plan.close() is then a no-op)
            for p in list(self._live_plans):
                p.close()
            self._plans = {}
            _lib.load().vrt_grid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _device_ordinal(device) -> int:
    """A device ordinal given as an int (bool and everything else: ValueError), checked before the library is loaded."""
    if isinstance(device, bool) or not isinstance(device, (int, np.integer)):
        raise ValueError(f"device must be None (host) or a device ordinal, not {device!r}")
    return int(device)


def voro(positions, bounds, neighbours_file: str | None = None, max_guess: int = 70, device=None) -> np.ndarray:
    """The reference's `voro` step (src/functions.jl:13-23: run the voro++ wrapper on the sites file)
    in-process: Voronoi neighbours of `positions` (n, 3) [z, x, y] in `bounds` = (z_min, z_max,
    x_min, x_max, y_min, y_max), periodic in x and y, walls -5 / -6 in z.  Returns the (D+1, n)
    matrix `read_cell` builds; with `neighbours_file` also writes the voro++ "%i %n" text file.
    device=None: host code (no GPU needed).  device=<ordinal>: the same matrix from the device
    tessellation (`vrt_tessellate_gpu`; sites it cannot hold are recomputed by the host code)."""
    dev = None if device is None else _device_ordinal(device)
    L = _lib.load()
    pos = _f64(positions)
    n = pos.shape[0]
    b = np.array([float(v) for v in bounds], dtype=np.float64)
    M = np.zeros((max_guess + 1, n), dtype=np.int64)
    mx = ctypes.c_int64()
    if dev is None:
        check(L.vrt_tessellate(n, _d(pos), _d(b), max_guess + 1, _i(M), ctypes.byref(mx)))
    else:
        check(L.vrt_tessellate_gpu(dev, n, _d(pos), _d(b), max_guess + 1, _i(M), ctypes.byref(mx), None))
    if neighbours_file is not None:
        check(L.vrt_write_neighbours_file(neighbours_file.encode(), n, _i(M), max_guess + 1))
    return np.ascontiguousarray(M[: mx.value + 1])


def voro_dev(pos_tensor, bounds, max_guess: int = 70):
    """`voro` on positions that are on the device already (`vrt_tessellate_dev`): pos_tensor is a contiguous float64
    torch tensor (n, 3) [z, x, y] on a GPU, e.g. what rejection_sampling_dev filled.  Returns (M, host_sites): M the
    (max_guess + 1, n) int64 matrix on that device (row 0 the counts, zeros beyond a site's count), host_sites the
    sites the host code had to recompute.  Runs on torch's current stream of that device and synchronises it."""
    import torch

    if not isinstance(pos_tensor, torch.Tensor) or pos_tensor.dtype != torch.float64:
        raise ValueError("pos_tensor must be a float64 torch tensor")
    if pos_tensor.dim() != 2 or pos_tensor.shape[1] != 3 or not pos_tensor.is_contiguous():
        raise ValueError("pos_tensor must be contiguous with shape (n, 3)")
    if pos_tensor.device.type != "cuda":
        raise ValueError("pos_tensor must be on a GPU")
    L = _lib.load()
    dev = pos_tensor.device
    n = pos_tensor.shape[0]
    b = np.array([float(v) for v in bounds], dtype=np.float64)
    M = torch.empty((max_guess + 1, n), dtype=torch.int64, device=dev)
    mx, hs = ctypes.c_int64(), ctypes.c_int64()
    check(L.vrt_tessellate_dev(dev.index or 0, n, pos_tensor.data_ptr(), _d(b), max_guess + 1, M.data_ptr(), ctypes.byref(mx),
                               ctypes.byref(hs), torch.cuda.current_stream(dev).cuda_stream or None))
    return M, hs.value


def read_cell(fname: str, n_sites: int, positions, bounds, device: int = 0) -> VoronoiSites:
    """read_cell (src/voronoi_utils.jl:36-85): parse the voro++ "%i %n" neighbour file, layer the
    grid from both walls, sort, and compute the Delaunay lines.  `bounds` =
    (z_min, z_max, x_min, x_max, y_min, y_max)."""
    pos = _f64(positions)
    if pos.shape[0] != n_sites:
        raise ValueError("positions does not have n_sites rows")
    return VoronoiSites(pos, None, bounds, device=device, _from_file=fname)


class FormalPlan:
    """Upwind tables + sweep schedule for a set of directions on one grid (`vrt_plan`)."""

    def __init__(self, sites: VoronoiSites, k, n_sweeps: int = 3, dirs=None):
        L = _lib.load()
        self.sites = sites
        self.k = _f64(np.atleast_2d(k))
        if self.k.shape[1] != 3:
            raise ValueError("k must have shape (n_angles, 3)")
        self.n_angles = self.k.shape[0]
        self.n_sweeps = int(n_sweeps)
        h = ctypes.c_void_p()
        if dirs is None:
            check(L.vrt_plan_create(sites.handle, self.n_angles, _d(self.k), self.n_sweeps,
                                    ctypes.byref(h)))
        else:
            d = np.ascontiguousarray(dirs, dtype=np.int32)
            check(L.vrt_plan_create_ex(sites.handle, self.n_angles, _d(self.k),
                                       d.ctypes.data_as(_lib.p_int), self.n_sweeps, ctypes.byref(h)))
        self._h = h
        sites._live_plans.add(self)
        for name, value in sites._options.items():      # options set on the grid follow into its plans
            try:
                self.set_option(name, value)
            except VrtError:
                pass                                     # a creation-only option: the environment presets those

    @property
    def num_levels(self) -> int:
        return int(_lib.load().vrt_plan_num_levels(self._h))

    @property
    def num_nodes(self) -> int:
        return int(_lib.load().vrt_plan_num_nodes(self._h))

    def upwind(self, angle: int):
        """(up (n,2) 1-based ids, dots (n,2), weights (n,2), path lengths (n,2))"""
        n = self.sites.n
        up = np.zeros((n, 2), dtype=np.int64)
        dots = np.zeros((n, 2))
        w = np.zeros((n, 2))
        r = np.zeros((n, 2))
        check(_lib.load().vrt_plan_get_upwind(self._h, angle, _i(up), _d(dots), _d(w), _d(r)))
        return up, dots, w, r

    def execute(self, S, alpha, weights=None, I0_up=None, I0_down=None, want_J=True,
                want_I=False, alpha_mode=None):
        """Host arrays in, host arrays out.  S (n, nlam); alpha (n,), (n, nlam) or
        (n_angles, n, nlam).  Returns (J or None, I or None) with I of shape
        (n_angles, n, nlam)."""
        S = _f64(S)
        if S.ndim == 1:
            S = S.reshape(-1, 1)
        n, nlam = S.shape
        if n != self.sites.n:
            raise ValueError("S has the wrong number of sites")
        alpha = _f64(alpha)
        if alpha_mode is None:
            alpha_mode = {1: _lib.ALPHA_SITE, 2: _lib.ALPHA_SITE_LAM,
                          3: _lib.ALPHA_ANGLE_SITE_LAM}[alpha.ndim]
        want = {_lib.ALPHA_SITE: n, _lib.ALPHA_SITE_LAM: n * nlam,
                _lib.ALPHA_ANGLE_SITE_LAM: self.n_angles * n * nlam}[alpha_mode]
        if alpha.size != want:
            raise ValueError("alpha has the wrong size for its mode")
        n1u = int(self.sites.layers_up[1] - 1)
        n1d = int(self.sites.layers_down[1] - 1)
        if I0_up is not None:
            I0_up = _f64(I0_up).reshape(-1, nlam)
            if I0_up.shape[0] != n1u:
                raise ValueError(f"I0_up has {I0_up.shape[0]} rows, bottom layer has {n1u} sites")
        if I0_down is not None:
            I0_down = _f64(I0_down).reshape(-1, nlam)
            if I0_down.shape[0] != n1d:
                raise ValueError(f"I0_down has {I0_down.shape[0]} rows, top layer has {n1d} sites")
        w = _f64(weights) if weights is not None else np.ones(self.n_angles)
        if w.size != self.n_angles:
            raise ValueError("weights has the wrong length")
        J = np.zeros((n, nlam)) if want_J else None
        Iout = np.zeros((self.n_angles, n, nlam)) if want_I else None
        check(_lib.load().vrt_plan_execute(self._h, nlam, nlam, _d(S), _d(alpha), alpha_mode,
                                           _d(I0_up), _d(I0_down), _d(w), _d(J), _d(Iout)))
        return J, Iout

    def execute_dev(self, nlam: int, ld: int, dS: int, dalpha: int, alpha_mode: int, weights,
                    dJ: int = 0, dI0_up: int = 0, dI0_down: int = 0, dI_out: int = 0,
                    stream: int = 0, f32: bool = False) -> None:
        """Device pointers (ints, e.g. torch.Tensor.data_ptr()) and a hipStream_t handle
        (torch.cuda.current_stream().cuda_stream).  Asynchronous on `stream`.  f32=True: the
        buffers hold float32 values (fp32 value path, arithmetic stays fp64)."""
        w = _f64(weights)
        fn = _lib.load().vrt_plan_execute_dev_f32 if f32 else _lib.load().vrt_plan_execute_dev
        check(fn(self._h, nlam, ld, dS, dalpha, alpha_mode, dI0_up or None, dI0_down or None, _d(w),
                 dJ or None, dI_out or None, stream or None))

    # ---- S and J in sweep order (include/voronoirt.h: vrt_plan_execute_native_dev) ----
    def native_plane_count(self, nlam: int) -> int:
        """values (float64, or float32 with the f32 entry points) of ONE direction's sweep-order plane set of S or J."""
        return int(_lib.load().vrt_plan_native_plane_count(self._h, nlam))

    def to_native_dev(self, nlam: int, ld: int, d_in: int, d_up: int = 0, d_down: int = 0, stream: int = 0, f32: bool = False) -> None:
        """Device (n, ld) array -> the sweep-order plane sets of both directions (either may be 0)."""
        fn = _lib.load().vrt_plan_to_native_dev_f32 if f32 else _lib.load().vrt_plan_to_native_dev
        check(fn(self._h, nlam, ld, d_in, d_up or None, d_down or None, stream or None))

    def from_native_dev(self, d: int, nlam: int, ld: int, d_native: int, d_out: int, stream: int = 0, f32: bool = False) -> None:
        """The sweep-order plane set of direction d (> 0: up) -> a device (n, ld) array."""
        fn = _lib.load().vrt_plan_from_native_dev_f32 if f32 else _lib.load().vrt_plan_from_native_dev
        check(fn(self._h, int(d), nlam, ld, d_native, d_out, stream or None))

    def J_from_native_dev(self, nlam: int, ld: int, dJ_up: int, dJ_down: int, dJ: int, stream: int = 0, f32: bool = False) -> None:
        """J = J_up + J_down in the caller's (n, ld) layout."""
        fn = _lib.load().vrt_plan_j_from_native_dev_f32 if f32 else _lib.load().vrt_plan_j_from_native_dev
        check(fn(self._h, nlam, ld, dJ_up or None, dJ_down or None, dJ, stream or None))

    def execute_native_dev(self, nlam: int, dS_up: int, dS_down: int, dalpha: int, alpha_mode: int, weights,
                           dJ_up: int = 0, dJ_down: int = 0, dI0_up: int = 0, dI0_down: int = 0, stream: int = 0,
                           f32: bool = False) -> None:
        """`execute_dev` with S read from and J reduced into sweep-order plane sets, in place (no layout change)."""
        w = _f64(weights)
        fn = _lib.load().vrt_plan_execute_native_dev_f32 if f32 else _lib.load().vrt_plan_execute_native_dev
        check(fn(self._h, nlam, dS_up or None, dS_down or None, dalpha, alpha_mode, dI0_up or None, dI0_down or None, _d(w),
                 dJ_up or None, dJ_down or None, stream or None))

    def check(self) -> None:
        """Raises if a chained launch of an earlier ASYNCHRONOUS execute gave up (call after synchronising)."""
        check(_lib.load().vrt_plan_check(self._h))

    def native_alpha_count(self, nlam: int) -> int:
        """Number of float64 values of the native per-angle alpha buffer (ALPHA_ANGLE_NATIVE)."""
        return int(_lib.load().vrt_plan_native_alpha_count(self._h, nlam))

    @property
    def native_pair_block(self) -> int:
        """Wavelength pairs of a site kept side by side in the native layout (include/voronoirt.h)."""
        return int(_lib.load().vrt_plan_native_pair_block(self._h))

    @property
    def native_pair_block_f32(self) -> int:
        """The same for the float native buffer (fp32 value path)."""
        return int(_lib.load().vrt_plan_native_pair_block_f32(self._h))

    def native_to_site_major(self, native, nlam: int, n_angles: int):
        """Host helper (tests, debugging): a native per-angle buffer (numpy float64 or float32) ->
        (n_angles, n, nlam) with rows in STORAGE order of each angle's direction."""
        native = np.asarray(native)
        n = self.sites.n
        B = self.native_pair_block_f32 if native.dtype == np.float32 else self.native_pair_block
        npair = (nlam + 1) // 2
        per = native.reshape(n_angles, npair * n * 2)
        out = np.empty((n_angles, n, 2 * npair), dtype=native.dtype)
        q0 = 0
        widths = [B] * (npair // B) + [1 << b for b in range(B.bit_length() - 2, -1, -1) if (npair % B) & (1 << b)]
        for w in widths:
            blk = per[:, q0 * n * 2:(q0 + w) * n * 2].reshape(n_angles, n, 2 * w)
            out[:, :, 2 * q0:2 * (q0 + w)] = blk
            q0 += w
        return out[:, :, :nlam]

    def alpha_to_native_dev(self, nlam: int, ld: int, dalpha: int, dalpha_native: int, stream: int = 0,
                            f32: bool = False) -> None:
        """Device (n_angles, n, ld) per-angle alpha -> the native layout, once per change of alpha
        (f32: float32 buffers, for execute_dev(..., f32=True))."""
        fn = _lib.load().vrt_plan_alpha_to_native_dev_f32 if f32 else _lib.load().vrt_plan_alpha_to_native_dev
        check(fn(self._h, nlam, ld, dalpha, dalpha_native, stream or None))

    def line_opacity_dev(self, lam, lambda0: float, c0: float, d_velocity: int, d_doppler: int, d_gamma: int,
                         d_line_strength: int, d_alpha_cont: int, d_alpha_native: int, stream: int = 0,
                         f32: bool = False) -> None:
        """Fused opacity prologue (`vrt_line_opacity_dev[_f32]`): α_tot of every angle of this plan from
        per-site line parameters (device pointers, float64), written in the native layout (f32: stored as
        float32 for execute_dev(..., f32=True))."""
        lam = _f64(lam)
        fn = _lib.load().vrt_line_opacity_dev_f32 if f32 else _lib.load().vrt_line_opacity_dev
        check(fn(self._h, lam.size, _d(lam), float(lambda0), float(c0), d_velocity, d_doppler, d_gamma, d_line_strength,
                 d_alpha_cont, d_alpha_native, stream or None))

    def line_lambda_diagonal_dev(self, nlam: int, d_alpha_native: int, weights, ld: int, d_diag: int, stream: int = 0) -> None:
        """Λ* of the line Λ-iteration (`vrt_line_lambda_diagonal_dev`) from this plan's native per-angle α (what
        `line_opacity_dev` or `alpha_to_native_dev` wrote) into d_diag, (n, ld) rows; asynchronous on `stream`."""
        check(_lib.load().vrt_line_lambda_diagonal_dev(self._h, nlam, d_alpha_native, _d(_f64(weights)), ld, d_diag,
                                                       stream or None))

    def set_option(self, name: str, value) -> None:
        """Tuning option of this plan (`vrt_plan_set_option`); results never depend on it."""
        if getattr(self, "_h", None):
            check(_lib.load().vrt_plan_set_option(self._h, name.encode(), str(value).encode()))

    def last_sweep_timing(self):
        ms = ctypes.c_double()
        launches = ctypes.c_int64()
        check(_lib.load().vrt_plan_last_sweep_timing(self._h, ctypes.byref(ms),
                                                     ctypes.byref(launches)))
        return ms.value, launches.value

    @property
    def patch_layout(self) -> dict:
        """How the patch path cut this plan: patches, the fewest patches of any (angle, layer), slots of the per-layer
        launches' work lists and how many of them are padding (0 until a per-layer execute has built the lists)."""
        out = (ctypes.c_int64 * 4)()
        check(_lib.load().vrt_plan_patch_layout(self._h, out))
        return {"patches": out[0], "fewest_per_angle_layer": out[1], "work_slots": out[2], "padding_slots": out[3]}

    @property
    def patch_ride_stats(self) -> dict:
        """The riding J reduction (VRT_PATCH_REDUCE_RIDE=1) in the last sweep: per-layer launches that reduced in their
        patch blocks, and the most chunks a block of them took (0, 0: every launch kept its reduction rows)."""
        out = (ctypes.c_int64 * 2)()
        check(_lib.load().vrt_plan_patch_ride_stats(self._h, out))
        return {"launches": int(out[0]), "max_chunks": int(out[1])}

    @property
    def last_launches(self) -> int:
        """Kernel launches of the last execute's sweep (1: the chained patch launch); waits for it to finish and
        raises if a chained launch gave up waiting for a dependency."""
        return int(self.last_sweep_timing()[1])

    @property
    def last_path(self) -> str:
        """Device path of the last execute: "levels", "tiles" or "steps" ("" before the first)."""
        return {0: "", 1: "levels", 2: "tiles", 3: "steps", 4: "patches"}[int(_lib.load().vrt_plan_last_path(self._h))]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.load().vrt_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiDevicePlan:
    """Several GPUs of a node from ONE process (`vrt_multi_*`): a grid + plan per device and an in-process RCCL
    communicator; `execute` is `FormalPlan.execute` for the node (host arrays in, J out), sharded by
    wavelength blocks when nλ >= devices, by angles (one RCCL all-reduce of J) otherwise.  Listing a device
    twice rehearses the sharding on a one-GPU box (no RCCL, partial sums added by a kernel)."""

    def __init__(self, positions, neighbours, bounds, k, dirs=None, n_sweeps: int = 3, devices=(0,)):
        L = _lib.load()
        pos = _f64(positions)
        nbr = np.ascontiguousarray(neighbours, dtype=np.int64)
        b = np.array([float(v) for v in bounds], dtype=np.float64)
        self.k = _f64(np.atleast_2d(k))
        self.n, self.n_angles = pos.shape[0], self.k.shape[0]
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        d = np.ascontiguousarray(dirs, dtype=np.int32) if dirs is not None else None
        h = ctypes.c_void_p()
        check(L.vrt_multi_create(dev.size, dev.ctypes.data_as(_lib.p_int), self.n, _d(pos), _i(nbr), nbr.shape[0], _d(b),
                                 self.n_angles, _d(self.k), d.ctypes.data_as(_lib.p_int) if d is not None else None,
                                 int(n_sweeps), ctypes.byref(h)))
        self._h = h

    def set_shard(self, mode: str) -> None:
        check(_lib.load().vrt_multi_set_shard(self._h, mode.encode()))

    @property
    def last_shard(self) -> str:
        return {0: "", 1: "lambda", 2: "angle"}[int(_lib.load().vrt_multi_last_shard(self._h))]

    @property
    def uses_rccl(self) -> bool:
        return bool(_lib.load().vrt_multi_uses_rccl(self._h))

    def execute(self, S, alpha, weights, I0_up=None, I0_down=None, alpha_mode=None) -> np.ndarray:
        S = _f64(S)
        if S.ndim == 1:
            S = S.reshape(-1, 1)
        n, nlam = S.shape
        alpha = _f64(alpha)
        if alpha_mode is None:
            alpha_mode = {1: _lib.ALPHA_SITE, 2: _lib.ALPHA_SITE_LAM, 3: _lib.ALPHA_ANGLE_SITE_LAM}[alpha.ndim]
        if I0_up is not None:
            I0_up = _f64(I0_up).reshape(-1, nlam)
        if I0_down is not None:
            I0_down = _f64(I0_down).reshape(-1, nlam)
        w = _f64(weights)
        J = np.zeros((n, nlam))
        check(_lib.load().vrt_multi_execute(self._h, nlam, nlam, _d(S), _d(alpha), alpha_mode, _d(I0_up), _d(I0_down),
                                            _d(w), _d(J)))
        return J

    def execute_line(self, S, populations, case, weights, perm_up, n1: int) -> np.ndarray:
        """`vrt_multi_execute_line`: J_λ_voronoi of the line case from host arrays, wavelength blocks over the devices,
        every device making the per-angle α_tot of its own wavelengths (`case`: a LineCase; I_0 = B_0 of the bottom
        layer, lambda_iteration.jl:99-101)."""
        S = _f64(S)
        n, nlam = S.shape
        pops = np.asarray(populations)
        gamma = _f64(case.gamma(pops))
        strength = _f64(case.strength_const * (pops[0] * case.Bij - pops[1] * case.Bji))
        lam, vel, dop, ac = _f64(case.lam), _f64(case.velocity), _f64(case.doppler), _f64(case.alpha_cont)
        I0 = _f64(np.asarray(case.B0)[np.asarray(perm_up)[:n1] - 1])
        J = np.zeros((n, nlam))
        check(_lib.load().vrt_multi_execute_line(self._h, nlam, nlam, _d(lam), float(case.lambda0), float(case.c0), _d(vel),
                                                 _d(dop), _d(gamma), _d(strength), _d(ac), _d(S), _d(I0), None,
                                                 _d(_f64(weights)), _d(J)))
        return J

    def lambda_iteration(self, eps_conv: float, maxiter: int, case, weights, S0=None, populations0=None, checkpoint=None,
                         checkpoint_every: int = 1, resume=None, ng=None, storage: str = "f64"):
        """Λ_voronoi (src/lambda_iteration.jl:205-300) across the devices (`vrt_multi_lambda_*`): wavelength blocks per
        device, one all-reduce of the rate-integral shares per iteration.  Returns (J, S_new, populations (3, n), history).
        S0, populations0, checkpoint, checkpoint_every, resume as for `Lambda_voronoi_host`
        (`vrt_multi_lambda_set_state`: every device takes its wavelength block of S and all the populations).
        ng=(start, period) as for `Lambda_voronoi_host` (`vrt_multi_lambda_set_acceleration`: every device keeps the history
        of its own block, the five sums are added on the host in device order, the step is taken on every device or on
        none); the tuple gains a fifth element, the list of (iterate, applied, a, b) of every due step.
        storage="f32": every device holds its block of S, J, B, I_0 and α as float32 (`vrt_multi_lambda_create_f32`; the
        shares, the all-reduce and the populations stay float64, the patch path only); the returned J and S are float64
        arrays of float32-representable values, checkpoints work unchanged, and `ng` raises ValueError before any device
        work, as for `Lambda_voronoi_host`."""
        f32 = _storage_f32(storage, "lambda_iteration")
        if f32 and ng is not None:
            raise ValueError("lambda_iteration: ng is not available with storage='f32'")
        L = _lib.load()
        lc, keep = case.c_struct()
        n, nlam = self.n, int(keep["lam"].size)
        start = _start_state(S0, populations0, resume, checkpoint_every, n, nlam, "lambda_iteration")
        h = ctypes.c_void_p()
        check((L.vrt_multi_lambda_create_f32 if f32 else L.vrt_multi_lambda_create)(self._h, ctypes.byref(lc), _d(_f64(weights)),
                                                                                    ctypes.byref(h)))
        try:
            if ng is not None:
                if not hasattr(L, "vrt_multi_lambda_set_acceleration"):
                    raise ImportError(f"lambda_iteration: ng needs {_lib.ACCEL_LIB_PATH}, which this build of the library lacks")
                check(L.vrt_multi_lambda_set_acceleration(h, 2, *_ng_settings(ng)))
            J, S, pops, history, steps, i = _session_loop(L, "multi_lambda", h, n, nlam, eps_conv, maxiter, start, checkpoint,
                                                          checkpoint_every, ng, "lambda_iteration")
            if i == 0:
                S[:] = keep["B0"] if start[0] is None else start[0]
                if f32:
                    S[:] = S.astype(np.float32)
                pops[:] = keep["lte"] if start[1] is None else start[1]
            return (J, S, pops, history) if ng is None else (J, S, pops, history, steps)
        finally:
            L.vrt_multi_lambda_destroy(h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.load().vrt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _single(fn_name, k, S, I_0, alpha, sites: VoronoiSites, n_sweeps: int):
    L = _lib.load()
    k = _f64(k)
    S = _f64(S)
    I_0 = _f64(I_0)
    alpha = _f64(alpha)
    if S.shape != (sites.n,) or alpha.shape != (sites.n,):
        raise ValueError("S and alpha must be vectors with one entry per site")
    out = np.zeros(sites.n)
    check(getattr(L, fn_name)(sites.handle, _d(k), _d(S), _d(I_0), I_0.size, _d(alpha),
                              int(n_sweeps), _d(out)))
    return out


def Delaunay_upII(k, S, I_0, alpha, sites: VoronoiSites, n_sweeps: int = 3) -> np.ndarray:
    """Intensity at every site for rays travelling up (src/irregular_ray_tracing.jl:15-82).
    I_0 is the boundary intensity of perm_up[1 : layers_up[2]-1]."""
    return _single("vrt_delaunay_up", k, S, I_0, alpha, sites, n_sweeps)


def Delaunay_downII(k, S, I_0, alpha, sites: VoronoiSites, n_sweeps: int = 3) -> np.ndarray:
    """Intensity at every site for rays travelling down (src/irregular_ray_tracing.jl:96-163)."""
    return _single("vrt_delaunay_down", k, S, I_0, alpha, sites, n_sweeps)


def quadrature_directions(theta, phi) -> np.ndarray:
    return np.stack([direction(t, p) for t, p in zip(theta, phi)])


def J_lambda_voronoi(S_lambda, alpha, sites: VoronoiSites, quadrature: str, I0_up=None,
                     I0_down=None, n_sweeps: int = 3) -> np.ndarray:
    """J_λ_voronoi: mean intensity J = Σ_angles w · I over a quadrature file
    (src/lambda_iteration.jl:60-113 for nλ > 1, src/lambda_continuum.jl:27-56 for the continuum).
    The angle × wavelength loop the reference threads over λ runs as one batched device solve.
    The opacity / boundary-intensity physics stays with the caller: `alpha` is α_tot (per site,
    per (site, λ) or per (angle, site, λ)), `I0_up` is B_λ(T) of the bottom layer
    (lambda_iteration.jl:99-101), `I0_down` defaults to zeros (:105-106)."""
    weights, theta, phi, _ = read_quadrature(quadrature)
    key = (os.path.basename(quadrature), int(n_sweeps))
    plan = sites._plans.get(key)
    if plan is None:
        # the reference branches on θ in degrees (lambda_iteration.jl:98,104), not on sign(k_z)
        dirs = [1 if t > 90 else (-1 if t < 90 else 0) for t in theta]
        plan = FormalPlan(sites, quadrature_directions(theta, phi), n_sweeps, dirs=dirs)
        sites._plans[key] = plan
    J, _ = plan.execute(S_lambda, alpha, weights=weights, I0_up=I0_up, I0_down=I0_down)
    return J


def build_schedule(sites: VoronoiSites, dir: int, up, n_sweeps: int = 3):
    """Host-side dependency schedule of one direction (introspection; works on a device=-1
    handle).  `up` is an (n, 2) array of 1-based upwind ids.  Returns (site ids 1-based sorted by
    level, zero-read flags, level offsets)."""
    L = _lib.load()
    up = np.ascontiguousarray(up, dtype=np.int64)
    h = ctypes.c_void_p()
    check(L.vrt_schedule_build(sites.handle, int(dir), _i(up), int(n_sweeps), ctypes.byref(h)))
    try:
        nn = int(L.vrt_schedule_num_nodes(h))
        nl = int(L.vrt_schedule_num_levels(h))
        site = np.zeros(nn, dtype=np.int64)
        z = np.zeros(nn, dtype=np.int32)
        off = np.zeros(nl + 1, dtype=np.int64)
        check(L.vrt_schedule_get(h, _i(site), z.ctypes.data_as(_lib.p_i32), _i(off)))
    finally:
        L.vrt_schedule_destroy(h)
    return site, z, off


def build_layer_schedule(sites: VoronoiSites, dir: int, up, n_sweeps: int = 3):
    """Layer-local schedule of the LDS layer-tile kernel (introspection, host only).  Returns
    (vis (n,) uint32: four packed 8-bit in-layer visit levels per site, nlev per layer (index =
    1-based layer), number of visits)."""
    L = _lib.load()
    up = np.ascontiguousarray(up, dtype=np.int64)
    vis = np.zeros(sites.n, dtype=np.uint32)
    layers = sites.layers_up if dir > 0 else sites.layers_down
    nlev = np.zeros(layers.size, dtype=np.int32)
    nv = ctypes.c_int64()
    check(L.vrt_layer_schedule(sites.handle, int(dir), _i(up), int(n_sweeps),
                               vis.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                               nlev.ctypes.data_as(_lib.p_i32), ctypes.byref(nv)))
    return vis, nlev, nv.value


def build_patch_schedule(sites: VoronoiSites, dir: int, up, n_sweeps: int = 3, own_target: int = 768,
                         entry_cap: int = 1024) -> dict:
    """Patch schedule of the fused layer kernel (introspection, host only): layers cut into ranges of
    consecutive storage positions, each with its in-layer dependency cone (own sites + halo).
    Returns a dict of numpy arrays (see vrt_patch_schedule_get) plus the counts."""
    L = _lib.load()
    up = np.ascontiguousarray(up, dtype=np.int64)
    h = ctypes.c_void_p()
    cnt = np.zeros(6, dtype=np.int64)
    check(L.vrt_patch_schedule_build(sites.handle, int(dir), _i(up), int(n_sweeps), int(own_target), int(entry_cap),
                                     ctypes.byref(h), _i(cnt)))
    try:
        P, E = int(cnt[0]), int(cnt[1])
        out = {"layer_patch_off": np.zeros(int(cnt[5]), dtype=np.int32), "patch_own_lo": np.zeros(P, dtype=np.int32),
               "patch_own_cnt": np.zeros(P, dtype=np.int32), "patch_nlev": np.zeros(P, dtype=np.int32),
               "patch_ent_off": np.zeros(P + 1, dtype=np.int64), "entry_pos": np.zeros(E, dtype=np.int32),
               "entry_vis": np.zeros(E, dtype=np.uint32), "entry_loc": np.zeros(E, dtype=np.uint32)}
        u32 = ctypes.POINTER(ctypes.c_uint32)
        check(L.vrt_patch_schedule_get(h, out["layer_patch_off"].ctypes.data_as(_lib.p_i32),
                                       out["patch_own_lo"].ctypes.data_as(_lib.p_i32),
                                       out["patch_own_cnt"].ctypes.data_as(_lib.p_i32),
                                       out["patch_nlev"].ctypes.data_as(_lib.p_i32), _i(out["patch_ent_off"]),
                                       out["entry_pos"].ctypes.data_as(_lib.p_i32),
                                       out["entry_vis"].ctypes.data_as(u32), out["entry_loc"].ctypes.data_as(u32)))
        out["dep_off"] = np.zeros(P + 1, dtype=np.int64)
        check(L.vrt_patch_schedule_get_deps(h, _i(out["dep_off"]), None))
        out["dep_list"] = np.zeros(int(out["dep_off"][-1]), dtype=np.int32)
        check(L.vrt_patch_schedule_get_deps(h, None, out["dep_list"].ctypes.data_as(_lib.p_i32)))
        # the angle's layer schedule, as the builder derives it on the way (= build_layer_schedule's outputs)
        out["layer_vis"] = np.zeros(sites.n, dtype=np.uint32)
        out["layer_nlev"] = np.zeros((sites.layers_up if dir > 0 else sites.layers_down).size, dtype=np.int32)
        nv = ctypes.c_int64()
        check(L.vrt_patch_schedule_get_layers(h, out["layer_vis"].ctypes.data_as(u32),
                                              out["layer_nlev"].ctypes.data_as(_lib.p_i32), ctypes.byref(nv)))
        out["layer_visits"] = nv.value
    finally:
        L.vrt_patch_schedule_destroy(h)
    out.update(patches=P, entries=E, visits=int(cnt[2]), live_visits=int(cnt[3]), max_entries=int(cnt[4]))
    return out


def layer_sorted_slots(sites: VoronoiSites, dir: int, vis):
    """Thread assignment of the layer-step level kernel for a layer schedule `vis` (host only):
    (store, self) = 1-based site id per storage position, 0-based storage position per sorted
    index (inside each layer sorted stably by visit pattern)."""
    vis = np.ascontiguousarray(vis, dtype=np.uint32)
    store = np.zeros(sites.n, dtype=np.int64)
    self_ = np.zeros(sites.n, dtype=np.int64)
    check(_lib.load().vrt_layer_sorted_slots(sites.handle, int(dir), vis.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                             _i(store), _i(self_)))
    return store, self_


# ---- regular grid ---------------------------------------------------------------
def short_characteristics_batch(k, up, S_0, I_0, alpha, z, x, y, n_sweeps: int = 3, device: int = 0):
    """Batched regular-grid formal solve.  k (n_solve, 3); up (n_solve,) bools; S_0 / alpha either
    one array (ny, nx, nz) shared by every solve or (n_solve, ny, nx, nz); I_0 (n_solve, ny, nx).
    numpy C-order (ny, nx, nz) is Julia's (nz, nx, ny).  Returns I (n_solve, ny, nx, nz)."""
    k = _f64(np.atleast_2d(k))
    ns = k.shape[0]
    upv = np.ascontiguousarray(np.asarray(up, dtype=bool).reshape(ns), dtype=np.int32)
    z, x, y = _f64(z), _f64(x), _f64(y)
    nz, nx, ny = z.size, x.size, y.size
    S_0, alpha, I_0 = _f64(S_0), _f64(alpha), _f64(I_0)
    vol = nz * nx * ny

    def stride(a, name):
        if a.shape == (ny, nx, nz):
            return 0
        if a.shape == (ns, ny, nx, nz):
            return vol
        raise ValueError(f"{name} has shape {a.shape}, expected {(ny, nx, nz)} or {(ns, ny, nx, nz)}")
    sS, sA = stride(S_0, "S_0"), stride(alpha, "alpha")
    I_0 = I_0.reshape(ns, ny, nx)
    out = np.zeros((ns, ny, nx, nz))
    check(_lib.load().vrt_short_characteristics(nz, nx, ny, _d(z), _d(x), _d(y), ns, _d(k),
                                                upv.ctypes.data_as(_lib.p_int), _d(S_0), sS, _d(alpha),
                                                sA, _d(I_0), int(n_sweeps), int(device), _d(out)))
    return out


def short_characteristics_up(k, S_0, I_0, alpha, z, x, y, n_sweeps: int = 3, device: int = 0):
    """Intensity on the regular grid for rays travelling up (src/characteristics.jl:19-95);
    the reference's `atmos` argument is replaced by its three axes."""
    return short_characteristics_batch([k], [True], S_0, I_0, alpha, z, x, y, n_sweeps, device)[0]


def short_characteristics_down(k, S_0, I_0, alpha, z, x, y, n_sweeps: int = 3, device: int = 0):
    """Intensity on the regular grid for rays travelling down (src/characteristics.jl:110-180)."""
    return short_characteristics_batch([k], [False], S_0, I_0, alpha, z, x, y, n_sweeps, device)[0]


class RegularSolver:
    """Device-resident regular-grid short characteristics (`vrt_regular_*`): the handle owns the
    grid axes and workspaces; `execute_dev` takes device pointers (torch `data_ptr()`) to S, alpha
    (Julia (nz, nx, ny) order, shared or per solve), I_0 (nx, ny, n_solve) and the output
    (nz, nx, ny, n_solve), and is asynchronous on `stream`."""

    def __init__(self, z, x, y, device: int = 0):
        z, x, y = _f64(z), _f64(x), _f64(y)
        self.nz, self.nx, self.ny = z.size, x.size, y.size
        self._h = ctypes.c_void_p()
        check(_lib.load().vrt_regular_create(self.nz, self.nx, self.ny, _d(z), _d(x), _d(y), int(device),
                                             ctypes.byref(self._h)))

    def execute_dev(self, k, up, dS: int, S_stride: int, dalpha: int, alpha_stride: int, dI0: int,
                    dI_out: int, n_sweeps: int = 3, stream: int = 0, field_period: int = 0):
        k = _f64(np.atleast_2d(k))
        ns = k.shape[0]
        upv = np.ascontiguousarray(np.asarray(up, dtype=bool).reshape(ns), dtype=np.int32)
        check(_lib.load().vrt_regular_execute_dev(self._h, ns, _d(k), upv.ctypes.data_as(_lib.p_int), dS,
                                                  int(S_stride), dalpha, int(alpha_stride), int(field_period),
                                                  dI0, int(n_sweeps), dI_out, stream or None))

    def last_solve_ms(self) -> float:
        out = ctypes.c_double()
        check(_lib.load().vrt_regular_last_solve_ms(self._h, ctypes.byref(out)))
        return out.value

    def last_launch_form(self):
        """What the last batch of solves was launched as (`vrt_regular_last_launch_form`): (form, threads, rows) with
        form one of `_lib.REG_FORMS`, threads the workgroup size, and rows -- the solve forms only, else None -- a dict
        {"yz": ..., "xz": ...} of "row_march" / "strided": the row loop a plane of that kind takes in this launch."""
        form, threads = ctypes.c_int(), ctypes.c_int()
        check(_lib.load().vrt_regular_last_launch_form(self._h, ctypes.byref(form), ctypes.byref(threads)))
        name = _lib.REG_FORMS[form.value & _lib.REG_FORM_KERNEL_MASK]
        rows = None
        if name.startswith("solve"):
            rows = {"yz": "row_march" if form.value & _lib.REG_FORM_YZ_ROW_MARCH else "strided",
                    "xz": "row_march" if form.value & _lib.REG_FORM_XZ_ROW_MARCH else "strided"}
        return name, threads.value, rows

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.load().vrt_regular_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- emergent spectra (src/plot_utils.jl: plotter :297-355, write_top_intensity :101-140, write_tau_unity :434-576) ----
SYNTH_FIELDS = ("velocity", "doppler", "gamma_static", "gamma_unsold", "temperature", "alpha_cont")


def periodic_axis(a) -> np.ndarray:
    """periodic_borders of an axis (src/atmosphere.jl:166-181): one ghost point either side, spaced a[1] - a[0]."""
    a = _f64(a).ravel()
    d = a[1] - a[0]
    return np.concatenate([[a[0] - d], a, [a[-1] + d]])


def _synth_consts(case, src_const, g_ratio):
    return (float(case.lambda0), float(case.c0), float(case.hc_over_kB), float(case.strength_const), float(case.Bij),
            float(case.Bji), float(src_const), float(g_ratio))


def _raster_inputs(raster, populations=None):
    """the raster's axes and fields as contiguous float64: velocity (3, ny, nx, nz), the others (ny, nx, nz),
    populations (nf >= 2, ny, nx, nz) of which the first two are used"""
    z, x, y = _axes(raster["z"], raster["x"], raster["y"])
    shape = (y.size, x.size, z.size)
    f = {}
    for name in SYNTH_FIELDS:
        a = _f64(raster[name])
        want = (3,) + shape if name == "velocity" else shape
        if a.shape != want:
            raise ValueError(f"raster field {name} has shape {a.shape}, expected {want}")
        f[name] = a
    if populations is not None:
        p = _f64(populations)
        if p.ndim != 4 or p.shape[0] < 2 or p.shape[1:] != shape:
            raise ValueError(f"populations have shape {p.shape}, expected (nf >= 2,) + {shape}")
        f["populations"] = np.ascontiguousarray(p[:2])
    return z, x, y, f


def synth_opacity(k, raster, populations, case, src_const: float, g_ratio: float = 4.0, lam=None, planck2=None,
                  device: int = 0):
    """plotter (src/plot_utils.jl:297-355) for one direction k on a raster (`vrt_synth_opacity`): the source function
    S = (α_l S_l + α_c S_c)/(α_l + α_c) and α_tot = α_l + α_c of every wavelength, with the periodic ghost border of
    periodic_borders.  `raster`: dict of the axes z, x, y and the fields velocity (3, ny, nx, nz) [z, x, y components],
    doppler, gamma_static, gamma_unsold, temperature, alpha_cont (ny, nx, nz); populations (nf >= 2, ny, nx, nz) as
    Voronoi_to_Raster_inv_dist returns them.  `case` gives lambda0, c0, hc_over_kB, strength_const, Bij, Bji and, unless
    passed, lam and planck2 (a LineCase does); src_const = 2hc²/λ0⁵, g_ratio = g_u/g_l (source_line, line.jl:385-393).
    Returns S, alpha, each (nlam, ny + 2, nx + 2, nz)."""
    z, x, y, f = _raster_inputs(raster, populations)
    lam = _f64(case.lam if lam is None else lam).ravel()
    planck2 = _f64(case.planck2 if planck2 is None else planck2).ravel()
    if planck2.size != lam.size:
        raise ValueError("lam and planck2 must have the same length")
    k = _f64(k).ravel()
    shape = (lam.size, y.size + 2, x.size + 2, z.size)
    S, A = np.zeros(shape), np.zeros(shape)
    check(_lib.load().vrt_synth_opacity(int(device), z.size, x.size, y.size, _d(k), lam.size, _d(lam), _d(planck2),
                                        *_synth_consts(case, src_const, g_ratio),
                                        *[_d(f[n]) for n in SYNTH_FIELDS + ("populations",)], _d(S), _d(A)))
    return S, A


def synth_opacity_dev(k, nz: int, nx: int, ny: int, case, src_const: float, d_fields: dict, d_populations: int,
                      d_S: int, d_alpha: int, g_ratio: float = 4.0, lam=None, planck2=None, stream: int = 0) -> None:
    """Device form (`vrt_synth_opacity_dev`, on the current device, asynchronous on `stream`): d_fields maps
    SYNTH_FIELDS to device pointers (torch data_ptr()) of the layouts of `synth_opacity`; d_S, d_alpha receive
    (nlam, ny + 2, nx + 2, nz).  Chunk wavelengths by passing slices of lam / planck2."""
    lam = _f64(case.lam if lam is None else lam).ravel()
    planck2 = _f64(case.planck2 if planck2 is None else planck2).ravel()
    if planck2.size != lam.size:
        raise ValueError("lam and planck2 must have the same length")
    k = _f64(k).ravel()
    check(_lib.load().vrt_synth_opacity_dev(int(nz), int(nx), int(ny), _d(k), lam.size, _d(lam), _d(planck2),
                                            *_synth_consts(case, src_const, g_ratio),
                                            *[d_fields[n] or None for n in SYNTH_FIELDS], d_populations or None,
                                            d_S or None, d_alpha or None, stream or None))


def top_intensity(k, S, alpha, z, x, y, n_sweeps: int = 3, device: int = 0) -> np.ndarray:
    """write_top_intensity (src/plot_utils.jl:101-140) for one direction (`vrt_top_intensity`): per wavelength
    short_characteristics_up with I_0 = the bottom plane of S, of which the top plane's interior is returned,
    (nlam, ny, nx).  S, alpha (nlam, ny + 2, nx + 2, nz) with the periodic ghost border; z, x, y the raster's own
    (interior) axes -- the solver's are periodic_axis(x), periodic_axis(y)."""
    z, xg, yg = _f64(z).ravel(), periodic_axis(x), periodic_axis(y)
    S, alpha = _f64(S), _f64(alpha)
    shape = (yg.size, xg.size, z.size)
    if S.ndim != 4 or S.shape[1:] != shape or alpha.shape != S.shape:
        raise ValueError(f"S and alpha must be (nlam,) + {shape}, got {S.shape} and {alpha.shape}")
    nlam = S.shape[0]
    k = _f64(k).ravel()
    out = np.zeros((nlam, yg.size - 2, xg.size - 2))
    check(_lib.load().vrt_top_intensity(z.size, xg.size, yg.size, _d(z), _d(xg), _d(yg), _d(k), nlam, _d(S), _d(alpha),
                                        int(n_sweeps), int(device), _d(out)))
    return out


def top_intensity_dev(solver: "RegularSolver", k, nlam: int, dS: int, dalpha: int, dI_top: int, n_sweeps: int = 3,
                      stream: int = 0) -> None:
    """Device form (`vrt_regular_emergent_dev`): `solver` is a RegularSolver on the ghosted axes, dS / dalpha hold
    nlam ghosted arrays, dI_top receives (nlam, ny - 2, nx - 2) of the solver's sizes.  Asynchronous on `stream`."""
    k = _f64(k).ravel()
    check(_lib.load().vrt_regular_emergent_dev(solver._h, _d(k), int(nlam), dS or None, dalpha or None, int(n_sweeps),
                                               dI_top or None, stream or None))


def tau_unity(k, alpha, z, x, y, device: int = 0) -> np.ndarray:
    """Heights of τ = 1 (write_tau_unity, src/plot_utils.jl:434-576; `vrt_tau_unity`) along the up solve's
    characteristic of direction k, traced back from the top plane: alpha (nlam, ny + 2, nx + 2, nz) ghosted, z, x, y
    the interior axes (x, y uniform, periodic).  Returns (nlam, ny, nx) heights.  At k = (±1, 0, 0) this is
    write_tau_unity(DATA) exactly; the inclined reference's defects are not reproduced."""
    z, x, y = _axes(z, x, y)
    alpha = _f64(alpha)
    shape = (y.size + 2, x.size + 2, z.size)
    if alpha.ndim != 4 or alpha.shape[1:] != shape:
        raise ValueError(f"alpha must be (nlam,) + {shape}, got {alpha.shape}")
    nlam = alpha.shape[0]
    k = _f64(k).ravel()
    out = np.zeros((nlam, y.size, x.size))
    check(_lib.load().vrt_tau_unity(z.size, x.size, y.size, _d(z), _d(x), _d(y), _d(k), nlam, _d(alpha), int(device),
                                    _d(out)))
    return out


def tau_unity_dev(k, z, x, y, nlam: int, d_alpha: int, d_height: int, stream: int = 0) -> None:
    """Device form (`vrt_tau_unity_dev`, on the current device): d_alpha (nlam, ny + 2, nx + 2, nz), d_height
    (nlam, ny, nx).  Synchronises `stream`."""
    z, x, y = _axes(z, x, y)
    k = _f64(k).ravel()
    check(_lib.load().vrt_tau_unity_dev(z.size, x.size, y.size, _d(z), _d(x), _d(y), _d(k), int(nlam), d_alpha or None,
                                        d_height or None, stream or None))


def emergent_spectrum(sites: "VoronoiSites", populations, raster, case, theta: float, phi: float, *, src_const: float,
                      g_ratio: float = 4.0, n_sweeps: int = 3, tau: bool = False, chunk: int = 0,
                      periodic: bool = False, device: int = 0):
    """The observable of a study, on the device: read_irregular's resampling of the site populations (n, nf >= 2) onto
    the raster (Voronoi_to_Raster_inv_dist, src/plot_utils.jl:252-295), plotter's S and α_tot for the direction (θ, ϕ)
    in degrees (:297-355), write_top_intensity's solve (:101-140) and, with `tau`, write_tau_unity's heights
    (:434-576), wavelength chunk by chunk (`chunk` wavelengths; 0: S and α of a chunk within 4 GiB).  `raster` and
    `case` as in synth_opacity.  Only the results leave the device: returns I_top (nlam, ny, nx), and with `tau` also
    the heights (nlam, ny, nx)."""
    import torch

    z, x, y, f = _raster_inputs(raster)
    pops = _f64(populations)
    if pops.ndim != 2 or pops.shape[0] != sites.n or pops.shape[1] < 2:
        raise ValueError(f"populations must be (n, nf >= 2) with n = {sites.n}, got {pops.shape}")
    if not all(np.all(np.diff(a) > 0) for a in (z, x, y)) or min(z.size, x.size, y.size) < 2:
        raise ValueError("the raster axes must be ascending with at least two points each")
    lam, planck2 = _f64(case.lam).ravel(), _f64(case.planck2).ravel()
    nz, nx, ny, nlam = z.size, x.size, y.size, lam.size
    volg = nz * (nx + 2) * (ny + 2)
    chunk = int(chunk) if chunk > 0 else max(1, (4 << 30) // (16 * volg))
    chunk = min(chunk, nlam)
    k = direction(theta, phi)
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_site = up(pops[:, :2])
        d_pops = torch.empty((2, ny, nx, nz), dtype=torch.float64, device=dev)
        Voronoi_to_Raster_dev(sites, z, x, y, 2, 2, d_site.data_ptr(), d_pops.data_ptr(), inv_dist=True,
                              periodic=periodic, stream=stream)
        d_f = {n: up(f[n]) for n in SYNTH_FIELDS}
        ptr = {n: t.data_ptr() for n, t in d_f.items()}
        d_S = torch.empty((chunk, ny + 2, nx + 2, nz), dtype=torch.float64, device=dev)
        d_A = torch.empty_like(d_S)
        I_top = torch.empty((nlam, ny, nx), dtype=torch.float64, device=dev)
        H = torch.empty_like(I_top) if tau else None
        solver = RegularSolver(z, periodic_axis(x), periodic_axis(y), device=int(device))
        try:
            for l0 in range(0, nlam, chunk):
                nc = min(chunk, nlam - l0)
                synth_opacity_dev(k, nz, nx, ny, case, src_const, ptr, d_pops.data_ptr(), d_S.data_ptr(), d_A.data_ptr(),
                                  g_ratio=g_ratio, lam=lam[l0:l0 + nc], planck2=planck2[l0:l0 + nc], stream=stream)
                top_intensity_dev(solver, k, nc, d_S.data_ptr(), d_A.data_ptr(), I_top[l0].data_ptr(), n_sweeps,
                                  stream=stream)
                if tau:
                    tau_unity_dev(k, z, x, y, nc, d_A.data_ptr(), H[l0].data_ptr(), stream=stream)
            torch.cuda.current_stream(dev).synchronize()
        finally:
            solver.close()
        out = I_top.cpu().numpy()
        return (out, H.cpu().numpy()) if tau else out


# ---- resampling between the sites and regular rasters -------------------------------------------------
def _metric(periodic: bool) -> int:
    return _lib.METRIC_PERIODIC_XY if periodic else _lib.METRIC_EUCLIDEAN


def nearest_sites(sites: VoronoiSites, points, k: int = 1, periodic: bool = False):
    """The k (1 or 2) nearest sites of `points` (nq, 3) [z, x, y] by a walk over the grid's neighbour rows
    (`vrt_grid_nearest`; exact when the rows are the Voronoi neighbours).  `periodic` = minimum image in x and y;
    the default is the reference's Euclidean KDTree.  Ties go to the lowest id.  Returns (idx 1-based, dist), each
    of shape (nq,) for k = 1 and (nq, 2) for k = 2."""
    q = _f64(points).reshape(-1, 3)
    nq = q.shape[0]
    idx = np.zeros((nq, k), dtype=np.int64)
    dist = np.zeros((nq, k))
    check(_lib.load().vrt_grid_nearest(sites.handle, nq, _d(q), _metric(periodic), int(k), _i(idx), _d(dist)))
    return (idx[:, 0], dist[:, 0]) if k == 1 else (idx, dist)


def _axes(z, x, y):
    return _f64(z).ravel(), _f64(x).ravel(), _f64(y).ravel()


def _to_raster(sites, fields, z, x, y, periodic, mode):
    z, x, y = _axes(z, x, y)
    f = _f64(fields)
    one = f.ndim == 1
    f = f.reshape(sites.n, -1)
    nf = f.shape[1]
    out = np.zeros((nf, y.size, x.size, z.size))
    check(_lib.load().vrt_grid_to_raster(sites.handle, z.size, x.size, y.size, _d(z), _d(x), _d(y), _metric(periodic),
                                         mode, nf, nf, _d(f), _d(out)))
    return out[0] if one else out


def Voronoi_to_Raster(sites: VoronoiSites, fields, z, x, y, periodic: bool = False):
    """Voronoi_to_Raster (src/voronoi_utils.jl:407-617): the value of the nearest site at every raster point.
    fields (n, nf) or (n,); returns (nf, ny, nx, nz) -- Julia's (nz, nx, ny, nf) -- or (ny, nx, nz)."""
    return _to_raster(sites, fields, z, x, y, periodic, _lib.RASTER_NEAREST)


def Voronoi_to_Raster_inv_dist(sites: VoronoiSites, fields, z, x, y, periodic: bool = False):
    """Voronoi_to_Raster_inv_dist (src/voronoi_utils.jl:773-816): the two nearest sites weighted by 1/d
    (inv_dist_itp, p = 1); a raster point on a site takes that site's value (the reference's NaN).  Shapes as
    Voronoi_to_Raster."""
    return _to_raster(sites, fields, z, x, y, periodic, _lib.RASTER_INV_DIST2)


def initialise(sites: VoronoiSites, z, x, y, raster_fields):
    """initialise (src/voronoi_utils.jl:687-707): trilinear interpolation (src/functions.jl:207-248) of raster
    fields (nf, ny, nx, nz) or (ny, nx, nz) onto the sites; returns (n, nf) or (n,)."""
    z, x, y = _axes(z, x, y)
    r = _f64(raster_fields)
    one = r.ndim == 3
    r = r.reshape(-1, y.size, x.size, z.size)
    nf = r.shape[0]
    out = np.zeros((sites.n, nf))
    check(_lib.load().vrt_raster_to_grid(sites.handle, z.size, x.size, y.size, _d(z), _d(x), _d(y), nf, _d(r), nf,
                                         _d(out)))
    return out[:, 0] if one else out


def Voronoi_to_Raster_dev(sites: VoronoiSites, z, x, y, nf: int, ld: int, d_fields: int, d_raster: int,
                          inv_dist: bool = False, periodic: bool = False, stream: int = 0) -> None:
    """Device form (`vrt_grid_to_raster_dev`): fields (n, ld) rows of which the first nf are used (torch
    data_ptr()), raster (nf, ny, nx, nz) -- per field the S array RegularSolver.execute_dev reads.  Synchronises
    `stream`."""
    z, x, y = _axes(z, x, y)
    mode = _lib.RASTER_INV_DIST2 if inv_dist else _lib.RASTER_NEAREST
    check(_lib.load().vrt_grid_to_raster_dev(sites.handle, z.size, x.size, y.size, _d(z), _d(x), _d(y),
                                             _metric(periodic), mode, int(nf), int(ld), d_fields, d_raster,
                                             stream or None))


def initialise_dev(sites: VoronoiSites, z, x, y, nf: int, d_raster: int, ld: int, d_fields: int, stream: int = 0) -> None:
    """Device form of `initialise` (`vrt_raster_to_grid_dev`): raster (nf, ny, nx, nz) -> fields (n, ld), the first
    nf of every row written.  Synchronises `stream`."""
    z, x, y = _axes(z, x, y)
    check(_lib.load().vrt_raster_to_grid_dev(sites.handle, z.size, x.size, y.size, _d(z), _d(x), _d(y), int(nf),
                                             d_raster, int(ld), d_fields, stream or None))


def raster_stats(sites: VoronoiSites) -> dict:
    """The grid's last nearest search (`vrt_grid_raster_stats`): walk and gather kernel times (ms), queries, summed
    walk steps, queries that took the Euclidean cell-list search."""
    ms = (ctypes.c_double(), ctypes.c_double())
    cnt = (ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64())
    check(_lib.load().vrt_grid_raster_stats(sites.handle, ctypes.byref(ms[0]), ctypes.byref(ms[1]),
                                            *[ctypes.byref(c) for c in cnt]))
    return {"nearest_ms": ms[0].value, "gather_ms": ms[1].value, "queries": cnt[0].value,
            "walk_steps": cnt[1].value, "fallbacks": cnt[2].value}


# ---- sites sampled from a raster density (src/functions.jl:79-120, src/sample_grids.jl) ------------------------------
def _seed(seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in [0, 2^64)")
    return seed


def rejection_sampling(n_sites: int, z, x, y, quantity, seed: int, max_proposals: int = 0, batch: int = 0,
                       device: int = 0, return_proposals: bool = False):
    """rejection_sampling (src/functions.jl:79-120) on the device (`vrt_sample_sites`), the raster's axes and
    `quantity` (ny, nx, nz) -- Julia's (nz, nx, ny), the layout `initialise` reads -- in place of `atmos`.

    Proposal j is uniform in the box of the axes' end points and is accepted when the trilinear value of `quantity`
    there exceeds u*(q_max - q_min) + q_min, u uniform: the reference's test, so the sites are distributed
    proportionally to q - q_min, not to q.  The uniforms are synth.counter_uniform(seed, c, j), c = 0..3, so the
    result depends on (axes, quantity, n_sites, seed) only; Julia's RNG stream is not reproduced.  Returns the
    positions (n_sites, 3) [z, x, y] of the first n_sites accepted proposals, and with `return_proposals` also the
    proposals used (1 + the j of the last).  `max_proposals` caps the proposals (0: 1000*n_sites + 2^20; reaching
    it raises VrtError); `batch` is the proposals per device batch (0: the library chooses; the result does not
    depend on it)."""
    z, x, y = _axes(z, x, y)
    q = _f64(quantity)
    if q.size != z.size * x.size * y.size:
        raise ValueError("quantity must hold ny*nx*nz values (layout (ny, nx, nz))")
    pos = np.zeros((max(int(n_sites), 0), 3))
    used = ctypes.c_int64()
    check(_lib.load().vrt_sample_sites(int(device), z.size, x.size, y.size, _d(z), _d(x), _d(y), _d(q), int(n_sites),
                                       _seed(seed), int(batch), int(max_proposals), _d(pos), ctypes.byref(used)))
    return (pos, used.value) if return_proposals else pos


def rejection_sampling_dev(n_sites: int, z, x, y, d_quantity: int, seed: int, d_positions: int,
                           max_proposals: int = 0, batch: int = 0, device: int = 0, stream: int = 0) -> int:
    """Device form (`vrt_sample_sites_dev`): quantity (ny, nx, nz) and positions (n_sites, 3) are device pointers
    (torch data_ptr()); q_min and q_max come from a device reduction.  Returns the proposals used.  Synchronises
    `stream`."""
    z, x, y = _axes(z, x, y)
    used = ctypes.c_int64()
    check(_lib.load().vrt_sample_sites_dev(int(device), z.size, x.size, y.size, _d(z), _d(x), _d(y), d_quantity,
                                           int(n_sites), _seed(seed), int(batch), int(max_proposals), d_positions,
                                           ctypes.byref(used), stream or None))
    return used.value


def sample_from_invNH_invT(z, x, y, N_H, T, n_sites: int, seed: int, **kw):
    """sample_from_invNH_invT (src/sample_grids.jl:223-230): q = log10(N_H)^-2 * T^(-2/5), formed on the host as
    written there (Julia's literal ^-2 is inv(v)*inv(v)); arrays (ny, nx, nz).  Keywords go to rejection_sampling."""
    inv = 1.0 / np.log10(_f64(N_H))
    return rejection_sampling(n_sites, z, x, y, (inv * inv) * _f64(T) ** (-2 / 5), seed, **kw)


def sample_from_logNH_invT(z, x, y, N_H, T, n_sites: int, seed: int, **kw):
    """sample_from_logNH_invT (src/sample_grids.jl:198-206): q = log10(N_H) * T^(-2/5)."""
    return rejection_sampling(n_sites, z, x, y, np.log10(_f64(N_H)) * _f64(T) ** (-2 / 5), seed, **kw)


def sample_from_logNH_invT_rootv(z, x, y, N_H, T, vx, vy, vz, n_sites: int, seed: int, **kw):
    """sample_from_logNH_invT_rootv (src/sample_grids.jl:208-221): q = log10(N_H) * T^(-2/5) * (vx^2 + vy^2 +
    vz^2)^(1/3)."""
    vx, vy, vz = _f64(vx), _f64(vy), _f64(vz)
    v_sqrd = vx * vx + vy * vy + vz * vz
    q = np.log10(_f64(N_H)) * _f64(T) ** (-2 / 5) * v_sqrd ** (1 / 3)
    return rejection_sampling(n_sites, z, x, y, q, seed, **kw)


def sample_from_temp_gradient(z, x, y, T, n_sites: int, seed: int, **kw):
    """sample_from_temp_gradient (src/sample_grids.jl:97-115): q = |dT/dz| with T (ny, nx, nz); every plane but the
    last takes the forward difference (T[k+1] - T[k])/(z[k+1] - z[k]), the last the backward one, as there."""
    z, T = _f64(z).ravel(), _f64(T)
    if T.shape[-1] != z.size or z.size < 2:
        raise ValueError("T must be (ny, nx, nz) with nz = len(z) >= 2")
    g = np.empty_like(T)
    g[..., :-1] = (T[..., 1:] - T[..., :-1]) / (z[1:] - z[:-1])
    g[..., -1] = (T[..., -1] - T[..., -2]) / (z[-1] - z[-2])
    return rejection_sampling(n_sites, z, x, y, np.abs(g), seed, **kw)


def ng_accelerate_dev(count: int, d_x0: int, d_x1: int, d_x2: int, d_x3: int, d_out: int, stream: int = 0):
    """Second-order Ng step (`vrt_ng_accelerate_dev`) on device pointers (torch data_ptr()) of `count` doubles, x0 the
    newest iterate; d_out aliases no input.  Returns (applied, sums (A1, B1, C1, B2, C2), coeffs (a, b)); synchronises."""
    sums, coeffs, applied = np.zeros(5), np.zeros(2), ctypes.c_int(0)
    check(_lib.load().vrt_ng_accelerate_dev(int(count), d_x0, d_x1, d_x2, d_x3, d_out, _d(sums), _d(coeffs),
                                            ctypes.byref(applied), stream or None))
    return bool(applied.value), sums, coeffs


def ng_accelerate(x0, x1, x2, x3, device: int = 0):
    """Second-order Ng extrapolation (Ng 1974; Olson, Auer & Buchler 1986) from the last four iterates of a positive
    quantity, x0 the newest: host arrays of one shape, staged through the device.  Returns (x_acc, sums, coeffs) with
    x_acc = (c x0 + a x1) + b x2, c = (1 - a) - b, or x_acc = None when the step is rejected (a sum or the determinant
    not finite or zero, or an x_acc that is not finite and positive)."""
    import torch
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in (x0, x1, x2, x3)]
    if any(x.shape != xs[0].shape for x in xs):
        raise ValueError("ng_accelerate: the four iterates must have one shape")
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        d = [torch.from_numpy(x.reshape(-1)).to(dev) for x in xs]
        out = torch.empty_like(d[0])
        applied, sums, coeffs = ng_accelerate_dev(xs[0].size, *(t.data_ptr() for t in d), out.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream)
        return (out.cpu().numpy().reshape(xs[0].shape) if applied else None), sums, coeffs


def ng_sums_dev(count: int, d_x0: int, d_x1: int, d_x2: int, d_x3: int, stream: int = 0) -> np.ndarray:
    """The five sums (A1, B1, C1, B2, C2) of the Ng step over `count` doubles at device pointers (`vrt_ng_sums_dev`): the
    bits `ng_accelerate_dev` reports for the same arrays.  A caller that holds S in pieces adds the pieces' sums in one
    fixed order and hands the total to `ng_coefficients`.  Synchronises."""
    sums = np.zeros(5)
    check(_lib.load().vrt_ng_sums_dev(int(count), d_x0, d_x1, d_x2, d_x3, _d(sums), stream or None))
    return sums


def ng_coefficients(sums):
    """(a, b) of the Ng step from its five sums (`vrt_ng_coefficients`, host only, the library's order of operations), or
    None when a sum or the determinant is not finite or the determinant is zero."""
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.shape != (5,):
        raise ValueError("ng_coefficients: five sums (A1, B1, C1, B2, C2)")
    coeffs = np.zeros(2)
    rc = _lib.load().vrt_ng_coefficients(_d(s), _d(coeffs))
    if rc < 0:
        check(rc)
    if rc == 0:
        return None
    return float(coeffs[0]), float(coeffs[1])


def ng_apply_dev(count: int, a: float, b: float, d_x0: int, d_x1: int, d_x2: int, d_out: int, stream: int = 0) -> bool:
    """x_acc = (c x0 + a x1) + b x2, c = (1 - a) - b, into d_out (`vrt_ng_apply_dev`; aliases no input).  Returns False
    when some x_acc is not finite or not > 0 (d_out is then unspecified).  Synchronises."""
    good = ctypes.c_int(0)
    check(_lib.load().vrt_ng_apply_dev(int(count), float(a), float(b), d_x0, d_x1, d_x2, d_out, ctypes.byref(good),
                                       stream or None))
    return bool(good.value)


def _ng_staged(arrays, device: int, who: str):
    import torch
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in arrays]
    if any(x.shape != xs[0].shape for x in xs):
        raise ValueError(f"{who}: the iterates must have one shape")
    dev = torch.device("cuda", int(device))
    return xs[0].shape, dev, [torch.from_numpy(x.reshape(-1)).to(dev) for x in xs]


def ng_sums(x0, x1, x2, x3, device: int = 0) -> np.ndarray:
    """`ng_sums_dev` for host arrays of one shape, staged through the device."""
    import torch
    _, dev, d = _ng_staged((x0, x1, x2, x3), device, "ng_sums")
    with torch.cuda.device(dev):
        return ng_sums_dev(d[0].numel(), *(t.data_ptr() for t in d), torch.cuda.current_stream(dev).cuda_stream)


def ng_apply(a: float, b: float, x0, x1, x2, device: int = 0):
    """`ng_apply_dev` for host arrays of one shape, staged through the device.  Returns (x_acc, good); x_acc is None when
    the verdict is bad."""
    import torch
    shape, dev, d = _ng_staged((x0, x1, x2), device, "ng_apply")
    with torch.cuda.device(dev):
        out = torch.empty_like(d[0])
        good = ng_apply_dev(d[0].numel(), a, b, *(t.data_ptr() for t in d), out.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream)
        return (out.cpu().numpy().reshape(shape) if good else None), good


def _ng_settings(ng):
    start, period = (int(v) for v in ng)
    return start, period


def _ng_last(fn, h, i, steps):
    """appends (iterate, applied, a, b) of iterate i when a step was due"""
    applied, coeffs = ctypes.c_int(0), np.zeros(2)
    check(fn(h, ctypes.byref(applied), None, _d(coeffs)))
    if applied.value:
        steps.append((i, applied.value == 1, float(coeffs[0]), float(coeffs[1])))


def lambda_update_dev(sites: VoronoiSites, nlam: int, ld: int, dJ: int, dB: int, deps: int, dS_old: int,
                      dS_new: int, stream: int = 0) -> float:
    """Device-resident Λ-iteration epilogue: S_new = (1 - ε) J + ε B (src/lambda_iteration.jl:261-263)
    and the convergence measure max |1 - S_old/S_new| of `criterion` (:325-349), which is returned.
    Arguments are device pointers (torch data_ptr())."""
    out = ctypes.c_double()
    check(_lib.load().vrt_lambda_update_dev(sites.handle, nlam, ld, dJ, dB, deps, dS_old, dS_new,
                                            ctypes.byref(out), stream or None))
    return out.value


def lambda_update_native_dev(sites: VoronoiSites, nlam: int, dJ_up: int, dJ_down: int, dB_up: int, deps: int, dS_up: int,
                             dS_down: int, stream: int = 0) -> float:
    """`lambda_update_dev` on sweep-order plane sets (`vrt_lambda_update_native_dev`): J = J_up + J_down, B in the up
    order, the old S read from and the new S written to dS_up (and its down-order copy to dS_down)."""
    out = ctypes.c_double()
    check(_lib.load().vrt_lambda_update_native_dev(sites.handle, nlam, dJ_up or None, dJ_down or None, dB_up, deps, dS_up,
                                                   dS_down, ctypes.byref(out), stream or None))
    return out.value


def lambda_ali_update_dev(sites: VoronoiSites, nlam: int, ld: int, dJ: int, dB: int, deps: int, d_diag: int, dS_old: int,
                          dS_new: int, stream: int = 0):
    """`lambda_update_dev` with the diagonal operator (`vrt_lambda_ali_update_dev`): with t = 1 - ε,
    S_new = (t (J - Λ* S_old) + ε B) / (1 - t Λ*), d_diag = Λ* as one more (n, ld) array; an entry whose denominator is not
    > 0 takes the plain update.  Returns (the criterion's maximum, the number of such entries)."""
    out, cnt = ctypes.c_double(), ctypes.c_int64()
    check(_lib.load().vrt_lambda_ali_update_dev(sites.handle, nlam, ld, dJ, dB, deps, d_diag, dS_old, dS_new,
                                                ctypes.byref(out), ctypes.byref(cnt), stream or None))
    return out.value, int(cnt.value)


def lambda_ali_update_native_dev(sites: VoronoiSites, nlam: int, dJ_up: int, dJ_down: int, dB_up: int, deps: int,
                                 d_diag_up: int, dS_up: int, dS_down: int, stream: int = 0):
    """`lambda_ali_update_dev` on sweep-order plane sets (`vrt_lambda_ali_update_native_dev`): Λ* as an up-order plane
    set like B."""
    out, cnt = ctypes.c_double(), ctypes.c_int64()
    check(_lib.load().vrt_lambda_ali_update_native_dev(sites.handle, nlam, dJ_up or None, dJ_down or None, dB_up, deps,
                                                       d_diag_up, dS_up, dS_down, ctypes.byref(out), ctypes.byref(cnt),
                                                       stream or None))
    return out.value, int(cnt.value)


def rates_populations_native_dev(sites: VoronoiSites, lam, blocks, dJ_up: int, dJ_down: int, planck2, lambda0: float, c0: float,
                                 d_doppler: int, d_gamma: int, sigma_bb_const: float, sigma_bf1, sigma_bf2,
                                 d_temperature: int, d_lte: int, hc_over_kB: float, pref_ij: float, pref_ji: float,
                                 d_C: int, d_atom_density: int, d_R: int, d_populations: int, stream: int = 0) -> None:
    """`rates_populations_dev` with J read from the sweep-order plane sets of both directions."""
    lam, planck2 = _f64(lam), _f64(planck2)
    blocks = np.ascontiguousarray(blocks, dtype=np.int64)
    s1, s2 = _f64(sigma_bf1), _f64(sigma_bf2)
    check(_lib.load().vrt_rates_populations_native_dev(sites.handle, lam.size, _d(lam), _i(blocks), dJ_up or None, dJ_down or None,
                                                       _d(planck2), float(lambda0), float(c0), d_doppler, d_gamma,
                                                       float(sigma_bb_const), _d(s1), _d(s2), d_temperature, d_lte,
                                                       float(hc_over_kB), float(pref_ij), float(pref_ji), d_C, d_atom_density,
                                                       d_R, d_populations, stream or None))


def lambda_update_native_dev_f32(plan: "FormalPlan", nlam: int, dJ_up: int, dJ_down: int, dB_up: int, deps: int, dS_up: int,
                                 dS_down: int, stream: int = 0) -> float:
    """`lambda_update_native_dev` on the plan's float32 plane sets (`vrt_lambda_update_native_dev_f32`; ε stays float64):
    J = f32(J_up + J_down), S_new = f32((1 - ε) J + ε B), the criterion from the stored float32 values."""
    out = ctypes.c_double()
    check(_lib.load().vrt_lambda_update_native_dev_f32(plan._h, nlam, dJ_up or None, dJ_down or None, dB_up, deps, dS_up,
                                                       dS_down, ctypes.byref(out), stream or None))
    return out.value


def rates_populations_native_dev_f32(plan: "FormalPlan", lam, blocks, dJ_up: int, dJ_down: int, planck2, lambda0: float, c0: float,
                                     d_doppler: int, d_gamma: int, sigma_bb_const: float, sigma_bf1, sigma_bf2,
                                     d_temperature: int, d_lte: int, hc_over_kB: float, pref_ij: float, pref_ji: float,
                                     d_C: int, d_atom_density: int, d_R: int, d_populations: int, stream: int = 0) -> None:
    """`rates_populations_native_dev` with J read from the plan's float32 plane sets (`vrt_rates_populations_native_dev_f32`):
    J = f32(J_up + J_down) widened; R and the populations are float64."""
    lam, planck2 = _f64(lam), _f64(planck2)
    blocks = np.ascontiguousarray(blocks, dtype=np.int64)
    s1, s2 = _f64(sigma_bf1), _f64(sigma_bf2)
    check(_lib.load().vrt_rates_populations_native_dev_f32(plan._h, lam.size, _d(lam), _i(blocks), dJ_up or None, dJ_down or None,
                                                           _d(planck2), float(lambda0), float(c0), d_doppler, d_gamma,
                                                           float(sigma_bb_const), _d(s1), _d(s2), d_temperature, d_lte,
                                                           float(hc_over_kB), float(pref_ij), float(pref_ji), d_C, d_atom_density,
                                                           d_R, d_populations, stream or None))


def _rate_shares(entry, handle, lam, blocks, l0, l1, dJ_up, dJ_down, planck2, lambda0, c0, d_doppler, d_gamma, sigma_bb_const,
                 sigma_bf1, sigma_bf2, d_temperature, d_lte, hc_over_kB, pref_ij, pref_ji, d_shares, stream):
    lam, planck2 = _f64(lam), _f64(planck2)
    blocks = np.ascontiguousarray(blocks, dtype=np.int64)
    s1, s2 = _f64(sigma_bf1), _f64(sigma_bf2)
    check(entry(handle, lam.size, int(l0), int(l1), _d(lam), _i(blocks), dJ_up or None, dJ_down or None, _d(planck2),
                float(lambda0), float(c0), d_doppler, d_gamma, float(sigma_bb_const), _d(s1), _d(s2), d_temperature, d_lte,
                float(hc_over_kB), float(pref_ij), float(pref_ji), d_shares, stream or None))


def rate_shares_native_dev(sites: VoronoiSites, lam, blocks, l0: int, l1: int, dJ_up: int, dJ_down: int, planck2, lambda0: float,
                           c0: float, d_doppler: int, d_gamma: int, sigma_bb_const: float, sigma_bf1, sigma_bf2,
                           d_temperature: int, d_lte: int, hc_over_kB: float, pref_ij: float, pref_ji: float, d_shares: int,
                           stream: int = 0) -> None:
    """The share of the wavelengths [l0, l1) of `lam` in the six rate integrals of every site (`vrt_rate_shares_native_dev`),
    into d_shares (6, n) float64.  dJ_up / dJ_down: float64 sweep-order plane sets of those l1 - l0 wavelengths only
    (wavelength l at local index l - l0).  The shares of a partition of the wavelengths, added, go to
    `populations_from_shares_dev`."""
    _rate_shares(_lib.load().vrt_rate_shares_native_dev, sites.handle, lam, blocks, l0, l1, dJ_up, dJ_down, planck2, lambda0, c0,
                 d_doppler, d_gamma, sigma_bb_const, sigma_bf1, sigma_bf2, d_temperature, d_lte, hc_over_kB, pref_ij, pref_ji,
                 d_shares, stream)


def rate_shares_native_dev_f32(plan: "FormalPlan", lam, blocks, l0: int, l1: int, dJ_up: int, dJ_down: int, planck2,
                               lambda0: float, c0: float, d_doppler: int, d_gamma: int, sigma_bb_const: float, sigma_bf1,
                               sigma_bf2, d_temperature: int, d_lte: int, hc_over_kB: float, pref_ij: float, pref_ji: float,
                               d_shares: int, stream: int = 0) -> None:
    """`rate_shares_native_dev` with J read from float32 plane sets of l1 - l0 wavelengths in the plan's float layout
    (`vrt_rate_shares_native_dev_f32`): J = f32(J_up + J_down) widened; the shares are float64."""
    _rate_shares(_lib.load().vrt_rate_shares_native_dev_f32, plan._h, lam, blocks, l0, l1, dJ_up, dJ_down, planck2, lambda0, c0,
                 d_doppler, d_gamma, sigma_bb_const, sigma_bf1, sigma_bf2, d_temperature, d_lte, hc_over_kB, pref_ij, pref_ji,
                 d_shares, stream)


def populations_from_shares_dev(n: int, d_shares: int, d_C: int, d_atom_density: int, d_R: int, d_populations: int,
                                stream: int = 0) -> None:
    """R (n, 3, 3) and the populations (3, n) of every site from the summed shares (6, n) of `rate_shares_native_dev[_f32]`
    (`vrt_populations_from_shares_dev`), on the current device."""
    check(_lib.load().vrt_populations_from_shares_dev(int(n), d_shares, d_C, d_atom_density, d_R, d_populations, stream or None))


def rates_populations_dev(sites: VoronoiSites, lam, blocks, ld: int, dJ: int, planck2, lambda0: float, c0: float,
                          d_doppler: int, d_gamma: int, sigma_bb_const: float, sigma_bf1, sigma_bf2,
                          d_temperature: int, d_lte: int, hc_over_kB: float, pref_ij: float, pref_ji: float,
                          d_C: int, d_atom_density: int, d_R: int, d_populations: int, stream: int = 0) -> None:
    """Device-resident rates + populations epilogue (`vrt_rates_populations_dev`): calculate_R
    (src/rates.jl:154-201) and get_revised_populations (src/populations.jl:191-221) from J in place."""
    lam, planck2 = _f64(lam), _f64(planck2)
    blocks = np.ascontiguousarray(blocks, dtype=np.int64)
    s1, s2 = _f64(sigma_bf1), _f64(sigma_bf2)
    check(_lib.load().vrt_rates_populations_dev(sites.handle, lam.size, ld, _d(lam), _i(blocks), dJ, _d(planck2),
                                                float(lambda0), float(c0), d_doppler, d_gamma, float(sigma_bb_const),
                                                _d(s1), _d(s2), d_temperature, d_lte, float(hc_over_kB),
                                                float(pref_ij), float(pref_ji), d_C, d_atom_density, d_R,
                                                d_populations, stream or None))


def line_terms_dev(sites: VoronoiSites, d_gamma_static: int, d_gamma_unsold: int, d_populations: int,
                   strength_const: float, Bij: float, Bji: float, d_gamma: int = 0, d_line_strength: int = 0,
                   stream: int = 0) -> None:
    """γ of the current populations (γ_constant, src/broadening.jl:63-82, as J_λ_voronoi evaluates it every
    iteration, lambda_iteration.jl:72-75) and the λ-independent factor of αline_λ (src/line.jl:219-225), on the
    device (`vrt_line_terms_dev`; device pointers)."""
    check(_lib.load().vrt_line_terms_dev(sites.handle, d_gamma_static or None, d_gamma_unsold or None, d_populations,
                                         float(strength_const), float(Bij), float(Bji), d_gamma or None,
                                         d_line_strength or None, stream or None))


# ---- the Λ-iteration driver, device-resident (src/lambda_iteration.jl:205-300, Λ_voronoi) -------------
class LineCase:
    """The per-site inputs Λ_voronoi derives before its loop (LTE populations, α_cont, B_0, ε, C; through
    Transparency.jl, which is outside this path) plus the line's constants, as plain numbers in ONE unit
    system.  Arrays: `lam` (nλ,) all wavelengths (bound-bound block first, then the two bound-free
    blocks; `blocks` = their six [lo, hi) offsets), `velocity` (n, 3) [z, x, y], `doppler`, `alpha_cont`,
    `eps`, `temperature`, `atom_density` (n,), `B0` (n, nλ), `lte` (3, n), `C` (n, 3, 3), `planck2` (nλ,),
    `sigma_bf1`, `sigma_bf2` (one per wavelength of their block).  γ_constant (src/broadening.jl:63-82) is
    `gamma_static` + `gamma_unsold` (n_1 + n_2): the natural + Stark widths, fixed per site, and the van der
    Waals width per unit neutral-hydrogen density, which follows the populations every iteration."""
    FIELDS = ("lam", "blocks", "lambda0", "c0", "velocity", "doppler", "gamma_static", "gamma_unsold", "alpha_cont", "eps",
              "temperature", "atom_density", "B0", "lte", "C", "planck2", "sigma_bf1", "sigma_bf2", "strength_const", "Bij",
              "Bji", "sigma_bb_const", "hc_over_kB", "pref_ij", "pref_ji")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw.pop(k))
        if kw:
            raise TypeError(f"unexpected fields {sorted(kw)}")

    def gamma(self, populations) -> np.ndarray:
        """γ_constant for populations (3, n)"""
        pops = np.asarray(populations)
        return np.asarray(self.gamma_static) + np.asarray(self.gamma_unsold) * (pops[0] + pops[1])

    def c_struct(self):
        """(vrt_line_case, the arrays it points into) for the host-pointer entry points"""
        keep = {k: _f64(getattr(self, k)) for k in ("lam", "velocity", "doppler", "gamma_static", "gamma_unsold", "alpha_cont",
                                                   "eps", "temperature", "atom_density", "B0", "lte", "C", "planck2",
                                                   "sigma_bf1", "sigma_bf2")}
        lc = _lib.LineCaseStruct()
        lc.nlam = keep["lam"].size
        lc.lambda_ = _d(keep["lam"])
        for q, v in enumerate(np.asarray(self.blocks, dtype=np.int64).reshape(6)):
            lc.blocks[q] = int(v)
        lc.lambda0, lc.c0 = float(self.lambda0), float(self.c0)
        for cname, k in (("velocity", "velocity"), ("doppler_width", "doppler"), ("gamma_static", "gamma_static"),
                         ("gamma_unsold", "gamma_unsold"), ("alpha_cont", "alpha_cont"), ("eps", "eps"),
                         ("temperature", "temperature"), ("atom_density", "atom_density"), ("B0", "B0"),
                         ("lte_populations", "lte"), ("C", "C"), ("planck2", "planck2"), ("sigma_bf1", "sigma_bf1"),
                         ("sigma_bf2", "sigma_bf2")):
            setattr(lc, cname, _d(keep[k]))
        for k in ("strength_const", "Bij", "Bji", "sigma_bb_const", "hc_over_kB", "pref_ij", "pref_ji"):
            setattr(lc, k, float(getattr(self, k)))
        return lc, keep


# ---- resuming a line Λ-iteration: the state is (S, populations) (src/recover_simulation.jl; vrt_*_lambda_set_state) ----
CHECKPOINT_KEYS = ("S", "populations", "iterate", "history")


def write_checkpoint(path, S, populations, iterate: int, history) -> None:
    """The checkpoint of a line Λ-iteration as an .npz with the keys `S` (n, nλ), `populations` (3, n), `iterate` (the
    number of iterates done in total) and `history` (every scalar so far).  Written under a temporary name in the
    directory of `path` and moved over it with os.replace: a run killed in between leaves the previous file whole."""
    path = os.fspath(path)
    tmp = f"{path}.{os.getpid()}.tmp.npz"          # (numpy appends .npz to a name that does not end in it)
    try:
        np.savez(tmp, S=_f64(S), populations=_f64(populations), iterate=np.int64(iterate), history=_f64(history).reshape(-1))
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def _check_state_shapes(S, populations, n: int, nlam: int, who: str):
    """S (n, nλ) and populations (3, n) as contiguous float64 (None stays None); ValueError for any other shape"""
    if S is not None:
        S = _f64(S)
        if S.shape != (n, nlam):
            raise ValueError(f"{who}: S has shape {S.shape}, the case needs {(n, nlam)}")
    if populations is not None:
        populations = _f64(populations)
        if populations.shape != (3, n):
            raise ValueError(f"{who}: the populations have shape {populations.shape}, the case needs {(3, n)}")
    return S, populations


def read_checkpoint(path, n: int | None = None, nlam: int | None = None) -> dict:
    """The four keys of `write_checkpoint` (S, populations as float64 arrays, iterate as int, history as a list).  With
    n and nλ given, a file whose shapes do not match them raises ValueError."""
    with np.load(os.fspath(path)) as f:
        missing = [k for k in CHECKPOINT_KEYS if k not in f.files]
        if missing:
            raise ValueError(f"{path}: not a Λ-iteration checkpoint, no {missing}")
        S, pops = _f64(f["S"]), _f64(f["populations"])
        iterate, history = int(f["iterate"]), [float(v) for v in np.asarray(f["history"]).reshape(-1)]
    if S.ndim != 2 or pops.shape != (3, S.shape[0]):
        raise ValueError(f"{path}: S {S.shape} and populations {pops.shape} are not (n, nλ) and (3, n)")
    if n is not None and nlam is not None:
        _check_state_shapes(S, pops, n, nlam, os.fspath(path))
    return {"S": S, "populations": pops, "iterate": iterate, "history": history}


def _start_state(S0, populations0, resume, checkpoint_every, n: int, nlam: int, who: str):
    """What a session-backed driver starts from, checked before any device work: (S0, populations0, iterate0, history0)"""
    if int(checkpoint_every) < 1:
        raise ValueError(f"{who}: checkpoint_every must be >= 1")
    if resume is None:
        S0, populations0 = _check_state_shapes(S0, populations0, n, nlam, who)
        return S0, populations0, 0, []
    if S0 is not None or populations0 is not None:
        raise ValueError(f"{who}: give either resume or S0 / populations0")
    ck = read_checkpoint(resume, n, nlam)
    return ck["S"], ck["populations"], ck["iterate"], ck["history"]


def _session_loop(L, prefix: str, h, n: int, nlam: int, eps_conv: float, maxiter: int, start, checkpoint, checkpoint_every: int,
                  ng, who: str):
    """The loop every session-backed line driver runs on its session `h` (vrt_<prefix>_iterate / _get / _set_state):
    returns (J, S, populations, history, steps, new iterates)."""
    fn = lambda name: getattr(L, f"vrt_{prefix}_{name}")
    S0, pops0, iterate0, history0 = start
    if S0 is not None or pops0 is not None:
        check(fn("set_state")(h, _d(S0), _d(pops0)))
    history, steps, i = list(history0), [], 0
    diff = history[-1] if history else 1.0                 # criterion(S_new = B, S_old = 0) = 1
    S, pops = np.zeros((n, nlam)), np.zeros((3, n))

    def save():
        check(fn("get")(h, None, _d(S), _d(pops), None, None))       # (J, R and γ are not part of the state)
        write_checkpoint(checkpoint, S, pops, iterate0 + i, history)

    saved = -1
    while diff > eps_conv and i < maxiter:
        d = ctypes.c_double()
        check(fn("iterate")(h, ctypes.byref(d)))
        diff = d.value
        history.append(diff)
        i += 1
        if ng is not None:
            _ng_last(fn("last_acceleration"), h, i, steps)
        if checkpoint is not None and i % int(checkpoint_every) == 0:
            save()
            saved = i
        if diff != diff:
            import warnings
            warnings.warn(f"{who}: NaN DIFF! at iteration {i} -- stopping, results are not converged")
    if checkpoint is not None and i > 0 and saved != i:
        save()
    J = np.zeros((n, nlam))
    check(fn("get")(h, _d(J), _d(S), _d(pops), None, None))
    return J, S, pops, history, steps, i


def _quadrature_plan(sites: VoronoiSites, quadrature: str, n_sweeps: int):
    w, th, ph, _ = read_quadrature(quadrature)
    key = (os.path.basename(quadrature), int(n_sweeps))
    plan = sites._plans.get(key)
    if plan is None:
        dirs = [1 if t > 90 else (-1 if t < 90 else 0) for t in th]
        plan = FormalPlan(sites, quadrature_directions(th, ph), n_sweeps, dirs=dirs)
        sites._plans[key] = plan
    return plan, w


def J_lambda_voronoi_line(S_lambda, populations, sites: VoronoiSites, case: LineCase, quadrature: str,
                          n_sweeps: int = 3) -> np.ndarray:
    """J_λ_voronoi, line method (src/lambda_iteration.jl:60-113), from HOST arrays through ONE call
    (`vrt_plan_execute_line`): γ and the line strength of `populations` (3, n), α_tot of every angle made on the
    device, I_0 = B_0 of the bottom layer for the up rays (:99-101), zeros for the down rays (:105-106)."""
    plan, w = _quadrature_plan(sites, quadrature, n_sweeps)
    S = _f64(S_lambda)
    n, nlam = S.shape
    pops = np.asarray(populations)
    gamma = _f64(case.gamma(pops))
    strength = _f64(case.strength_const * (pops[0] * case.Bij - pops[1] * case.Bji))
    lam, vel, dop, ac = _f64(case.lam), _f64(case.velocity), _f64(case.doppler), _f64(case.alpha_cont)
    n1 = int(sites.layers_up[1] - 1)
    I0 = _f64(np.asarray(case.B0)[sites.perm_up[:n1] - 1])
    J = np.zeros((n, nlam))
    check(_lib.load().vrt_plan_execute_line(plan._h, nlam, nlam, _d(lam), float(case.lambda0), float(case.c0), _d(vel),
                                            _d(dop), _d(gamma), _d(strength), _d(ac), _d(S), _d(I0), None, _d(_f64(w)),
                                            _d(J)))
    return J


def _storage_f32(storage, who: str) -> bool:
    if storage not in ("f64", "f32"):
        raise ValueError(f"{who}: storage must be 'f64' or 'f32'")
    return storage == "f32"


def _line_operator(operator, f32: bool, who: str) -> bool:
    """operator=None | "diagonal" of the line drivers, checked before any device work"""
    if operator not in _OPERATORS:
        raise ValueError(f"{who}: operator must be None or 'diagonal'")
    if operator is not None and f32:
        raise ValueError(f"{who}: operator='diagonal' is not available with storage='f32' (the ALI update works on float64 arrays)")
    return operator is not None


def _Lambda_voronoi_native(eps_conv: float, maxiter: int, sites: VoronoiSites, case: LineCase, quadrature: str, n_sweeps: int,
                           S0=None, populations0=None, f32: bool = False, ali: bool = False):
    import torch
    vt = torch.float32 if f32 else torch.float64                # what S, J, B, I_0 and α are stored as
    w, th, ph, nq = read_quadrature(quadrature)
    dev = torch.device("cuda", sites.device)
    n, nlam = sites.n, int(np.asarray(case.lam).size)
    plan = FormalPlan(sites, quadrature_directions(th, ph), n_sweeps, dirs=[1 if t > 90 else (-1 if t < 90 else 0) for t in th])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    d_vel, d_dop, d_gs, d_gu, d_ac, d_eps, d_T = (t(getattr(case, k)) for k in
                                                  ("velocity", "doppler", "gamma_static", "gamma_unsold", "alpha_cont", "eps",
                                                   "temperature"))
    d_B, d_lte, d_C, d_atom = t(case.B0), t(case.lte), t(case.C), t(case.atom_density)
    pops = d_lte.clone() if populations0 is None else t(populations0)
    d_S0 = d_B if S0 is None else t(S0)
    d_Bv, d_S0v = d_B.to(vt), d_S0.to(vt)
    st = torch.cuda.current_stream().cuda_stream
    cnt = plan.native_plane_count(nlam)
    S_up, S_dn, B_up, J_up, J_dn = (torch.zeros(cnt, dtype=vt, device=dev) for _ in range(5))
    plan.to_native_dev(nlam, nlam, d_S0v.data_ptr(), S_up.data_ptr(), S_dn.data_ptr(), stream=st, f32=f32)     # S_new = B_0 (or S0)
    plan.to_native_dev(nlam, nlam, d_Bv.data_ptr(), B_up.data_ptr(), 0, stream=st, f32=f32)
    native = torch.empty(plan.native_alpha_count(nlam), dtype=vt, device=dev)
    d_R = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
    d_gam, strength = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    n1 = int(sites.layers_up[1] - 1)
    I0_up = d_Bv[torch.as_tensor(sites.perm_up[:n1] - 1, device=dev)].contiguous()
    update, rates, owner = ((lambda_update_native_dev_f32, rates_populations_native_dev_f32, plan) if f32 else
                            (lambda_update_native_dev, rates_populations_native_dev, sites))
    if ali:                                                     # Λ* of every iterate's α: rows, then its up-order plane set
        L_rows, L_up = torch.zeros((n, nlam), dtype=vt, device=dev), torch.zeros(cnt, dtype=vt, device=dev)
    history = []
    diff, i = 1.0, 0
    try:
        while diff > eps_conv and i < maxiter:
            line_terms_dev(sites, d_gs.data_ptr(), d_gu.data_ptr(), pops.data_ptr(), case.strength_const, case.Bij, case.Bji,
                           d_gam.data_ptr(), strength.data_ptr(), stream=st)
            plan.line_opacity_dev(case.lam, case.lambda0, case.c0, d_vel.data_ptr(), d_dop.data_ptr(), d_gam.data_ptr(),
                                  strength.data_ptr(), d_ac.data_ptr(), native.data_ptr(), stream=st, f32=f32)
            plan.execute_native_dev(nlam, S_up.data_ptr(), S_dn.data_ptr(), native.data_ptr(), _lib.ALPHA_ANGLE_NATIVE, w,
                                    dJ_up=J_up.data_ptr(), dJ_down=J_dn.data_ptr(), dI0_up=I0_up.data_ptr(), stream=st, f32=f32)
            if ali:
                plan.line_lambda_diagonal_dev(nlam, native.data_ptr(), w, nlam, L_rows.data_ptr(), stream=st)
                plan.to_native_dev(nlam, nlam, L_rows.data_ptr(), L_up.data_ptr(), 0, stream=st)
                diff, _ = lambda_ali_update_native_dev(sites, nlam, J_up.data_ptr(), J_dn.data_ptr(), B_up.data_ptr(),
                                                       d_eps.data_ptr(), L_up.data_ptr(), S_up.data_ptr(), S_dn.data_ptr(),
                                                       stream=st)
            else:
                diff = update(owner, nlam, J_up.data_ptr(), J_dn.data_ptr(), B_up.data_ptr(), d_eps.data_ptr(),
                              S_up.data_ptr(), S_dn.data_ptr(), stream=st)
            new_pops = torch.empty_like(pops)
            rates(owner, case.lam, case.blocks, J_up.data_ptr(), J_dn.data_ptr(), case.planck2, case.lambda0,
                  case.c0, d_dop.data_ptr(), d_gam.data_ptr(), case.sigma_bb_const, case.sigma_bf1,
                  case.sigma_bf2, d_T.data_ptr(), d_lte.data_ptr(), case.hc_over_kB, case.pref_ij,
                  case.pref_ji, d_C.data_ptr(), d_atom.data_ptr(), d_R.data_ptr(), new_pops.data_ptr(), stream=st)
            pops = new_pops
            history.append(diff)
            i += 1
            if diff != diff:
                import warnings
                warnings.warn(f"Lambda_voronoi: NaN DIFF! at iteration {i} -- stopping, results are not converged")
        J, S = torch.zeros((n, nlam), dtype=vt, device=dev), torch.zeros((n, nlam), dtype=vt, device=dev)
        plan.J_from_native_dev(nlam, nlam, J_up.data_ptr(), J_dn.data_ptr(), J.data_ptr(), stream=st, f32=f32)
        plan.from_native_dev(1, nlam, nlam, S_up.data_ptr(), S.data_ptr(), stream=st, f32=f32)
        torch.cuda.synchronize()
        plan.check()
        return J.double().cpu().numpy(), S.double().cpu().numpy(), pops.cpu().numpy(), history
    finally:
        plan.close()


def Lambda_voronoi_host(eps_conv: float, maxiter: int, sites: VoronoiSites, case: LineCase, quadrature: str,
                        n_sweeps: int = 3, ng=None, S0=None, populations0=None, checkpoint=None, checkpoint_every: int = 1,
                        resume=None, storage: str = "f64", operator=None):
    """Λ_voronoi (src/lambda_iteration.jl:205-300) for a host WITHOUT device arrays: the library owns the device
    state (`vrt_lambda_create` / `_iterate` / `_get`), one call per iteration, only the criterion's scalar
    comes back inside the loop.  Returns (J, S_new, populations (3, n), history).
    ng=(start, period): second-order Ng acceleration inside the session (`vrt_lambda_set_acceleration`), the first
    step after iterate `start`, then every `period` iterates (both >= 4); the tuple gains a fifth element, the list of
    (iterate, applied, a, b) of every due step.
    S0 (n, nλ), populations0 (3, n): start from this state instead of LTE with S = B_0 (`vrt_lambda_set_state`, the
    reference's recover_voronoi); either alone replaces that half.  The run continues bit for bit as the one that
    produced them.  checkpoint="run.npz": `write_checkpoint` after every `checkpoint_every`-th iterate and after the
    last.  resume="run.npz": start from such a file; the returned history is the file's followed by the new scalars,
    `maxiter` counts the new iterates; a file whose shapes do not match the case raises ValueError before any device work.
    storage="f32": the session holds S, J, B, I_0 and α as float32 (`vrt_lambda_create_f32`; arithmetic stays float64, the
    patch path only); the returned J and S are float64 arrays of float32-representable values, checkpoints work unchanged,
    and `ng` raises ValueError before any device work (the Ng kernels work on float64 planes).
    operator="diagonal": accelerated Λ-iteration with the diagonal operator Λ* formed from every iterate's α
    (`vrt_lambda_use_operator`): the same fixed point in fewer iterates where ε is small; composes with `ng`,
    checkpoints and `resume` (nothing more is saved: Λ* is a function of the populations).  ValueError with storage="f32"
    before any device work."""
    L = _lib.load()
    f32 = _storage_f32(storage, "Lambda_voronoi_host")
    ali = _line_operator(operator, f32, "Lambda_voronoi_host")
    if f32 and ng is not None:
        raise ValueError("Lambda_voronoi_host: ng is not available with storage='f32'")
    lc, keep = case.c_struct()
    n, nlam = sites.n, int(keep["lam"].size)
    start = _start_state(S0, populations0, resume, checkpoint_every, n, nlam, "Lambda_voronoi_host")
    plan, w = _quadrature_plan(sites, quadrature, n_sweeps)
    h = ctypes.c_void_p()
    check((L.vrt_lambda_create_f32 if f32 else L.vrt_lambda_create)(plan._h, ctypes.byref(lc), _d(_f64(w)), ctypes.byref(h)))
    try:
        if ng is not None:
            check(L.vrt_lambda_set_acceleration(h, 2, *_ng_settings(ng)))
        if ali:
            check(L.vrt_lambda_use_operator(h, 1))
        J, S, pops, history, steps, i = _session_loop(L, "lambda", h, n, nlam, eps_conv, maxiter, start, checkpoint,
                                                      checkpoint_every, ng, "Lambda_voronoi_host")
        if i == 0:
            S[:] = keep["B0"] if start[0] is None else start[0]
            if f32:
                S[:] = S.astype(np.float32)
            pops[:] = keep["lte"] if start[1] is None else start[1]
        return (J, S, pops, history) if ng is None else (J, S, pops, history, steps)
    finally:
        L.vrt_lambda_destroy(h)


def Lambda_voronoi(eps_conv: float, maxiter: int, sites: VoronoiSites, case: LineCase, quadrature: str,
                   n_sweeps: int = 3, native: bool = False, S0=None, populations0=None, storage: str = "f64", operator=None):
    """Λ_voronoi (src/lambda_iteration.jl:205-300) with everything between two convergence checks on
    the device, over the device-pointer entry points: per iteration `vrt_line_terms_dev` (γ and the line
    strength of the current populations, :72-75), `vrt_line_opacity_dev` (α_tot of every angle, :72-96),
    `vrt_plan_execute_dev` (J_λ, :84-111), `vrt_lambda_update_dev` (S_new and the criterion's scalar, :261-263,
    :325-349) and `vrt_rates_populations_dev` (:269, :274); only that scalar crosses PCIe inside the loop.
    Starts in LTE with S = B_0 like the reference.
    native=True: S and J stay in the sweep's own per-direction plane sets between the steps
    (`vrt_plan_execute_native_dev`, `vrt_lambda_update_native_dev`, `vrt_rates_populations_native_dev`): no layout
    change inside the loop, the same results bit for bit.
    S0 (n, nλ), populations0 (3, n): the loop starts from them instead (S finite and > 0, populations finite and >= 0;
    ValueError otherwise) and continues bit for bit as the run that produced them.
    storage="f32" (with native=True; ValueError otherwise): the plane sets, I_0 and α are float32 torch tensors and the loop
    runs the `_f32` entry points (`vrt_line_opacity_dev_f32`, `vrt_plan_execute_native_dev_f32`,
    `vrt_lambda_update_native_dev_f32`, `vrt_rates_populations_native_dev_f32`); J and S come back as float64 arrays of
    float32-representable values, the same as `Lambda_voronoi_host(storage="f32")` bit for bit.
    operator="diagonal" (both `native` forms; ValueError with storage="f32"): per iteration also
    `vrt_line_lambda_diagonal_dev` (Λ* from the α just written) and `vrt_lambda_ali_update_dev` /
    `vrt_lambda_ali_update_native_dev` in place of the plain update -- `Lambda_voronoi_host(operator="diagonal")` bit for bit.
    Returns (J, S_new, populations (3, n), history of the criterion's differences) as numpy arrays."""
    import torch
    f32 = _storage_f32(storage, "Lambda_voronoi")
    if f32 and not native:
        raise ValueError("Lambda_voronoi: storage='f32' needs native=True (the float loop runs on sweep-order plane sets)")
    ali = _line_operator(operator, f32, "Lambda_voronoi")
    S0, populations0 = _check_state_shapes(S0, populations0, sites.n, int(np.asarray(case.lam).size), "Lambda_voronoi")
    if S0 is not None and not (np.isfinite(S0).all() and (S0 > 0).all()):
        raise ValueError("Lambda_voronoi: S0 must be finite and > 0 everywhere")
    if populations0 is not None and not (np.isfinite(populations0).all() and (populations0 >= 0).all()):
        raise ValueError("Lambda_voronoi: populations0 must be finite and >= 0 everywhere")
    if native:
        return _Lambda_voronoi_native(eps_conv, maxiter, sites, case, quadrature, n_sweeps, S0, populations0, f32, ali)
    w, th, ph, nq = read_quadrature(quadrature)
    dev = torch.device("cuda", sites.device)
    n, nlam = sites.n, int(np.asarray(case.lam).size)
    plan = FormalPlan(sites, quadrature_directions(th, ph), n_sweeps, dirs=[1 if t > 90 else (-1 if t < 90 else 0) for t in th])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    d_vel, d_dop, d_gs, d_gu, d_ac, d_eps, d_T = (t(getattr(case, k)) for k in
                                                  ("velocity", "doppler", "gamma_static", "gamma_unsold", "alpha_cont", "eps",
                                                   "temperature"))
    d_B, d_lte, d_C, d_atom = t(case.B0), t(case.lte), t(case.C), t(case.atom_density)
    pops = d_lte.clone() if populations0 is None else t(populations0)       # populations = copy(LTE_pops)
    S_new, S_old, J = d_B.clone() if S0 is None else t(S0), torch.zeros_like(d_B), torch.zeros_like(d_B)
    native = torch.empty(plan.native_alpha_count(nlam), dtype=torch.float64, device=dev)
    d_R = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
    d_gam, strength = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    n1 = int(sites.layers_up[1] - 1)
    bottom = torch.as_tensor(sites.perm_up[:n1] - 1, device=dev)
    I0_up = d_B[bottom].contiguous()                           # B_λ(λ_l, T) of the bottom layer, :99-101
    d_L = torch.zeros_like(d_B) if ali else None               # Λ* of every iterate's α
    st = torch.cuda.current_stream().cuda_stream
    history = []
    diff, i = 1.0, 0                                           # criterion(S_new = B, S_old = 0) = |1 - 0/B| = 1
    try:
        while diff > eps_conv and i < maxiter:                 # criterion, :325-349
            S_old.copy_(S_new)
            # γ_constant of the current populations (:72-75) and αline_λ's population factor (src/line.jl:219-225)
            line_terms_dev(sites, d_gs.data_ptr(), d_gu.data_ptr(), pops.data_ptr(), case.strength_const, case.Bij, case.Bji,
                           d_gam.data_ptr(), strength.data_ptr(), stream=st)
            plan.line_opacity_dev(case.lam, case.lambda0, case.c0, d_vel.data_ptr(), d_dop.data_ptr(), d_gam.data_ptr(),
                                  strength.data_ptr(), d_ac.data_ptr(), native.data_ptr(), stream=st)
            plan.execute_dev(nlam, nlam, S_old.data_ptr(), native.data_ptr(), _lib.ALPHA_ANGLE_NATIVE, w,
                             dJ=J.data_ptr(), dI0_up=I0_up.data_ptr(), stream=st)
            if ali:
                plan.line_lambda_diagonal_dev(nlam, native.data_ptr(), w, nlam, d_L.data_ptr(), stream=st)
                diff, _ = lambda_ali_update_dev(sites, nlam, nlam, J.data_ptr(), d_B.data_ptr(), d_eps.data_ptr(), d_L.data_ptr(),
                                                S_old.data_ptr(), S_new.data_ptr(), stream=st)
            else:
                diff = lambda_update_dev(sites, nlam, nlam, J.data_ptr(), d_B.data_ptr(), d_eps.data_ptr(), S_old.data_ptr(),
                                         S_new.data_ptr(), stream=st)
            new_pops = torch.empty_like(pops)
            rates_populations_dev(sites, case.lam, case.blocks, nlam, J.data_ptr(), case.planck2, case.lambda0, case.c0,
                                  d_dop.data_ptr(), d_gam.data_ptr(), case.sigma_bb_const, case.sigma_bf1, case.sigma_bf2,
                                  d_T.data_ptr(), d_lte.data_ptr(), case.hc_over_kB, case.pref_ij, case.pref_ji,
                                  d_C.data_ptr(), d_atom.data_ptr(), d_R.data_ptr(), new_pops.data_ptr(), stream=st)
            pops = new_pops
            history.append(diff)
            i += 1
            if diff != diff:                                   # the reference prints "NaN DIFF!" (:336-338); its
                import warnings                                # NaN diff then ends the loop (NaN > ϵ is false)
                warnings.warn(f"Lambda_voronoi: NaN DIFF! at iteration {i} -- stopping, results are not converged")
        torch.cuda.synchronize()
        return J.cpu().numpy(), S_new.cpu().numpy(), pops.cpu().numpy(), history
    finally:
        plan.close()


# ---- the line Λ-iteration on the regular grid (src/lambda_iteration.jl:1-58 J_λ_regular, :116-205 Λ_regular) ----------
def _regular_directions(quadrature: str):
    """weights, k (n_angles, 3) and dirs (1 up for θ > 90, -1 down for θ < 90, 0 for θ = 90, which adds nothing)"""
    w, th, ph, _ = read_quadrature(quadrature)
    dirs = np.ascontiguousarray([1 if t > 90 else (-1 if t < 90 else 0) for t in th], dtype=np.int32)
    return _f64(w), _f64(quadrature_directions(th, ph)), dirs


def _regular_solver(z, x, y, n: int, device: int) -> RegularSolver:
    solver = RegularSolver(z, x, y, device=device)
    if solver.nz * solver.nx * solver.ny != n:
        solver.close()
        raise ValueError(f"the line case has {n} points, the raster nz nx ny = {solver.nz * solver.nx * solver.ny}")
    return solver


def J_lambda_regular_line(S, populations, z, x, y, case: LineCase, quadrature: str, n_sweeps: int = 3,
                          device: int = 0) -> np.ndarray:
    """J_λ_regular, line method (src/lambda_iteration.jl:1-58), from HOST arrays through ONE call
    (`vrt_regular_execute_line`).  z, x, y are the raster's axes with the periodic ghost border, and every one of its
    n = nz nx ny points is a point of `case` (LineCase, Julia point order i = iz + nz (ix + nx iy), i.e. numpy
    (ny, nx, nz) C-order flattened).  S (n, nλ); γ and the line strength from `populations` (3, n); α_tot of every
    angle made on the device; I_0 = B_0's bottom plane for the up rays (:38), zeros for the down rays."""
    S = _f64(S)
    n, nlam = S.shape
    w, k, dirs = _regular_directions(quadrature)
    pops = np.asarray(populations)
    gamma = _f64(case.gamma(pops))
    strength = _f64(case.strength_const * (pops[0] * case.Bij - pops[1] * case.Bji))
    lam, vel, dop, ac = _f64(case.lam), _f64(case.velocity), _f64(case.doppler), _f64(case.alpha_cont)
    solver = _regular_solver(z, x, y, n, device)
    try:
        # B_0's bottom plane as I_0 (nx, ny, nλ) Julia order = numpy (nλ, ny, nx)
        I0 = _f64(np.asarray(case.B0).reshape(solver.ny, solver.nx, solver.nz, nlam)[:, :, 0, :].transpose(2, 0, 1))
        J = np.zeros((n, nlam))
        check(_lib.load().vrt_regular_execute_line(solver._h, k.shape[0], _d(k), dirs.ctypes.data_as(_lib.p_int), _d(w), nlam,
                                                   _d(lam), float(case.lambda0), float(case.c0), _d(vel), _d(dop), _d(gamma),
                                                   _d(strength), _d(ac), _d(S), _d(I0), int(n_sweeps), _d(J)))
        return J
    finally:
        solver.close()


def Lambda_regular(eps_conv: float, maxiter: int, z, x, y, case: LineCase, quadrature: str, n_sweeps: int = 3,
                   device: int = 0, ng=None, S0=None, populations0=None, checkpoint=None, checkpoint_every: int = 1,
                   resume=None, operator=None):
    """Λ_regular (src/lambda_iteration.jl:116-205) with library-owned device state (`vrt_regular_lambda_create` /
    `_iterate` / `_get`): one call per iteration, only the criterion's scalar comes back inside the loop.  The raster
    and `case` as for `J_lambda_regular_line`; every point, ghost border included, is a point of the loop.  Starts
    in LTE with S = B_0; stops like `Lambda_voronoi_host` (criterion, NaN).  Returns (J, S_new, populations (3, n),
    history); ng=(start, period) as for `Lambda_voronoi_host` (`vrt_regular_lambda_set_acceleration`), with the list of
    (iterate, applied, a, b) as a fifth element.  S0, populations0, checkpoint, checkpoint_every, resume as for
    `Lambda_voronoi_host` (`vrt_regular_lambda_set_state`, the reference's recover_regular).
    operator="diagonal": accelerated Λ-iteration with the raster's one-sweep diagonal Λ* formed from every iterate's
    per-angle α (`vrt_regular_lambda_use_operator`; `line_lambda_diagonal_regular` returns such a Λ*), as
    `Lambda_voronoi_host(operator="diagonal")` on the other grid; composes with `ng`, checkpoints and `resume`."""
    ali = _line_operator(operator, False, "Lambda_regular")
    L = _lib.load()
    w, k, dirs = _regular_directions(quadrature)
    lc, keep = case.c_struct()
    nlam = int(keep["lam"].size)
    n = int(keep["doppler"].size)
    start = _start_state(S0, populations0, resume, checkpoint_every, n, nlam, "Lambda_regular")
    solver = _regular_solver(z, x, y, n, device)
    h = ctypes.c_void_p()
    try:
        check(L.vrt_regular_lambda_create(solver._h, k.shape[0], _d(k), dirs.ctypes.data_as(_lib.p_int), _d(w),
                                          ctypes.byref(lc), int(n_sweeps), ctypes.byref(h)))
        if ng is not None:
            check(L.vrt_regular_lambda_set_acceleration(h, 2, *_ng_settings(ng)))
        if ali:
            check(L.vrt_regular_lambda_use_operator(h, 1))
        J, S, pops, history, steps, _ = _session_loop(L, "regular_lambda", h, n, nlam, eps_conv, maxiter, start, checkpoint,
                                                      checkpoint_every, ng, "Lambda_regular")
        return (J, S, pops, history) if ng is None else (J, S, pops, history, steps)
    finally:
        if h:
            L.vrt_regular_lambda_destroy(h)
        solver.close()


# ---- the continuum scattering Λ-iteration on both grids (src/lambda_continuum.jl) -------------------------------------
class ContinuumCase:
    """The inputs Λ_voronoi / Λ_regular of src/lambda_continuum.jl derive before their loop (:116-137, :63-84), as plain
    numbers: `alpha` α_cont = α_s + α_a, `eps` ε = α_a / α_cont and `B0` the Planck function, each (n, nλ) -- or (n,) for
    the reference's single wavelength -- and `eps_thick`: the criterion sees only entries with ε > eps_thick (the
    reference: 1e-4)."""

    def __init__(self, alpha, eps, B0, eps_thick: float = 1e-4):
        two = lambda a: (lambda b: b.reshape(-1, 1) if b.ndim == 1 else b)(_f64(a))
        self.alpha, self.eps, self.B0 = two(alpha), two(eps), two(B0)
        self.eps_thick = float(eps_thick)
        if not (self.alpha.shape == self.eps.shape == self.B0.shape) or self.B0.ndim != 2:
            raise ValueError("ContinuumCase: alpha, eps and B0 must share one (n, nlam) shape")

    @property
    def n(self) -> int:
        return self.B0.shape[0]

    @property
    def nlam(self) -> int:
        return self.B0.shape[1]

    def thick(self) -> np.ndarray:
        return self.eps > self.eps_thick

    def c_struct(self):
        cc = _lib.ContinuumCaseStruct()
        cc.nlam = self.nlam
        cc.alpha, cc.eps, cc.B0 = _d(self.alpha), _d(self.eps), _d(self.B0)
        cc.eps_thick = self.eps_thick
        return cc

    def check(self) -> None:
        """`vrt_continuum_case_check`: raises VrtError for what a session would refuse; needs no device"""
        cc = self.c_struct()
        check(_lib.load().vrt_continuum_case_check(ctypes.byref(cc), self.n))


def continuum_update_dev(sites: VoronoiSites, J, B, eps, S_old, S_new, eps_thick: float = 1e-4, nlam: int | None = None):
    """The masked update of the continuum Λ-iteration (`vrt_continuum_update_dev`) on torch tensors of sites' device,
    each (n, ld) float64 and contiguous: S_new = (1 - ε) J + ε B at every entry of the first `nlam` columns (default:
    all), and the criterion max |1 - S_old/S_new| over the entries with ε > eps_thick (lambda_continuum.jl:148, :188).
    Returns (that maximum -- NaN if a thick entry's term is NaN --, the number of thick entries); synchronises."""
    import torch
    n, ld = S_new.shape
    for t in (J, B, eps, S_old, S_new):
        if t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != (n, ld):
            raise ValueError("continuum_update_dev: contiguous float64 tensors of one (n, ld) shape")
    out, cnt = ctypes.c_double(), ctypes.c_int64()
    st = torch.cuda.current_stream(S_new.device).cuda_stream
    check(_lib.load().vrt_continuum_update_dev(sites.handle, int(ld if nlam is None else nlam), int(ld), J.data_ptr(),
                                               B.data_ptr(), eps.data_ptr(), float(eps_thick), S_old.data_ptr(),
                                               S_new.data_ptr(), ctypes.byref(out), ctypes.byref(cnt), st or None))
    return out.value, int(cnt.value)


def lambda_diagonal(sites: VoronoiSites, alpha, quadrature: str, n_sweeps: int = 3) -> np.ndarray:
    """The diagonal approximate operator Λ* of accelerated Λ-iteration (`vrt_plan_lambda_diagonal`): per (site, wavelength)
    the coefficient of the site's own S in the last Gauss-Seidel visit of every angle of `quadrature`, summed with the
    quadrature weights.  alpha (n,) or (n, nλ), finite and > 0; returns (n, nλ)."""
    alpha = _f64(alpha)
    if alpha.ndim == 1:
        alpha = alpha.reshape(-1, 1)
    if alpha.ndim != 2 or alpha.shape[0] != sites.n:
        raise ValueError(f"lambda_diagonal: alpha must be ({sites.n},) or ({sites.n}, nlam)")
    plan, w = _quadrature_plan(sites, quadrature, n_sweeps)
    diag = np.zeros_like(alpha)
    check(_lib.load().vrt_plan_lambda_diagonal(plan._h, alpha.shape[1], alpha.shape[1], _d(alpha), _d(_f64(w)), _d(diag)))
    return diag


def line_lambda_diagonal(sites: VoronoiSites, alpha_per_angle, quadrature: str, n_sweeps: int = 3) -> np.ndarray:
    """Λ* of the line Λ-iteration (`vrt_line_lambda_diagonal_dev`): `lambda_diagonal` with an α of its own per angle,
    alpha_per_angle (n_angles, n, nλ) in quadrature order (the Doppler-shifted α_tot of the line loop), brought into the
    plan's native per-angle layout on the device.  Every angle of `quadrature` must be active (no θ = 90).  Returns (n, nλ)."""
    import torch
    alpha = _f64(alpha_per_angle)
    plan, w = _quadrature_plan(sites, quadrature, n_sweeps)
    if alpha.ndim != 3 or alpha.shape[0] != len(w) or alpha.shape[1] != sites.n:
        raise ValueError(f"line_lambda_diagonal: alpha_per_angle must be ({len(w)}, {sites.n}, nlam)")
    nlam = alpha.shape[2]
    dev = torch.device("cuda", sites.device)
    d_alpha = torch.from_numpy(alpha).to(dev)
    native = torch.empty(plan.native_alpha_count(nlam), dtype=torch.float64, device=dev)
    diag = torch.zeros((sites.n, nlam), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    plan.alpha_to_native_dev(nlam, nlam, d_alpha.data_ptr(), native.data_ptr(), stream=st)
    plan.line_lambda_diagonal_dev(nlam, native.data_ptr(), w, nlam, diag.data_ptr(), stream=st)
    torch.cuda.synchronize(dev)
    return diag.cpu().numpy()


def continuum_ali_update_dev(sites: VoronoiSites, J, B, eps, diag, S_old, S_new, eps_thick: float = 1e-4,
                             nlam: int | None = None):
    """`continuum_update_dev` with the diagonal operator (`vrt_continuum_ali_update_dev`): with t = 1 - ε,
    S_new = (t (J - Λ* S_old) + ε B) / (1 - t Λ*), `diag` = Λ* as one more (n, ld) tensor; the same criterion and
    return value."""
    import torch
    n, ld = S_new.shape
    for t in (J, B, eps, diag, S_old, S_new):
        if t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != (n, ld):
            raise ValueError("continuum_ali_update_dev: contiguous float64 tensors of one (n, ld) shape")
    out, cnt = ctypes.c_double(), ctypes.c_int64()
    st = torch.cuda.current_stream(S_new.device).cuda_stream
    check(_lib.load().vrt_continuum_ali_update_dev(sites.handle, int(ld if nlam is None else nlam), int(ld), J.data_ptr(),
                                                   B.data_ptr(), eps.data_ptr(), diag.data_ptr(), float(eps_thick),
                                                   S_old.data_ptr(), S_new.data_ptr(), ctypes.byref(out), ctypes.byref(cnt),
                                                   st or None))
    return out.value, int(cnt.value)


_OPERATORS = {None: 0, "diagonal": 1}


def _continuum_loop(L, prefix: str, h, case: ContinuumCase, eps_conv: float, maxiter: int, ng, S0, who: str, operator=None):
    fn = lambda name: getattr(L, prefix + name)
    steps, history, diff, i = [], [], 1.0, 0                   # criterion(S_new = B, S_old = 0) = 1
    if S0 is not None:
        S0 = _f64(S0).reshape(case.n, case.nlam)
        check(fn("set_source")(h, _d(S0)))
    if operator is not None:
        # (the raster session's setter is vrt_regular_continuum_select_operator)
        check(fn("select_operator" if prefix == "vrt_regular_continuum_" else "set_operator")(h, _OPERATORS[operator]))
    if ng is not None:
        check(fn("set_acceleration")(h, 2, *_ng_settings(ng)))
    while diff > eps_conv and i < maxiter:                     # criterion: diff > ϵ && i < maxiter, :178, :197
        d = ctypes.c_double()
        check(fn("iterate")(h, ctypes.byref(d)))
        diff = d.value
        history.append(diff)
        i += 1
        if ng is not None:
            _ng_last(fn("last_acceleration"), h, i, steps)
        if diff != diff:
            import warnings
            warnings.warn(f"{who}: NaN DIFF! at iteration {i} -- stopping, results are not converged")
    J, S = np.zeros((case.n, case.nlam)), np.zeros((case.n, case.nlam))
    check(fn("get")(h, _d(J), _d(S)))
    return (J, S, history) if ng is None else (J, S, history, steps)


def Lambda_continuum(eps_conv: float, maxiter: int, sites: VoronoiSites, case: ContinuumCase, quadrature: str, ng=None,
                     S0=None, native: bool = True, n_sweeps: int = 3, operator=None):
    """Λ_voronoi of src/lambda_continuum.jl:109-160 with library-owned device state (`vrt_continuum_create` /
    `_iterate` / `_get`): one call per iteration, only the criterion's scalar -- the maximum over the thick entries --
    comes back inside the loop.  Starts from S = B_0, or from S0 (n, nλ) (`vrt_continuum_set_source`: a warm start or a
    resumed run).  native=False keeps the caller's layout inside the session (VRT_LAMBDA_NATIVE=0): the same bits.
    Returns (J, S_new, history); ng=(start, period) as for `Lambda_voronoi_host`, with the list of (iterate, applied, a,
    b) as a fourth element.  operator="diagonal": accelerated Λ-iteration with the local operator Λ*
    (`vrt_continuum_set_operator`; `lambda_diagonal` returns that Λ*), which composes with ng."""
    L = _lib.load()
    if case.n != sites.n:
        raise ValueError(f"the continuum case has {case.n} points, the grid {sites.n}")
    if operator not in _OPERATORS:
        raise ValueError(f"Lambda_continuum: operator must be None or 'diagonal', not {operator!r}")
    if native:
        plan, w = _quadrature_plan(sites, quadrature, n_sweeps)
        own = None
    else:                                                      # (the option is read when the session is created)
        w, th, ph, _ = read_quadrature(quadrature)
        own = plan = FormalPlan(sites, quadrature_directions(th, ph), n_sweeps,
                                dirs=[1 if t > 90 else (-1 if t < 90 else 0) for t in th])
        plan.set_option("VRT_LAMBDA_NATIVE", 0)
    cc = case.c_struct()
    h = ctypes.c_void_p()
    try:
        check(L.vrt_continuum_create(plan._h, ctypes.byref(cc), _d(_f64(w)), ctypes.byref(h)))
        return _continuum_loop(L, "vrt_continuum_", h, case, eps_conv, maxiter, ng, S0, "Lambda_continuum", operator)
    finally:
        if h:
            L.vrt_continuum_destroy(h)
        if own is not None:
            own.close()


def lambda_diagonal_regular(z, x, y, alpha, quadrature: str, device: int = 0) -> np.ndarray:
    """The diagonal approximate operator Λ* of accelerated Λ-iteration on a raster (`vrt_regular_lambda_diagonal`): per
    (point, wavelength) the coefficient of the point's own S in its intensity after one sweep of the raster solve, summed
    over the angles of `quadrature` with their weights; exactly 0 on the ghost border.  z, x, y are the axes with the
    periodic ghost border, alpha (n,) or (n, nλ) over all nz nx ny points in Julia order, finite and > 0; returns (n, nλ)."""
    alpha = _f64(alpha)
    if alpha.ndim == 1:
        alpha = alpha.reshape(-1, 1)
    n = int(np.size(z)) * int(np.size(x)) * int(np.size(y))
    if alpha.ndim != 2 or alpha.shape[0] != n:
        raise ValueError(f"lambda_diagonal_regular: alpha must be ({n},) or ({n}, nlam)")
    w, k, dirs = _regular_directions(quadrature)
    solver = _regular_solver(z, x, y, n, device)
    try:
        diag = np.zeros_like(alpha)
        check(_lib.load().vrt_regular_lambda_diagonal(solver._h, k.shape[0], _d(k), dirs.ctypes.data_as(_lib.p_int), _d(w),
                                                      alpha.shape[1], alpha.shape[1], _d(alpha), _d(diag)))
        return diag
    finally:
        solver.close()


def line_lambda_diagonal_regular(z, x, y, alpha_per_angle, quadrature: str, device: int = 0) -> np.ndarray:
    """Λ* of the line Λ-iteration on a raster (`vrt_regular_line_lambda_diagonal`): `lambda_diagonal_regular` with an α of its
    own per angle, alpha_per_angle (n_angles, n, nλ) in quadrature order over all nz nx ny points in Julia order (the
    Doppler-shifted α_tot of the line loop), finite and > 0; the block of a θ = 90 angle is never read.  Returns (n, nλ)."""
    alpha = _f64(alpha_per_angle)
    n = int(np.size(z)) * int(np.size(x)) * int(np.size(y))
    w, k, dirs = _regular_directions(quadrature)
    if alpha.ndim != 3 or alpha.shape[0] != len(w) or alpha.shape[1] != n:
        raise ValueError(f"line_lambda_diagonal_regular: alpha_per_angle must be ({len(w)}, {n}, nlam)")
    nlam = alpha.shape[2]
    solver = _regular_solver(z, x, y, n, device)
    try:
        diag = np.zeros((n, nlam))
        check(_lib.load().vrt_regular_line_lambda_diagonal(solver._h, k.shape[0], _d(k), dirs.ctypes.data_as(_lib.p_int), _d(w),
                                                           nlam, nlam, _d(alpha), _d(diag)))
        return diag
    finally:
        solver.close()


def Lambda_continuum_regular(eps_conv: float, maxiter: int, z, x, y, case: ContinuumCase, quadrature: str, ng=None,
                             S0=None, n_sweeps: int = 3, device: int = 0, operator=None):
    """Λ_regular of src/lambda_continuum.jl:58-107 with library-owned device state (`vrt_regular_continuum_*`).  z, x, y
    are the raster's axes with the periodic ghost border; every one of its nz nx ny points is a point of `case` (Julia
    order i = iz + nz (ix + nx iy), i.e. numpy (ny, nx, nz) flattened).  Otherwise as `Lambda_continuum`, operator="diagonal"
    included (`vrt_regular_continuum_select_operator`; `lambda_diagonal_regular` returns that Λ*)."""
    L = _lib.load()
    if operator not in _OPERATORS:
        raise ValueError(f"Lambda_continuum_regular: operator must be None or 'diagonal', not {operator!r}")
    w, k, dirs = _regular_directions(quadrature)
    solver = _regular_solver(z, x, y, case.n, device)
    cc = case.c_struct()
    h = ctypes.c_void_p()
    try:
        check(L.vrt_regular_continuum_create(solver._h, k.shape[0], _d(k), dirs.ctypes.data_as(_lib.p_int), _d(w),
                                             ctypes.byref(cc), int(n_sweeps), ctypes.byref(h)))
        return _continuum_loop(L, "vrt_regular_continuum_", h, case, eps_conv, maxiter, ng, S0, "Lambda_continuum_regular",
                               operator)
    finally:
        if h:
            L.vrt_regular_continuum_destroy(h)
        solver.close()
