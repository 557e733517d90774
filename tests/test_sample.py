"""Site sampling from a raster density on the GPU (vrt_sample_sites[_dev]) against a numpy restatement of its
semantics (include/voronoirt.h, "sites sampled from a raster density"), and the whole chain raster -> sites ->
tessellation -> fields on the sites -> J in one process."""
import re

import numpy as np
import pytest

import voronoirt_amd as vrt
from oracle import oracle as orc
from oracle.parity import rel
from voronoirt_amd import _lib, synth

pytestmark = pytest.mark.gpu

RTOL = 1e-10     # the fp64 tolerance of tests/test_gpu_parity.py


# ---- numpy restatement ----------------------------------------------------------------------------------------------
def trilinear(zk, xk, yk, z, x, y, q):
    """src/functions.jl:207-248 at points (zk, xk, yk) of one raster q (ny, nx, nz)"""
    def itv(ax, v):
        return np.clip(np.searchsorted(ax, v, side="left") - 1, 0, ax.size - 2)
    iz, ix, iy = itv(z, zk), itv(x, xk), itv(y, yk)
    x_d = (xk - x[ix]) / (x[ix + 1] - x[ix])
    y_d = (yk - y[iy]) / (y[iy + 1] - y[iy])
    z_d = (zk - z[iz]) / (z[iz + 1] - z[iz])
    V = lambda a, b, c: q[iy + c, ix + b, iz + a]      # noqa: E731  (vals[idz+a, idx+b, idy+c])
    c00 = V(0, 0, 0) * (1 - x_d) + V(0, 1, 0) * x_d
    c01 = V(1, 0, 0) * (1 - x_d) + V(1, 1, 0) * x_d
    c10 = V(0, 0, 1) * (1 - x_d) + V(0, 1, 1) * x_d
    c11 = V(1, 0, 1) * (1 - x_d) + V(1, 1, 1) * x_d
    c0 = c00 * (1 - y_d) + c10 * y_d
    c1 = c01 * (1 - y_d) + c11 * y_d
    return c0 * (1 - z_d) + c1 * z_d


def sample_numpy(z, x, y, q, n, seed, max_proposals=0, chunk=1 << 20):
    """proposals j in chunks; the first n accepted.  Returns (positions (k, 3), proposals used), k < n at the cap"""
    q = np.asarray(q, dtype=np.float64).reshape(y.size, x.size, z.size)
    q_min, q_max = q.min(), q.max()
    dq = q_max - q_min
    cap = max_proposals or 1000 * n + (1 << 20)
    rows, got, j0 = [], 0, 0
    while got < n and j0 < cap:
        j = np.arange(j0, min(j0 + chunk, cap), dtype=np.uint64)
        u = [synth.counter_uniform(seed, c, j) for c in range(4)]
        zr = u[0] * (z[-1] - z[0]) + z[0]
        xr = u[1] * (x[-1] - x[0]) + x[0]
        yr = u[2] * (y[-1] - y[0]) + y[0]
        take = np.nonzero(trilinear(zr, xr, yr, z, x, y, q) > u[3] * dq + q_min)[0][: n - got]
        rows.append(np.stack([zr[take], xr[take], yr[take]], 1))
        got += take.size
        used = j0 + int(take[-1]) + 1 if got == n else min(j0 + chunk, cap)
        j0 += chunk
    return np.concatenate(rows), used


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- rasters ------------------------------------------------------------------------------------------------------------
def small_raster():
    rng = np.random.default_rng(17)
    z = np.cumsum(rng.uniform(0.2, 1.0, 17)) - 3.0         # non-uniform, 17 x 11 x 13 (nz, nx, ny)
    x = np.cumsum(rng.uniform(0.5, 1.5, 11))
    y = np.cumsum(rng.uniform(0.1, 2.0, 13)) + 100.0
    return z, x, y, rng


def quantities():
    z, x, y, rng = small_raster()
    shape = (y.size, x.size, z.size)
    pos = rng.random(shape) + 0.2
    neg = rng.normal(size=shape) * 3.0 - 1.5                # q_min < 0
    Y, X, Z = np.meshgrid(y, x, z, indexing="ij")
    zc, xc, yc = z[8], x[5], y[6]
    spike = np.exp(-(((Z - zc) / 0.95) ** 2 + ((X - xc) / 1.3) ** 2 + ((Y - yc) / 1.55) ** 2))   # ~1 % acceptance
    return z, x, y, {"positive": pos, "negative": neg, "spike": spike}


def test_native_library_is_the_compute_path():
    assert _lib.load().vrt_device_count() >= 1
    assert _lib.LIB_PATH.endswith("voronoirt_amd/libvrt_hip.so")


@pytest.mark.parametrize("name", ["positive", "negative", "spike"])
@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15])
def test_bit_equal_to_numpy(name, seed):
    z, x, y, qs = quantities()
    q = qs[name]
    for n in (1, 63, 64, 65, 5000):
        ref, ref_used = sample_numpy(z, x, y, q, n, seed)
        got, used = vrt.rejection_sampling(n, z, x, y, q, seed, return_proposals=True)
        assert ref.shape == (n, 3)
        assert same_bits(got, ref), (name, seed, n)
        assert used == ref_used, (name, seed, n)
        if name == "spike" and n == 5000:
            assert 0.003 < n / used < 0.03                    # about 1 % accepted
    # the box is the axes' end points
    assert got[:, 0].min() >= z[0] and got[:, 0].max() <= z[-1] and got[:, 2].min() >= y[0]


def test_independent_of_batch():
    z, x, y, qs = quantities()
    outs = []
    for q, n in ((qs["negative"], 3000), (qs["spike"], 700)):
        base, used = vrt.rejection_sampling(n, z, x, y, q, 5, return_proposals=True)
        for batch in (64, 1000, 10 ** 7):
            got, u = vrt.rejection_sampling(n, z, x, y, q, 5, batch=batch, return_proposals=True)
            assert same_bits(got, base) and u == used, batch
        outs.append(base)
    # batches that end inside a wave of 64 proposals, and one proposal per batch
    got = vrt.rejection_sampling(40, z, x, y, qs["spike"], 5, batch=1)
    assert same_bits(got, outs[1][:40])
    got = vrt.rejection_sampling(700, z, x, y, qs["spike"], 5, batch=97)
    assert same_bits(got, outs[1])


def test_host_and_device_forms_agree():
    import torch
    z, x, y, qs = quantities()
    q = qs["negative"]
    n = 4097
    ref, ref_used = vrt.rejection_sampling(n, z, x, y, q, 11, return_proposals=True)
    s = torch.cuda.Stream()
    P = q.size
    big = torch.full((P + 13,), 7.0e300, dtype=torch.float64, device="cuda")   # the slice's neighbours are the max
    big[13:] = torch.as_tensor(q.ravel(), device="cuda")
    dq = big[13:]
    assert dq.storage_offset() == 13
    dpos = torch.full((n + 5, 3), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        used = vrt.rejection_sampling_dev(n, z, x, y, dq.data_ptr(), 11, dpos.data_ptr(), stream=s.cuda_stream)
        used2 = vrt.rejection_sampling_dev(n, z, x, y, dq.data_ptr(), 11, dpos[1:].data_ptr(), batch=333,
                                           stream=s.cuda_stream)
    torch.cuda.synchronize()
    got = dpos.cpu().numpy()
    assert used == used2 == ref_used
    assert same_bits(got[1:n + 1], ref) and np.isnan(got[n + 1:]).all()
    assert same_bits(got[:1], ref[:1])


def test_cap_is_enforced():
    import torch
    z, x, y, _ = quantities()
    q = np.zeros((y.size, x.size, z.size))
    q[6, 5, 8] = 1.0                       # accepted only near one raster node: about 7e-4 of the box
    n, cap = 1000, 20000
    ref, ref_used = sample_numpy(z, x, y, q, n, 3, max_proposals=cap)
    k = ref.shape[0]
    assert 0 < k < n and ref_used == cap
    with pytest.raises(vrt.VrtError) as e:
        vrt.rejection_sampling(n, z, x, y, q, 3, max_proposals=cap)
    assert e.value.code == _lib.VRT_EINVAL
    m = re.search(r"(\d+) of (\d+) sites accepted in (\d+) proposals", e.value.message)
    assert m and (int(m[1]), int(m[2]), int(m[3])) == (k, n, cap), e.value.message
    # the device form has written the accepted rows and nothing past them
    dq = torch.as_tensor(q.ravel(), device="cuda")
    dpos = torch.full((n, 3), np.nan, dtype=torch.float64, device="cuda")
    with pytest.raises(vrt.VrtError) as e:
        vrt.rejection_sampling_dev(n, z, x, y, dq.data_ptr(), 3, dpos.data_ptr(), max_proposals=cap, batch=4096)
    assert e.value.code == _lib.VRT_EINVAL and f"{k} of {n} sites accepted in {cap} proposals" in e.value.message
    got = dpos.cpu().numpy()
    assert same_bits(got[:k], ref) and np.isnan(got[k:]).all()
    # a quantity that accepts nothing is refused, on the host and after the device reduction
    for bad in (np.full_like(q, 2.5), np.where(q > 0, np.nan, q)):
        with pytest.raises(vrt.VrtError) as e:
            vrt.rejection_sampling(10, z, x, y, bad, 3)
        assert e.value.code == _lib.VRT_EINVAL
        with pytest.raises(vrt.VrtError) as e:
            vrt.rejection_sampling_dev(10, z, x, y, torch.as_tensor(bad.ravel(), device="cuda").data_ptr(), 3,
                                       dpos.data_ptr())
        assert e.value.code == _lib.VRT_EINVAL


def test_distribution_of_a_linear_quantity():
    """q = 2 + 3 (z - z_0) on a non-uniform z axis: trilinear reproduces it, so the sites have the density
    2 (z - z_0)/Lz^2 in z (proportional to q - q_min) and are uniform in x and y."""
    z = np.array([0.0, 0.05, 0.2, 0.5, 0.55, 1.0, 1.6, 2.0])
    x = np.linspace(-3.0, 3.0, 5)
    y = np.linspace(0.0, 1.0, 4)
    q = np.broadcast_to(2.0 + 3.0 * (z - z[0]), (y.size, x.size, z.size)).copy()
    n, nb = 200_000, 20
    pos, used = vrt.rejection_sampling(n, z, x, y, q, 21, return_proposals=True)
    assert abs(n / used - 0.5) < 0.01                         # the mean of (z - z0)/Lz
    Lz = z[-1] - z[0]
    e = np.linspace(0.0, 1.0, nb + 1)
    cz = np.histogram((pos[:, 0] - z[0]) / Lz, e)[0]
    exp_z = n * (e[1:] ** 2 - e[:-1] ** 2)
    cx = np.histogram((pos[:, 1] - x[0]) / (x[-1] - x[0]), e)[0]
    cy = np.histogram((pos[:, 2] - y[0]) / (y[-1] - y[0]), e)[0]
    # bound: 5 standard deviations of a binomial count (the seed is fixed: the test is deterministic)
    for c, ex in ((cz, exp_z), (cx, np.full(nb, n / nb)), (cy, np.full(nb, n / nb))):
        assert (np.abs(c - ex) < 5 * np.sqrt(ex * (1 - ex / n)) + 1).all(), (c, ex)


def test_full_size_bit_equal():
    a = synth.atmosphere_raster(128, 256, 256, seed=1)
    inv = 1.0 / np.log10(a["N_H"])
    q = (inv * inv) * a["T"] ** (-0.4)
    n = 1_000_000
    got, used = vrt.sample_from_invNH_invT(a["z"], a["x"], a["y"], a["N_H"], a["T"], n, 8, return_proposals=True)
    ref, ref_used = sample_numpy(a["z"], a["x"], a["y"], q, n, 8)
    assert used == ref_used and same_bits(got, ref)


def test_raster_to_J_in_one_process():
    """sample_from_invNH_invT -> voro -> VoronoiSites -> initialise (T, N_H) -> J_lambda_voronoi, against the oracle"""
    a = synth.atmosphere_raster(48, 24, 24, seed=6)
    z, x, y = a["z"], a["x"], a["y"]
    n = 6000
    pos = vrt.sample_from_invNH_invT(z, x, y, a["N_H"], a["T"], n, 2)
    bounds = (z[0], z[-1], x[0], x[-1], y[0], y[-1])
    nbr = vrt.voro(pos, bounds)
    sites = vrt.VoronoiSites(pos, nbr, bounds)
    try:
        fields = vrt.initialise(sites, z, x, y, np.stack([a["T"], a["N_H"]]))
        T, N_H = fields[:, 0], fields[:, 1]
        assert np.isfinite(fields).all() and T.min() > 3000 and N_H.min() > 1e17
        # more sites where q = log10(N_H)^-2 T^-0.4 - q_min is larger: the top (low N_H, hot) is sparser per volume
        nlam = 4
        S = (T / 5000.0)[:, None] ** 4 * (1.0 + 0.1 * np.arange(nlam))[None, :]
        alpha = (1e-26 * N_H)[:, None] * (1.0 + 0.5 * np.arange(nlam))[None, :]
        I0 = S[sites.perm_up[: sites.layers_up[1] - 1] - 1]
        J = vrt.J_lambda_voronoi(S, alpha, sites, "ul7n12.dat", I0_up=I0)
        so = orc.make_sites(pos, nbr, bounds)
        w, th, ph, _ = vrt.read_quadrature("ul7n12.dat")
        ref = orc.J_voronoi(w, th, ph, S, alpha, so, I0_up=I0, nthreads=8)
        assert J.shape == (n, nlam) and rel(J, ref) < RTOL
    finally:
        sites.close()
