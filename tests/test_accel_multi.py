"""Ng acceleration with S held in pieces: the standalone halves of the step (vrt_ng_sums_dev, vrt_ng_coefficients,
vrt_ng_apply_dev; api.ng_sums / ng_coefficients / ng_apply) and distributed.ng_step.

Bounds: a sum against numpy's exact sum, 2^-40 Σ|t| (test_accel.py; adding the partial sums of W pieces on the host
lengthens the longest chain of additions by W links, far inside the 8192 the bound admits).  The elementwise results (x_acc,
the split sums against the fused ones for one array) are compared bit for bit."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from voronoirt_amd import api
from test_accel import SUM_BOUND, _accelerate, _device, _geometric, _iterates, _reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ptrs(d):
    return [t.data_ptr() for t in d]


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- 1: split equals fused -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097, 1_000_003, 2 ** 26 + 3])
def test_gpu_ng_sums_and_apply_are_the_fused_call_bit_for_bit(count):
    import torch
    xs = _iterates(count, seed=count % 1000)
    d = _device(xs)
    applied, sums, coeffs, out = _accelerate(d)
    assert np.array_equal(api.ng_sums_dev(count, *_ptrs(d), _stream()), sums)
    co = api.ng_coefficients(sums)
    if co is None:                                  # (one element: a rank-one system)
        assert not applied
        return
    assert np.array(co).tobytes() == coeffs.tobytes()
    out2 = torch.full_like(d[0], -7.0)
    good = api.ng_apply_dev(count, coeffs[0], coeffs[1], *_ptrs(d[:3]), out2.data_ptr(), _stream())
    assert good == applied
    if applied:
        assert torch.equal(out, out2)


@pytest.mark.gpu
def test_gpu_ng_sums_and_apply_take_unaligned_arrays_with_the_same_bits():
    import torch
    count = 100_001
    xs = _iterates(count, seed=17)
    d = _device(xs)
    applied, sums, coeffs, out = _accelerate(d)
    assert applied
    pad = [torch.empty(count + 1, dtype=torch.float64, device="cuda:0") for _ in range(5)]
    off = []
    for p, t in zip(pad, d):
        p[1:] = t
        off.append(p[1:])
        assert off[-1].data_ptr() % 16 == 8
    assert np.array_equal(api.ng_sums_dev(count, *_ptrs(off), _stream()), sums)
    out_u = pad[4][1:]
    assert api.ng_apply_dev(count, coeffs[0], coeffs[1], *_ptrs(off[:3]), out_u.data_ptr(), _stream())
    assert torch.equal(out, out_u)


@pytest.mark.gpu
def test_gpu_ng_pieces_host_arrays():
    x_star, xs = _geometric(0.9, 0.5, N=2000)
    xs = [x.reshape(50, 40) for x in xs]
    x_acc, sums, coeffs = api.ng_accelerate(*xs)
    s = api.ng_sums(*xs)
    assert np.array_equal(s, sums)
    a, b = api.ng_coefficients(s)
    assert (a, b) == tuple(coeffs)
    y, good = api.ng_apply(a, b, *xs[:3])
    assert good and y.shape == (50, 40) and np.array_equal(y, x_acc)
    assert api.ng_coefficients(np.zeros(5)) is None


# ---- 2: a split S gives the verdict of the whole -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_ng_split_arrays_give_the_sums_and_the_verdict_of_the_whole():
    import torch
    x_star, xs = _geometric(0.9, 0.5, N=50_000)
    j = 31_337
    for k in range(4):
        xs[k][j] = -0.01 + 0.9 ** k * 0.5
    ref = _reference(*xs)
    applied, sums, coeffs, _ = _accelerate(_device(xs))
    assert not applied
    cut = 20_001                                    # odd: the second half starts 8 bytes off a 16-byte boundary
    d = _device(xs)
    halves = [[t[:cut] for t in d], [t[cut:] for t in d]]
    assert halves[1][0].data_ptr() % 16 == 8
    parts = [api.ng_sums_dev(h[0].numel(), *_ptrs(h), _stream()) for h in halves]
    total = np.zeros(5)
    for p in parts:                                 # in the order of the pieces
        total = total + p
    err = np.abs(total - sums)
    print(f"split at {cut}: |Σ parts - fused| / Σ|t| = {err / ref['mags']}, bound {SUM_BOUND:.3e}")
    assert (err <= SUM_BOUND * ref["mags"]).all()
    assert (np.abs(total - ref["sums"]) <= SUM_BOUND * ref["mags"]).all()
    a, b = api.ng_coefficients(total)
    assert abs(a - ref["a"]) <= ref["da"] and abs(b - ref["b"]) <= ref["db"]
    verdicts = []
    for h in halves:
        out = torch.empty_like(h[0])
        verdicts.append(api.ng_apply_dev(h[0].numel(), a, b, *_ptrs(h[:3]), out.data_ptr(), _stream()))
    assert verdicts == [j >= cut, j < cut]          # exactly the half that holds the offending element is bad


# ---- 3: the sharded leg -----------------------------------------------------------------------------------------------------------------------
_NG_STEP_WORKER = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch, torch.distributed as dist
from voronoirt_amd import api, distributed as D
rank, world = D.init_process_group("nccl", force=True)
assert (rank, world) == (0, 1) and dist.is_initialized()
rng = np.random.default_rng(3)
N = 100_001
x_star = rng.uniform(1.0, 2.0, N)
u, v = 0.1 * rng.normal(size=N), 0.1 * rng.normal(size=N)
xs = [x_star + 0.9 ** k * u + 0.5 ** k * v for k in range(4)]
d = [torch.from_numpy(x).to("cuda:0") for x in xs]
out = torch.empty_like(d[0])
ok, sums, coeffs = api.ng_accelerate_dev(N, *(t.data_ptr() for t in d), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
applied, s2, c2, y = D.ng_step(*d)
assert ok and applied and np.array_equal(s2, sums) and np.array_equal(c2, coeffs) and torch.equal(y, out)
# a step that leaves the positive numbers is refused through the MAX of the inverted verdicts
for k in range(4):
    d[k][77] = -0.01 + 0.9 ** k * 0.5
applied, s3, c3, _ = D.ng_step(*d)
assert not applied and c3 is not None
# a singular system is refused before any apply
applied, s4, c4, _ = D.ng_step(d[0], d[0], d[0], d[0])
assert not applied and c4 is None and not s4.any()
dist.destroy_process_group()
print("ok")
"""


@pytest.mark.gpu
def test_gpu_distributed_ng_step_on_a_world_of_one(tmp_path):
    script = tmp_path / "ng_step_worker.py"
    script.write_text(_NG_STEP_WORKER)
    with socket.socket() as s:                      # a port that is free now (a fixed one collides with a concurrent run)
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
