"""sg_pairwise_sqdist (csrc/pdist.hip) on the GPU against the direct fp64 sum of (a - b)^2 (tests/nnref.py).
Small-integer inputs make every product, every f32 chain of at most C = sg_pairwise_sqdist_chunk() terms (9 C < 2^24) and
every f64 sum exact, so those cases compare with ==: a dropped, doubled or misplaced element cannot hide.  The float
cases carry the rigorous bound 2 gamma_n (|a_i|^2 + |b_j|^2), n = min(v, C); the 64-bit case a closed form."""
import ctypes as C_

import numpy as np
import pytest
import torch

from tests import nnref

pytestmark = pytest.mark.gpu


def _chunk():
    from saragan_amd import _lib
    return int(_lib.load().sg_pairwise_sqdist_chunk())


def _ints(rng, m, v):
    return rng.integers(-3, 4, size=(m, v)).astype(np.float32)


def _run(a, b=None):
    from saragan_amd.metrics.sample_metrics import pairwise_sqdist
    ta = torch.as_tensor(a, device='cuda')
    out = pairwise_sqdist(ta, None if b is None else torch.as_tensor(b, device='cuda'))
    assert out.dtype == torch.float64 and out.is_cuda
    return out


# (ma, mb or None for the symmetric call, v as a function of the chunk C)
EXACT = [(1, None, lambda C: 1), (2, None, lambda C: 7), (33, None, lambda C: 257), (130, None, lambda C: 4099),
         (64, None, lambda C: C - 1), (64, None, lambda C: C), (64, None, lambda C: C + 1), (70, None, lambda C: 3 * C + 5),
         (5, 67, lambda C: 3 * C + 5), (67, 5, lambda C: 3 * C + 5), (1, 129, lambda C: 8191),
         # beyond the issue's list: 3 x 3 tiles of 128 with the 16-byte loads, 2 x 2 tiles of 128 two-set, 16-byte loads on
         # the 64-row tile across a chunk boundary, and the 64 / 65-row switch between the two tile sizes
         (300, None, lambda C: 68), (130, 200, lambda C: 100), (40, 64, lambda C: 2 * C + 8), (65, None, lambda C: 36)]


@pytest.mark.parametrize('case', range(len(EXACT)))
def test_integer_inputs_are_exact(case):
    ma, mb, vf = EXACT[case]
    C = _chunk()
    assert 9 * C < 2 ** 24
    v = vf(C)
    rng = np.random.default_rng(100 + case)
    a = _ints(rng, ma, v)
    if mb is None:
        out = _run(a)
        want = nnref.sqdist(a)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (ma, v, np.argwhere(got != want)[:5])
        assert torch.equal(out, out.t().contiguous())                   # bitwise mirror
        assert torch.count_nonzero(torch.diagonal(out)).item() == 0     # exact zeros
        two = _run(a, a.copy())                                         # the two-set path on a and a clone
        assert torch.equal(out, two)
    else:
        b = _ints(rng, mb, v)
        got = _run(a, b).cpu().numpy()
        want = nnref.sqdist(a, b)
        assert got.shape == (ma, mb) and np.array_equal(got, want), (ma, mb, v, np.argwhere(got != want)[:5])


@pytest.mark.parametrize('ma,mb,v', [(70, None, 50000), (37, 41, 12345)])
def test_float_inputs_within_the_rounding_bound(ma, mb, v):
    rng = np.random.default_rng(7)
    a = rng.standard_normal((ma, v)).astype(np.float32)
    b = None if mb is None else rng.standard_normal((mb, v)).astype(np.float32)
    out = _run(a, b)
    again = _run(a, b)
    assert torch.equal(out, again)                                      # deterministic: the same bits
    want = nnref.sqdist(a, b)
    bound = nnref.sqdist_bound(a, a if b is None else b, _chunk())
    err = np.abs(out.cpu().numpy() - want)
    na = (a.astype(np.float64) ** 2).sum(1)
    nb = na if b is None else (b.astype(np.float64) ** 2).sum(1)
    print(f'pairwise_sqdist ({ma}, {mb}, {v}): max |err| / (|a_i|^2 + |b_j|^2) = {(err / (na[:, None] + nb[None, :])).max():.3e}'
          f' (bound {2 * nnref.gamma(min(v, _chunk())):.3e})')
    assert (err <= bound).all(), float((err / bound).max())
    if b is None:
        assert torch.equal(out, out.t().contiguous()) and torch.count_nonzero(torch.diagonal(out)).item() == 0


def test_offsets_past_32_bits():
    """5 rows of 2^29 + 1 voxels: the last rows start past element 2^31 and the tensor ends past byte 2^33."""
    from saragan_amd.metrics.sample_metrics import pairwise_sqdist
    v = 2 ** 29 + 1
    if torch.cuda.mem_get_info()[0] < 16 * 2 ** 30:
        pytest.skip('under 16 GiB of free device memory')
    c = [0, 1, 2, 3, -1]
    x = torch.empty((5, v), dtype=torch.float32, device='cuda')
    for i, ci in enumerate(c):
        x[i].fill_(float(ci))
    first = [ci + (1 if i % 2 == 1 else 0) for i, ci in enumerate(c)]
    last = list(c)
    last[4] += 2
    for i in range(5):
        x[i, 0] = float(first[i])
        x[i, v - 1] = float(last[i])
    got = pairwise_sqdist(x).cpu().numpy()
    want = np.array([[(v - 2) * (c[i] - c[j]) ** 2 + (first[i] - first[j]) ** 2 + (last[i] - last[j]) ** 2 for j in range(5)]
                     for i in range(5)], dtype=np.float64)
    del x
    assert np.array_equal(got, want), (got, want)


def test_invalid_arguments_return_the_error_code_and_launch_nothing():
    from saragan_amd import _lib
    lib = _lib.load()
    ma, mb, v = 3, 4, 10
    a = torch.ones((ma, v), device='cuda')
    b = torch.ones((mb, v), device='cuda')
    out = torch.full((ma, mb), -7.0, dtype=torch.float64, device='cuda')
    nbytes = lib.sg_pairwise_sqdist_workspace(ma, mb, v)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    p = lambda t: C_.c_void_p(t.data_ptr())
    st = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(a=p(a), b=p(b), out=p(out), ma=ma, mb=mb, v=v, ws=p(ws), nbytes=nbytes)
    bad = [dict(a=None), dict(b=None), dict(out=None), dict(ws=None), dict(ma=0), dict(mb=0), dict(v=0), dict(ma=-1),
           dict(nbytes=nbytes - 1), dict(nbytes=0)]
    for change in bad:
        k = dict(good, **change)
        rc = lib.sg_pairwise_sqdist(k['a'], k['b'], k['out'], k['ma'], k['mb'], k['v'], k['ws'], k['nbytes'], st)
        assert rc in (_lib_code('SG_EINVAL'), _lib_code('SG_EWORKSPACE')), (change, rc)
        assert rc == (_lib_code('SG_EWORKSPACE') if 'nbytes' in change else _lib_code('SG_EINVAL')), (change, rc)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()), change
    assert lib.sg_pairwise_sqdist_workspace(0, 4, 10) == 0
    k = good
    assert lib.sg_pairwise_sqdist(k['a'], k['b'], k['out'], ma, mb, v, k['ws'], nbytes, st) == 0
    assert bool((out == 0.0).all())          # all-ones rows: every distance is 0


def _lib_code(name):
    return {'SG_EINVAL': -1, 'SG_EWORKSPACE': -2}[name]


def test_workspace_stays_bounded():
    """The split shrinks as the tiles grow: 2048 pooled volumes do not take a fixed split's gigabytes."""
    from saragan_amd import _lib
    lib = _lib.load()
    v = 32 * 128 * 128
    assert lib.sg_pairwise_sqdist_workspace(2048, 2048, v) < 256 * 2 ** 20
    assert lib.sg_pairwise_sqdist_workspace(48, 48, 64 * 256 * 256) < 256 * 2 ** 20
