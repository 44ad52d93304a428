"""sg_sqdist_exact and sg_topk_merge (csrc/sqdist_exact.hip) on the GPU against int64 arithmetic by the definition,
sum_e (q[i][e] - r[j][e])^2 -- torch int64 on the device, one query row at a time (tests/memref.py's formula).  Every
comparison is ==: the kernel's byte split, its i32 chunks, its K splits and its tile edges either give the integer or do not."""
import ctypes as C_

import numpy as np
import pytest
import torch

from tests import memref

pytestmark = pytest.mark.gpu

DTYPES = {'uint8': torch.uint8, 'int8': torch.int8, 'int16': torch.int16, 'uint16': torch.uint16}
RANGE = {'uint8': (0, 255), 'int8': (-128, 127), 'int16': (-32768, 32767), 'uint16': (0, 65535)}
I64_MAX = 2 ** 63 - 1
SG_EINVAL, SG_EWORKSPACE, SG_EALIGN = -1, -2, -3


def _lib():
    from saragan_amd import _lib
    return _lib.load()


def _chunk():
    return int(_lib().sg_sqdist_exact_chunk())


def _rand(gen, m, v, dtype):
    lo, hi = RANGE[dtype]
    return torch.randint(lo, hi + 1, (m, v), generator=gen, device='cuda', dtype=torch.int32).to(DTYPES[dtype])


def _ref(q, r):
    """int64 [mq, mr] on the device, one query row at a time, the reference rows in slices of 2^24 voxels."""
    out = torch.zeros((q.shape[0], r.shape[0]), dtype=torch.int64, device=q.device)
    step = 1 << 24
    for at in range(0, q.shape[1], step):
        r64 = r[:, at:at + step].to(torch.int64)
        for i in range(q.shape[0]):
            out[i] += ((r64 - q[i:i + 1, at:at + step].to(torch.int64)) ** 2).sum(dim=1)
    return out


def _run(q, r=None):
    from saragan_amd import functional as F
    out = F.sqdist_exact(q, r)
    assert out.dtype == torch.int64 and out.is_cuda and tuple(out.shape) == (q.shape[0], (q if r is None else r).shape[0])
    again = F.sqdist_exact(q, r)
    assert torch.equal(out, again)      # two calls, the same bits
    return out


# (mq, mr, v as a function of the chunk C): one tile, ragged tiles, more than one tile a side; v below, at and past the MFMA
# K, the load width and the chunk; an odd v across many chunks; a K split forced (2 x 2, 2^22) and not (130 x 130, 64)
SHAPES = [(1, 1, lambda C: 1), (17, 33, lambda C: 15), (33, 17, lambda C: 63), (130, 130, lambda C: 64), (130, 1, lambda C: 65),
          (1, 130, lambda C: C - 1), (17, 17, lambda C: C), (33, 130, lambda C: C + 1), (130, 33, lambda C: 2 * C + 5),
          (17, 17, lambda C: 1000003), (2, 2, lambda C: 1 << 22)]


def test_chunk_cannot_overflow_i32():
    C = _chunk()
    assert 1 <= C <= 2 ** 16 and 2 * 2 ** 14 * C < 2 ** 31      # two byte products a voxel in the cross accumulator


@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('case', range(len(SHAPES)))
def test_random_rows_are_exact(case, dtype):
    mq, mr, vf = SHAPES[case]
    v = vf(_chunk())
    gen = torch.Generator(device='cuda').manual_seed(1000 + case)
    q, r = _rand(gen, mq, v, dtype), _rand(gen, mr, v, dtype)
    got, want = _run(q, r), _ref(q, r)
    assert torch.equal(got, want), (mq, mr, v, (got != want).nonzero()[:5].tolist())


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_extremes_do_not_overflow(dtype):
    v = 2 * _chunk() + 5
    lo, hi = RANGE[dtype]
    a = torch.full((3, v), lo, dtype=torch.int32, device='cuda').to(DTYPES[dtype])
    b = torch.full((2, v), hi, dtype=torch.int32, device='cuda').to(DTYPES[dtype])
    want = (hi - lo) ** 2 * v
    assert dtype not in ('int16', 'uint16') or want == 65535 ** 2 * v
    assert _run(a, b).tolist() == [[want] * 2] * 3
    assert _run(b, a).tolist() == [[want] * 3] * 2
    assert _run(a, a.clone()).tolist() == [[0] * 3] * 3 and _run(b, b.clone()).tolist() == [[0] * 2] * 2


def test_constant_minimum_row():
    v = 2 * _chunk() + 5
    q = torch.full((1, v), -32768, dtype=torch.int16, device='cuda')
    r = torch.stack([q[0], torch.full((v,), 32767, dtype=torch.int16, device='cuda')])
    assert _run(q, r).tolist() == [[0, 65535 ** 2 * v]]
    assert _run(q).tolist() == [[0]]


@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('m,vf', [(1, lambda C: 7), (33, lambda C: 64), (130, lambda C: 2 * C + 5), (200, lambda C: 129)])
def test_symmetric_call(m, vf, dtype):
    v = vf(_chunk())
    gen = torch.Generator(device='cuda').manual_seed(7 + m)
    q = _rand(gen, m, v, dtype)
    if m > 2:
        q[2] = q[0]      # an off-diagonal zero
    out = _run(q)
    assert torch.count_nonzero(torch.diagonal(out)).item() == 0
    assert torch.equal(out, out.t().contiguous())
    assert torch.equal(out, _run(q, q.clone()))
    assert torch.equal(out, _run(q, q))
    assert torch.equal(out, _ref(q, q))


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_rows_that_are_only_element_aligned(dtype):
    mq, mr, v = 17, 33, 1001
    gen = torch.Generator(device='cuda').manual_seed(11)
    bq, br = _rand(gen, 1, mq * v + 1, dtype)[0], _rand(gen, 1, mr * v + 3, dtype)[0]
    q, r = bq[1:].view(mq, v), br[3:].view(mr, v)
    assert q.data_ptr() % 16 != 0 and r.data_ptr() % 16 != 0 and q.is_contiguous()
    assert torch.equal(_run(q, r), _ref(q.clone(), r.clone()))
    assert torch.equal(_run(q), _ref(q.clone(), q.clone()))


def test_reference_rows_past_four_gib():
    """u8, mq = 1, mr = 5, v = 2^30 + 7: the last reference row begins 2^32 + 28 bytes into its buffer."""
    v, mr = (1 << 30) + 7, 5
    gen = torch.Generator(device='cuda').manual_seed(5)
    r = torch.randint(0, 256, (mr, v), generator=gen, device='cuda', dtype=torch.uint8)
    q = torch.randint(0, 256, (1, v), generator=gen, device='cuda', dtype=torch.uint8)
    q[0, -9:] = 255
    r[mr - 1, -9:] = 0      # the very end of the last row counts
    assert (mr - 1) * v > 2 ** 32
    from saragan_amd import functional as F
    got, want = F.sqdist_exact(q, r), _ref(q, r)
    assert torch.equal(got, want), (got.tolist(), want.tolist())


def _raw(q, r, dt, mq, mr, v, out, ws, ws_bytes):
    p = lambda x: C_.c_void_p(x) if x else None
    return _lib().sg_sqdist_exact(p(q), p(r), dt, mq, mr, v, p(out), p(ws), ws_bytes, C_.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_contract_errors_return_before_any_launch():
    from saragan_amd import _lib as L
    lib = _lib()
    mq, mr, v = 3, 4, 100
    q = torch.ones((mq, v + 1), dtype=torch.int16, device='cuda')
    r = torch.ones((mr, v + 1), dtype=torch.int16, device='cuda')
    out = torch.full((mq * mr + 1,), -7, dtype=torch.int64, device='cuda')
    nbytes = int(lib.sg_sqdist_exact_workspace(mq, mr, v))
    assert nbytes > 0 and lib.sg_sqdist_exact_workspace(0, mr, v) == 0
    ws = torch.full((nbytes // 8 + 1,), -7, dtype=torch.int64, device='cuda')
    Q, R, O, W, I16 = q.data_ptr(), r.data_ptr(), out.data_ptr(), ws.data_ptr(), L.SG_SRC_I16
    bad = [((0, R, I16, mq, mr, v, O, W, nbytes), SG_EINVAL), ((Q, 0, I16, mq, mr, v, O, W, nbytes), SG_EINVAL),
           ((Q, R, I16, mq, mr, v, 0, W, nbytes), SG_EINVAL), ((Q, R, I16, mq, mr, v, O, 0, nbytes), SG_EINVAL),
           ((Q, R, I16, 0, mr, v, O, W, nbytes), SG_EINVAL), ((Q, R, I16, mq, 0, v, O, W, nbytes), SG_EINVAL),
           ((Q, R, I16, -1, mr, v, O, W, nbytes), SG_EINVAL), ((Q, R, I16, mq, mr, 0, O, W, nbytes), SG_EINVAL),
           ((Q, R, I16, mq, mr, 2 ** 31, O, W, nbytes), SG_EINVAL),
           ((Q, R, L.SG_SRC_F16, mq, mr, v, O, W, nbytes), SG_EINVAL), ((Q, R, L.SG_SRC_F32, mq, mr, v, O, W, nbytes), SG_EINVAL),
           ((Q, R, L.SG_SRC_BF16, mq, mr, v, O, W, nbytes), SG_EINVAL), ((Q, R, 99, mq, mr, v, O, W, nbytes), SG_EINVAL),
           ((Q, R, -1, mq, mr, v, O, W, nbytes), SG_EINVAL),
           ((Q, R, I16, mq, mr, v, O, W, nbytes - 1), SG_EWORKSPACE), ((Q, R, I16, mq, mr, v, O, W, 0), SG_EWORKSPACE),
           ((Q + 1, R, I16, mq, mr, v, O, W, nbytes), SG_EALIGN), ((Q, R + 1, I16, mq, mr, v, O, W, nbytes), SG_EALIGN),
           ((Q, R, L.SG_SRC_U16, mq, mr, v, O + 4, W, nbytes), SG_EALIGN), ((Q, R, I16, mq, mr, v, O, W + 4, nbytes), SG_EALIGN)]
    for args, code in bad:
        assert _raw(*args) == code, args
    torch.cuda.synchronize()
    assert (out == -7).all() and (ws == -7).all()
    assert _raw(Q + 1, R + 1, L.SG_SRC_U8, mq, mr, v, O, W, nbytes) == 0      # bytes need no alignment
    assert _raw(Q + 2, R + 2, I16, mq, mr, v, O, W, nbytes) == 0              # 16-bit rows: 2-byte alignment is enough
    torch.cuda.synchronize()
    assert (out[:mq * mr] == 0).all() and out[-1] == -7


def test_python_wrapper_checks_its_arguments():
    from saragan_amd import functional as F
    x = torch.zeros((2, 4), dtype=torch.int16, device='cuda')
    with pytest.raises(TypeError):
        F.sqdist_exact(x.float())
    with pytest.raises(TypeError):
        F.sqdist_exact(x, x.to(torch.uint16))
    with pytest.raises(ValueError):
        F.sqdist_exact(x, torch.zeros((2, 5), dtype=torch.int16, device='cuda'))
    with pytest.raises(ValueError):
        F.sqdist_exact(x, x.cpu())


# ---- sg_topk_merge
def _merge(d, k, steps, skip):
    from saragan_amd import functional as F
    mq, mr = d.shape
    q_ids = torch.arange(mq, dtype=torch.int64, device='cuda') if skip else None
    best = None
    for at, step in steps:
        part = torch.from_numpy(np.ascontiguousarray(d[:, at:at + step])).cuda()
        best = F.nearest_rows(part, k, r_base=at, q_ids=q_ids, best=best)
    return best[0].cpu(), best[1].cpu()


@pytest.mark.parametrize('k', [1, 3, 16])
@pytest.mark.parametrize('skip', [False, True])
def test_topk_ties_tails_chunks_and_own_id(k, skip):
    rng = np.random.default_rng(5)
    mq, mr = 9, 11
    d = rng.integers(0, 4, size=(mq, mr)).astype(np.int64)      # repeated values: ties everywhere
    d[np.arange(mq), np.arange(mq)] = 0
    d[3] = 5
    d[3, 3] = 0      # the own id is the only zero-distance candidate of row 3
    want_d, want_i = memref.nearest(d, k, skip_self=skip)
    results = []
    for step in (1, 3, mr):
        bd, bi = _merge(d, k, [(at, step) for at in range(0, mr, step)], skip)
        for i in range(mq):
            n = len(want_d[i])
            assert bd[i, :n].tolist() == want_d[i] and bi[i, :n].tolist() == want_i[i], (step, i)
            assert (bd[i, n:] == I64_MAX).all() and (bi[i, n:] == -1).all()      # k past the candidates: the tails stay empty
        results.append((bd, bi))
    assert all(torch.equal(r[0], results[0][0]) and torch.equal(r[1], results[0][1]) for r in results)
    if skip:
        assert results[0][1][3, 0] == 0 and results[0][0][3, 0] == 5 and not (results[0][1] == torch.arange(mq)[:, None]).any()
    else:
        assert results[0][1][3, 0] == 3 and results[0][0][3, 0] == 0


def test_topk_many_candidates_and_large_ids():
    rng = np.random.default_rng(9)
    d = rng.integers(0, 50, size=(5, 700)).astype(np.int64)
    d[0] = 2 ** 62
    d[1, ::2] = 0
    want_d, want_i = memref.nearest(d, 16)
    bd, bi = _merge(d, 16, [(0, 130), (130, 1), (131, 569)], False)
    assert bd.tolist() == want_d and bi.tolist() == want_i
    from saragan_amd import functional as F
    far = F.nearest_rows(torch.from_numpy(d[:, :3].copy()).cuda(), 2, r_base=2 ** 40)
    assert far[1].cpu().tolist() == [[2 ** 40 + j for j in memref.nearest(d[:, :3], 2)[1][i]] for i in range(5)]


def test_topk_contract_errors():
    lib = _lib()
    d = torch.zeros((2, 3), dtype=torch.int64, device='cuda')
    bd = torch.full((2, 16), -7, dtype=torch.int64, device='cuda')
    bi = torch.full((2, 16), -7, dtype=torch.int64, device='cuda')
    st = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: C_.c_void_p(x) if x else None
    D, BD, BI = d.data_ptr(), bd.data_ptr(), bi.data_ptr()
    for args, code in [((D, 2, 3, 0, 0, 0, BD, BI), SG_EINVAL), ((D, 2, 3, 0, 0, 17, BD, BI), SG_EINVAL),
                       ((D, 2, 3, 0, 0, -1, BD, BI), SG_EINVAL), ((0, 2, 3, 0, 0, 3, BD, BI), SG_EINVAL),
                       ((D, 2, 3, 0, 0, 3, 0, BI), SG_EINVAL), ((D, 2, 3, 0, 0, 3, BD, 0), SG_EINVAL),
                       ((D, 0, 3, 0, 0, 3, BD, BI), SG_EINVAL), ((D, 2, 0, 0, 0, 3, BD, BI), SG_EINVAL),
                       ((D, 2, 3, -1, 0, 3, BD, BI), SG_EINVAL), ((D + 4, 2, 3, 0, 0, 3, BD, BI), SG_EALIGN),
                       ((D, 2, 3, 0, 0, 3, BD + 4, BI), SG_EALIGN), ((D, 2, 3, 0, BD + 4, 3, BD, BI), SG_EALIGN)]:
        a = args
        assert lib.sg_topk_merge(p(a[0]), a[1], a[2], a[3], p(a[4]), a[5], p(a[6]), p(a[7]), st) == code, args
    torch.cuda.synchronize()
    assert (bd == -7).all() and (bi == -7).all()
