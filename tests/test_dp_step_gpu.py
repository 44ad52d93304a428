"""The data-parallel training step on more than one rank, for everything that only happens when world_size > 1: gscale =
1 / world through every update rule, the clip and the norms; hook-launched small buckets that parameters straddle; the
reduce-scatter + all-gather form; bf16 gradients on the wire; `alternate` with a reducer; the Adasum delta form.

Conventions of tests/test_dp_gpu.py: `spawn` context, gloo, every rank on cuda:0, InjectedRandom sliced per rank, the halves
of a golden fixture's batch as the ranks' batches, rank 0 loads p0 and broadcast_global_variables spreads it, f32, reproducible
mode.  One set of workers runs a whole group of variants in sequence (each with a fresh store, optimisers and step graph inside
the same process group); the parent replays the oracle in fp64 and asserts, one test id per variant.

Group A (averaging reducer): the losses are batch means (tests/test_dp_premise_host.py), so the expected result is the oracle's
FULL-batch step.  Group B (Adasum): the reference is assembled from the oracle's per-rank steps.  Tolerances are those of each
variant's single-process twin (tests/test_step_gpu.py, tests/test_lamb_step_gpu.py, tests/test_configs_gpu.py)."""
import argparse
import hashlib
import os
import queue
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import dpref

pytestmark = pytest.mark.gpu

P3_WGAN, P2_MIX, P3_LOGISTIC = 'oracle_step_p3_wgan_a000.npz', 'oracle_step_p2_wgan_a060.npz', 'oracle_step_p3_logistic_a025.npz'
MANY, ODD, FINE = 4096, 4 * 1023, 1024      # bucket_bytes: 16 buckets per network; an odd element count; 14+ buckets of a frozen step
SPLIT = 4 * 211                             # bucket boundaries INSIDE five bias vectors of the phase-3 networks (see `bias_split`)


def _v(vid, fixture=P3_WGAN, kind='Adam', strategy='simultaneous', steps=2, bucket=MANY, **kw):
    return dict(dict(id=vid, fixture=fixture, kind=kind, d_kind=kind, strategy=strategy, steps=steps, bucket=bucket, clip=False,
                     scale=1.0, fetch=False, freeze=False, algo='allreduce', wire='f32', d_op='Average'), **kw)


GROUPS = {
    'adam': (2, [
        _v('buckets'),
        _v('rs_ag', algo='rs_ag', bucket=ODD),
        _v('bias_split', bucket=SPLIT),
        _v('fetch', fetch=True),
        _v('clip', fetch=True, clip=True, scale=1.5),
        _v('mix_wgan', fixture=P2_MIX, freeze=True, bucket=FINE),
        _v('mix_logistic', fixture=P3_LOGISTIC, freeze=True, bucket=FINE),
        _v('bf16_wire', wire='bf16', fetch=True, steps=1),
    ]),
    'rules': (2, [_v('alt_wgan_mix', fixture=P2_MIX, strategy='alternate', freeze=True, fetch=True, bucket=FINE),
                  _v('alt_logistic', fixture=P3_LOGISTIC, strategy='alternate', freeze=True, fetch=True, bucket=FINE)]
              + [_v(f'{k}_{s}', kind=k, strategy=s, steps=3, clip=s == 'simultaneous')
                 for k in ('SGD', 'Momentum', 'Adadelta') for s in ('simultaneous', 'alternate')]),
    'lamb': (2, [_v(f'{k}_{s}', kind=k, strategy=s, steps=3) for k in ('LAMB', 'AdamW') for s in ('simultaneous', 'alternate')]),
    'adasum2': (2, [_v('adasum_sgd', d_kind='SGD', d_op='Adasum'), _v('adasum_adam', d_op='Adasum')]),
    'adasum4': (4, [_v('adasum_sgd', d_kind='SGD', d_op='Adasum')]),
}


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ----------------------------------------------------------------------------------------------------------------------
# the ranks
# ----------------------------------------------------------------------------------------------------------------------
def _run_variant(v, rank, world, golden):
    import saragan_amd.optimization as opt
    from saragan_amd import parallel
    from saragan_amd.ExtendedEMA import ExtendedEMA
    from saragan_amd.networks import loss as L
    from saragan_amd.networks.ops import ScalarVariable
    from saragan_amd.networks.pgan.discriminator import discriminator
    from saragan_amd.networks.pgan.generator import generator
    from saragan_amd.varstore import VariableStore, set_compute_dtype, use_store
    from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT, load_step_fixture
    os.environ['SARAGAN_DP_ALGO'] = v['algo']            # (read when a reducer is made)
    os.environ['SARAGAN_DP_GRAD_DTYPE'] = v['wire']
    fx = load_step_fixture(os.path.join(golden, v['fixture']), torch.float64)
    n = fx['real'].shape[0] // world
    sl = slice(rank * n, (rank + 1) * n)
    set_compute_dtype(torch.float32)
    store = VariableStore('cuda', seed=100 + rank)
    L.set_random_source(L.InjectedRandom({k: t[sl].float() for k, t in fx['rnd'].items()}))
    ns = argparse.Namespace(optimizer=v['kind'], d_optimizer=v['d_kind'], adam_beta1=0.0, adam_beta2=0.9, d_adam_beta1=0.0,
                            d_adam_beta2=0.9, rho=0.9, d_rho=0.9, momentum=0.8, d_momentum=0.8, weight_decay=dpref.DECAY,
                            d_weight_decay=dpref.DECAY)
    og, od = opt.get_optimizer(ScalarVariable(dpref.LR[v['d_kind']], 'd_lr'), ScalarVariable(dpref.LR[v['kind']], 'g_lr'), ns)
    og = parallel.DistributedOptimizer(og, bucket_bytes=v['bucket'])
    od = parallel.DistributedOptimizer(od, bucket_bytes=v['bucket'], op=getattr(parallel, v['d_op']))
    ph = opt.Placeholder([n, 1, 1, 1, 1])
    freeze = list(fx['freeze']) if v['freeze'] and fx['freeze'] is not None else None
    with use_store(store):
        tup = opt.optimize_step(og, od, generator, discriminator, ph, LATENT, ScalarVariable(fx['alpha'], 'alpha'), fx['phase'],
                                BASE_SHAPE, KERNEL_SPEC, FILTER_SPEC, 'leaky_relu', 0.2, fx['loss_fn'], fx['cfg']['gp_weight'],
                                v['strategy'], v['clip'], v['clip'], 0.01, freeze)
    if rank == 0:                                       # the other ranks keep different weights until the broadcast
        store.load_state_dict(dpref.scaled_p0(fx, v['scale']), strict=True)
    graph = tup[0].graph
    ema = ExtendedEMA(list(store.vars), 0.99, graph=graph)
    graph._ensure_flat()
    parallel.broadcast_global_variables(store, 0)
    ema.reset_to_variables()
    # what each averaging reducer is armed with: the number of ranges, and the parameters begin() counts as done because
    # the graph below `roots` does not reach them
    info = {}
    for net, o in (('generator', og), ('discriminator', od)):
        red = o.distributed
        if isinstance(red, parallel.AdasumReducer):
            continue
        info[net] = dict(nranges=0, unreached=0)

        def begin(flat_grad, ranges, params, roots=None, _red=red, _rec=info[net], _begin=red.begin):
            _rec['nranges'] = max(_rec['nranges'], len(ranges))
            if roots is not None:
                reach = parallel.reachable_leaves(roots)
                _rec['unreached'] = max(_rec['unreached'], sum(id(p) not in reach for p in params))
            return _begin(flat_grad, ranges, params, roots)
        red.begin = begin
    fz = freeze is not None
    tg, td = (tup[12], tup[16]) if fz else (tup[0], tup[1])
    handles = [tg, td, tup[2], tup[3]]
    if v['fetch']:
        handles += [tup[13], tup[17], tup[15], tup[19]] if fz else [tup[6], tup[8], tup[10], tup[11]]
    gv, dv = (tup[14], tup[18]) if fz else (tup[7], tup[9])
    sess = opt.Session('cuda')
    feed = {ph: fx['real'][sl].float()}
    rec = dict(steps=[], info=info)
    for step in range(v['steps']):
        got = sess.run(handles if step == 0 else handles[:4], feed_dict=feed)
        if step == 0:
            if v['wire'] == 'bf16':      # the reduced sums, before anything scales them: every element is a bf16 value
                for prefix in ('generator/', 'discriminator/'):
                    g = store.flat[prefix]['grad']
                    assert int((g.view(torch.int32) & 0xFFFF).count_nonzero()) == 0 and int(g.count_nonzero()) > 0, prefix
            if v['fetch']:
                rec['g_grads'] = {h.key: g.detach().cpu().numpy().copy() for h, g in zip(gv, got[4])}
                rec['d_grads'] = {h.key: g.detach().cpu().numpy().copy() for h, g in zip(dv, got[5])}
                rec['max_norm'] = (float(got[6]), float(got[7]))
        sess.run(ema.apply())
        rec['steps'].append(dict(gl=float(got[2]), dl=float(got[3]),
                                 w={k: p.detach().cpu().numpy().copy() for k, p in store.vars.items()},
                                 ema={k: ema.average(k).detach().cpu().numpy().copy() for k in store.vars}))
    torch.cuda.synchronize()
    for net, o in (('generator', og), ('discriminator', od)):
        red = o.distributed
        assert red.world_size == world and red.algo == v['algo'] and red.grad_dtype == v['wire']
        if net in info:
            # small buckets: many per network, and at least one parameter in two of them
            assert len(red._buckets) >= 8, (v['id'], net, len(red._buckets))
            assert any(len(b) > 1 for b in red._owner.values()), (v['id'], net)
            assert all(b['launched'] for b in red._buckets)
            info[net]['buckets'] = len(red._buckets)
            info[net]['tails'] = sum(1 for b in red._buckets if b['len'] % world)
            if v['algo'] == 'rs_ag':
                assert info[net]['tails'] >= 1, (v['id'], net)      # the tail all-reduce of _launch_rs_ag was taken
    h = hashlib.sha256()
    for s in rec['steps']:
        for part in (s['w'], s['ema']):
            for k in sorted(part):
                h.update(part[k].tobytes())
    for key in ('g_grads', 'd_grads'):
        for k in sorted(rec.get(key, {})):
            h.update(rec[key][k].tobytes())
    rec['digest'] = h.hexdigest()
    return rec


def _worker(rank, world, port, golden, q, variants, backend):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank) if backend == 'nccl' else '0', SARAGAN_DIST_BACKEND=backend,
                      HSA_ENABLE_IPC_MODE_LEGACY='0', SARAGAN_DP_TIMING='1')
    import saragan_amd
    from saragan_amd import parallel
    parallel.init_distributed()
    saragan_amd.set_deterministic(True)
    out = {}
    for v in variants:
        rec = _run_variant(v, rank, world, golden)
        out[v['id']] = rec if rank == 0 else dict(digest=rec['digest'])      # rank 0 returns the results
    q.put((rank, out))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


_RESULTS = {}


def _group(golden, group, backend='gloo'):
    """{variant id: rank 0's record, with the other ranks' digests}: the group's workers run once per session."""
    key = (group, backend)
    if key not in _RESULTS:
        try:
            _RESULTS[key] = _spawn(golden, group, backend)
        except BaseException as e:      # no retry: every variant of the group reports the one failure
            _RESULTS[key] = e
    if isinstance(_RESULTS[key], BaseException):
        raise _RESULTS[key]
    return _RESULTS[key]


def _spawn(golden, group, backend):
    import time
    world, variants = GROUPS[group]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, golden, q, variants, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    deadline = time.monotonic() + 180 + 20 * len(variants)
    try:
        while len(res) < world:
            try:
                r, out = q.get(timeout=1)
                res[r] = out
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f'group {group}: a worker exited with {dead}'
                assert time.monotonic() < deadline, f'group {group}: no result within the time limit'
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0, f'group {group}: worker exit code {p.exitcode}'
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    for v in variants:
        res[0][v['id']]['digests'] = [res[r][v['id']]['digest'] for r in range(world)]
    return res[0]


# ----------------------------------------------------------------------------------------------------------------------
# the parent's checks
# ----------------------------------------------------------------------------------------------------------------------
def _fixture(golden, v):
    from tests.stepfix import load_step_fixture
    return load_step_fixture(os.path.join(golden, v['fixture']), torch.float64)


def _variant(group, vid):
    return next(v for v in GROUPS[group][1] if v['id'] == vid)


def _replicas_identical(rec):
    assert len(set(rec['digests'])) == 1, rec['digests']


def _report(what, worst):
    print(f'{what}: worst |err| / bound = {worst[0]:.3f} ({worst[1]}, |err| {worst[2]:.3e})')


def _close(got, want, what, rtol=1e-4, atol=2e-5):
    worst = (0.0, None, 0.0)
    for k, ref in want.items():      # (each figure is printed before anything is asserted)
        err = np.abs(got[k].astype(np.float64) - ref.numpy())
        ratio = float((err / (atol + rtol * np.abs(ref.numpy()))).max())
        worst = max(worst, (ratio, k, float(err.max())))
    _report(what, worst)
    for k, ref in want.items():
        np.testing.assert_allclose(got[k].astype(np.float64), ref.numpy(), rtol=rtol, atol=atol, err_msg=f'{what} {k}')


def _grads_close(got, want, what, rtol=1e-3):
    assert list(got) == list(want)
    worst = (0.0, None, 0.0)
    for k, ref in want.items():
        r = ref.numpy()
        err = np.abs(got[k].astype(np.float64) - r)
        worst = max(worst, (float((err / (1e-4 * np.abs(r).max() + 1e-9 + rtol * np.abs(r))).max()), k, float(err.max())))
    _report(what, worst)
    for k, ref in want.items():
        r = ref.numpy()
        np.testing.assert_allclose(got[k].astype(np.float64), r, rtol=rtol, atol=1e-4 * np.abs(r).max() + 1e-9, err_msg=f'{what} {k}')


def _frozen_untouched(rec, fx):
    for k in fx['freeze']:
        if k in rec['steps'][-1]['w']:
            for s in rec['steps']:      # quirk Q4: previous-phase variables are not updated while alpha > 0
                np.testing.assert_array_equal(s['w'][k], fx['p0'][k].float().numpy(), err_msg=k)


ADAM = ['buckets', 'rs_ag', 'bias_split', 'fetch', 'clip', 'mix_wgan', 'mix_logistic']


def _check_adam_variant(golden_dir, vid, backend='gloo'):
    v = _variant('adam', vid)
    rec = _group(golden_dir, 'adam', backend)[vid]
    fx = _fixture(golden_dir, v)
    _replicas_identical(rec)
    if v['clip']:
        p0 = dpref.scaled_p0(fx, v['scale'])
        probe = dpref.oracle_run(fx, 'simultaneous', 'Adam', 1, p0=p0)[0]['out']
        gn = {k: float(torch.sqrt(sum((g * g).sum() for g in probe[k].values()))) for k in ('g_grads', 'd_grads')}
        assert gn['d_grads'] > 1.0 and gn['g_grads'] > 1.0, gn      # the clip bites, for both networks
        ref = dpref.oracle_run(fx, 'simultaneous', 'Adam', v['steps'], p0=p0, clip=True)
        want = [(r['p'], r['shadow']) for r in ref]
        out = ref[0]['out']
        atol, grtol = 2e-5, 2e-3      # (test_global_norm_clipping_matches_oracle's)
    else:
        want = [(fx['p1'], fx['ema1']), (fx['p2'], fx['ema2'])]
        out = dict(g_grads=fx['gg'], d_grads=fx['dg'])
        atol, grtol = (3e-5 if v['fixture'] == P3_WGAN else 2e-5), 1e-3      # (the two-rank twin's, test_step_matches_oracle_fp32's)
    for s, (p, sh) in enumerate(want):
        _close(rec['steps'][s]['w'], p, f'{vid} step {s} weight', atol=atol)
        _close(rec['steps'][s]['ema'], sh, f'{vid} step {s} ema', atol=atol)
    if v['fetch']:      # hvd.DistributedOptimizer.compute_gradients returns AVERAGED gradients, clipped or not
        _grads_close(rec['g_grads'], out['g_grads'], f'{vid} G gradient', grtol)
        _grads_close(rec['d_grads'], out['d_grads'], f'{vid} D gradient', grtol)
        np.testing.assert_allclose(rec['max_norm'][0], dpref.max_var_norm(out['g_grads']), rtol=1e-3)
        np.testing.assert_allclose(rec['max_norm'][1], dpref.max_var_norm(out['d_grads']), rtol=1e-3)
    if v['freeze']:
        _frozen_untouched(rec, fx)
    return rec


@pytest.mark.parametrize('vid', ADAM)
def test_adam_step_at_world_2_equals_full_batch_oracle(golden_dir, vid):
    """A1-A5.  buckets / rs_ag: 16 buckets per network, parameters straddling them; rs_ag with an odd bucket size so that every
    bucket takes the tail all-reduce.  bias_split: a weight's last bucket also holds its layer's bias, whose gradient the same
    backward node writes, so a bucket that forgot the straddling weight would still go out late enough; a bias cut by a
    boundary shares its second bucket with the NEXT layer's weight, which backward finishes first -- only there does a plan
    that registers a straddling parameter with its first bucket alone send a bucket out before its gradient is there (the replicas then differ).
    fetch / clip: the fetched gradients are the full-batch (averaged) ones and max_norm is
    their largest per-variable norm, without clipping (gscale^2 in the norms) and with it (scale * gscale in the clip).
    mix_*: the *_fz train ops.  The frozen variables come first in the flat buffers, so begin() is given ONE range, and while
    alpha is inside (0, 1) every trained parameter is reached: neither several ranges nor the `roots` shortcut occurs in a
    mixing step.  The shortcut is taken in the stabilising fixture (alpha = 0: the faded to_rgb / from_rgb branch), which the
    `buckets` variant asserts."""
    rec = _check_adam_variant(golden_dir, vid)
    info = rec['info']
    if vid == 'buckets':
        assert info['generator']['unreached'] + info['discriminator']['unreached'] >= 1, info
    if vid.startswith('mix'):
        assert all(i['nranges'] == 1 and i['unreached'] == 0 for i in info.values()), info


def test_adam_variants_over_rccl(golden_dir):
    """The same variants with one device per rank on RCCL (in-order queues: the all-gather is issued behind its reduce-scatter
    without a host wait)."""
    if torch.cuda.device_count() < 2:
        pytest.skip('RCCL needs one device per rank: fewer than 2 GPUs here (the 8-GPU node runs this variant)')
    for vid in ADAM:
        _check_adam_variant(golden_dir, vid, 'nccl')


def test_bf16_wire_gradients_within_the_collective_bound(golden_dir):
    """A9.  SARAGAN_DP_GRAD_DTYPE=bf16: the worker asserts that every reduced element is a bf16 value; the fetched gradients lie
    within world * 2^-8 * sum_r |g_r| (the bound tests/test_dp_gloo.py derives for the collective) plus the f32 gradient
    tolerance of sum_r g_r / world, g_r the oracle's gradients of rank r's half batch; replicas identical; and the result is
    not the f32-wire one."""
    world = 2
    v = _variant('adam', 'bf16_wire')
    res = _group(golden_dir, 'adam')
    rec, f32 = res['bf16_wire'], res['fetch']
    fx = _fixture(golden_dir, v)
    _replicas_identical(rec)
    parts = [dpref.oracle_run(fx, 'simultaneous', 'Adam', 1, rank=r, world=world)[0]['out'] for r in range(world)]
    differs = False
    for key in ('g_grads', 'd_grads'):
        assert list(rec[key]) == list(parts[0][key])
        for k, got in rec[key].items():
            mean = sum(p[key][k] for p in parts).numpy() / world
            mag = sum(p[key][k].abs() for p in parts).numpy()
            bound = world * 2.0 ** -8 * mag + 1e-3 * np.abs(mean) + 1e-4 * np.abs(mean).max() + 1e-9
            err = np.abs(got.astype(np.float64) - mean)
            assert np.all(err <= bound), (key, k, float((err - bound).max()))
            differs = differs or not np.array_equal(got, f32[key][k])
    assert differs


RULES_VARIANTS = [v['id'] for v in GROUPS['rules'][1]]


@pytest.mark.parametrize('vid', RULES_VARIANTS)
def test_alternate_and_the_fused_rules_at_world_2(golden_dir, vid):
    """A6: `alternate` with a reducer attached (never captured): D's reduction has finished before the G forward reads the
    updated D.  A7: SGD / Momentum (Nesterov) / Adadelta, three steps; `simultaneous` clips (scale * gscale), `alternate` does
    not, so gscale = 0.5 reaches sg_optim_step."""
    v = _variant('rules', vid)
    rec = _group(golden_dir, 'rules')[vid]
    fx = _fixture(golden_dir, v)
    _replicas_identical(rec)
    freeze = fx['freeze'] if v['freeze'] else None
    ref = dpref.oracle_run(fx, v['strategy'], v['kind'], v['steps'], freeze=freeze, clip=v['clip'])
    if v['kind'] == 'Adam':
        rtol, atol = 1e-4, 2e-5                                   # test_alternate_step_matches_oracle_fp32
    else:
        rtol, atol = 2e-4, (1e-4 if v['kind'] == 'Adadelta' else 2e-5)      # test_other_optimizers_match_oracle
    for s, r in enumerate(ref):
        _close(rec['steps'][s]['w'], r['p'], f'{vid} step {s} weight', rtol, atol)
        _close(rec['steps'][s]['ema'], r['shadow'], f'{vid} step {s} ema', rtol, atol)
    if v['fetch']:
        _grads_close(rec['g_grads'], ref[0]['out']['g_grads'], f'{vid} G gradient')
        _grads_close(rec['d_grads'], ref[0]['out']['d_grads'], f'{vid} D gradient')
    if freeze is not None:
        _frozen_untouched(rec, fx)


LAMB_VARIANTS = [v['id'] for v in GROUPS['lamb'][1]]


@pytest.mark.parametrize('vid', LAMB_VARIANTS)
def test_lamb_and_adamw_at_world_2(golden_dir, vid):
    """A8: no clipping, so gscale = 0.5 reaches sg_adamw_ema and the sg_lamb_moments / ratios / update chain (the trust-ratio
    norms see the averaged gradient).  The three-run bound of tests/test_lamb_step_gpu.py: rtol 2e-4, atol 2e-5, plus the
    distance between the exact oracle and the oracles whose rules read f32 gradients."""
    v = _variant('lamb', vid)
    rec = _group(golden_dir, 'lamb')[vid]
    fx = _fixture(golden_dir, v)
    _replicas_identical(rec)
    runs = [dpref.oracle_run(fx, v['strategy'], v['kind'], v['steps'], f32_error=e) for e in (None, 1, -1)]
    for s in range(v['steps']):
        for what, key in (('p', 'w'), ('shadow', 'ema')):
            for k, want in runs[0][s][what].items():
                err = np.abs(rec['steps'][s][key][k].astype(np.float64) - want.numpy())
                dist = torch.maximum((want - runs[1][s][what][k]).abs(), (want - runs[2][s][what][k]).abs()).numpy()
                over = err - (2e-5 + 2e-4 * np.abs(want.numpy()) + dist)
                assert np.all(over <= 0), (f'{vid} step {s} {what} {k}: {int((over > 0).sum())} of {err.size} elements outside '
                                           f'the bound, worst |err| {float(err.flat[over.argmax()]):.3e}')


def _adasum_reference(fx, v, world):
    """Step 1: G from the full-batch step; D = p0 + Adasum over ranks of (p_r - p0), p_r the oracle's LOCAL step on rank r's
    slice with fresh rule state; D's shadow sees the combined weights."""
    from tests.test_dp_gloo import _adasum_numpy
    full = dpref.oracle_run(fx, 'simultaneous', v['kind'], 1, d_kind=v['d_kind'])[0]
    local = [dpref.oracle_run(fx, 'simultaneous', v['kind'], 1, d_kind=v['d_kind'], rank=r, world=world)[0]['p'] for r in range(world)]
    p, shadow = dict(full['p']), dict(full['shadow'])
    for k, start in fx['p0'].items():
        if k.startswith('discriminator/'):
            deltas = [(lp[k] - start).numpy().reshape(-1) for lp in local]
            comb = torch.from_numpy(_adasum_numpy(deltas, [(0, deltas[0].size)])).reshape(start.shape)
            p[k] = start + comb
            shadow[k] = 0.99 * start + 0.01 * p[k]
    return p, shadow


def _check_adasum(golden_dir, group, vid):
    from tests.cfgutil import assert_adam_close
    world = GROUPS[group][0]
    v = _variant(group, vid)
    rec = _group(golden_dir, group)[vid]
    fx = _fixture(golden_dir, v)
    _replicas_identical(rec)
    assert 'discriminator' not in rec['info'] and rec['info']['generator']['buckets'] >= 8
    p, shadow = _adasum_reference(fx, v, world)
    got = rec['steps'][0]
    for k in p:
        if k.startswith('generator/'):      # the averaged half: as in group A
            np.testing.assert_allclose(got['w'][k], p[k].numpy(), rtol=1e-4, atol=3e-5, err_msg=k)
            np.testing.assert_allclose(got['ema'][k], shadow[k].numpy(), rtol=1e-4, atol=3e-5, err_msg=k)
        elif v['d_kind'] == 'SGD':          # the deltas are smooth in the gradient: SGD's tolerance
            np.testing.assert_allclose(got['w'][k], p[k].numpy(), rtol=2e-4, atol=2e-5, err_msg=k)
            np.testing.assert_allclose(got['ema'][k], shadow[k].numpy(), rtol=2e-4, atol=2e-5, err_msg=k)
        else:                               # a first Adam step is -lr * sign(g) (tests/test_configs_gpu.py)
            assert_adam_close(got['w'][k], p[k], 1e-3, 1e-4, k)
            assert_adam_close(got['ema'][k], shadow[k], 1e-3 * 0.01, 1e-4, 'ema:' + k)
    # the combined weights were written behind the packed weight images: rank 0's second step must read them.  Its losses
    # are those of the oracle on rank 0's slice at the reference weights -- and not those with D left at p0.
    rnd, real = dpref.rank_batch(fx, 0, world)
    fresh = lambda: (dpref.make_rule(v['kind']), dpref.make_rule(v['d_kind']))
    second = dpref.oracle_step(dict(p), *fresh(), None, fx, 'simultaneous', rnd, real)
    stale = dpref.oracle_step({k: (fx['p0'][k] if k.startswith('discriminator/') else t) for k, t in p.items()}, *fresh(), None,
                              fx, 'simultaneous', rnd, real)
    for key, name in (('gl', 'gen_loss'), ('dl', 'disc_loss')):
        np.testing.assert_allclose(rec['steps'][1][key], float(second[name]), rtol=1e-4, atol=1e-5, err_msg=name)
    # (gen_loss = -mean D(fake) is the one that tells: with D left at p0 it lies 50 tolerances away, disc_loss under one)
    assert abs(float(stale['gen_loss']) - float(second['gen_loss'])) > 10 * (1e-4 * abs(float(second['gen_loss'])) + 1e-5)


@pytest.mark.parametrize('vid', ['adasum_sgd', 'adasum_adam'])
def test_adasum_delta_form_at_world_2(golden_dir, vid):
    """B: D under op=Adasum (clone start, local rule step, combine_deltas, EMA left to ExtendedEMA.apply), G averaged."""
    _check_adasum(golden_dir, 'adasum2', vid)


def test_adasum_delta_form_at_world_4(golden_dir):
    """One sample per rank: the pairing tree ((0,1), (2,3)), then the pair of pairs."""
    _check_adasum(golden_dir, 'adasum4', 'adasum_sgd')
