"""Non-finite step guard (saragan_amd.set_nonfinite_guard, SARAGAN_NONFINITE_GUARD=1): the all-finite flag kernels, the
guarded optimiser launches and the bookkeeping thread, then whole steps -- eager, replayed from a hipGraph, with clipping,
over two data-parallel ranks, and the training loop's stop after N consecutive skips.  With the guard, a train op whose
gradient holds a NaN / Inf leaves its network's parameters, optimiser slots and step count as they were (the EMA update
still runs); with it off, one bad batch poisons the discriminator (the behaviour the guard exists to stop)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
NAME = 'oracle_step_p3_wgan_a000.npz'


def _flag():
    return torch.zeros(1, dtype=torch.int32, device='cuda')


# ---------------------------------------------------------------------------------------------------------------------
# 1. the flag kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 4, 1023, 2 ** 22 + 5])
def test_flag_equals_isfinite_all(n):
    from saragan_amd import functional as F
    x = torch.randn(n, device='cuda')
    where = {0, n - 1}
    if n % 4:
        where.add(n - n % 4)                 # first entry of the numel % 4 tail
    flag, fused = _flag(), _flag()
    bounds = torch.tensor([0, n // 2, n] if n > 1 else [0, n], dtype=torch.int64, device='cuda')
    nseg = bounds.numel() - 1
    F.nonfinite_flag_(flag, x)
    assert int(flag) == 0
    for i in sorted(where):
        for bad in (float('nan'), float('inf'), float('-inf')):
            keep = x[i].item()
            x[i] = bad
            F.nonfinite_flag_(flag, x)
            sq = F.segment_sumsq(x, bounds, nseg, flag=fused)
            assert int(flag) == int(not bool(torch.isfinite(x).all())) == 1, (n, i, bad)
            assert int(fused) == 1, (n, i, bad)
            x[i] = keep
            F.nonfinite_flag_(flag, x)
            sq = F.segment_sumsq(x, bounds, nseg, flag=fused)
            assert int(flag) == 0 and int(fused) == 0, (n, i, bad)
    # the fused pass computes exactly the plain sums of squares
    assert torch.equal(sq, F.segment_sumsq(x, bounds, nseg))


def test_flag_accumulates_over_ranges():
    from saragan_amd import functional as F
    a, b = torch.randn(64, device='cuda'), torch.randn(37, device='cuda')
    b[36] = float('nan')
    flag = _flag()
    F.nonfinite_flag_(flag, b)
    F.nonfinite_flag_(flag, a, accumulate=True)           # a finite second range keeps the first one's verdict
    assert int(flag) == 1
    F.nonfinite_flag_(flag, a)                            # a fresh test clears it
    assert int(flag) == 0


def test_huge_and_subnormal_values_are_finite():
    from saragan_amd import functional as F
    x = torch.full((4099,), 3e38, device='cuda')
    x[1::3] = -3e38
    x[2::5] = 1e-45                                       # subnormal
    x[7] = torch.finfo(torch.float32).max
    flag, fused = _flag(), _flag()
    F.nonfinite_flag_(flag, x)
    bounds = torch.tensor([0, x.numel()], dtype=torch.int64, device='cuda')
    sq = F.segment_sumsq(x, bounds, 1, flag=fused)
    assert not torch.isfinite(sq).all()                   # the norm overflows ...
    assert int(flag) == 0 and int(fused) == 0             # ... the gradient is still finite


# ---------------------------------------------------------------------------------------------------------------------
# 2. guarded updates and the bookkeeping thread
# ---------------------------------------------------------------------------------------------------------------------
N = 1027          # vector body + a 3-entry tail


def _bufs(seed, slots):
    g = torch.Generator(device='cuda').manual_seed(seed)
    r = lambda: torch.randn(N, device='cuda', generator=g)
    return dict(p=r(), g=r(), ema=r(), **{s: r().abs() for s in slots})


def _clone(d):
    return {k: v.clone() for k, v in d.items()}


def test_guarded_adam_flag_set_is_ema_only():
    from saragan_amd import functional as F
    b = _bufs(1, ('m', 'v'))
    b['g'][5] = float('nan')
    ref = _clone(b)
    lr_t = torch.tensor([1e-3], device='cuda')
    flag = F.nonfinite_flag_(_flag(), b['g'])
    F.adam_ema_(b['p'], b['g'], b['m'], b['v'], b['ema'], 0.0, 0.0, 0.9, 0, 1e-8, 1.0, 0.99, lr_dev=lr_t, skip=flag)
    for k in ('p', 'm', 'v'):
        assert torch.equal(b[k], ref[k]), k
    F.adam_ema_(ref['p'], None, None, None, ref['ema'], 0.0, 0.0, 0.9, 1, ema_decay=0.99)      # the existing EMA-only launch
    assert torch.equal(b['ema'], ref['ema'])


def test_guarded_adam_flag_clear_matches_dev_launch():
    from saragan_amd import functional as F
    b = _bufs(2, ('m', 'v'))
    ref = _clone(b)
    lr_t = torch.tensor([F.adam_step_size(1e-3, 0.5, 0.9, 3)], device='cuda')
    flag = F.nonfinite_flag_(_flag(), b['g'])
    assert int(flag) == 0
    F.adam_ema_(b['p'], b['g'], b['m'], b['v'], b['ema'], 0.0, 0.5, 0.9, 0, 1e-8, 0.5, 0.99, lr_dev=lr_t, skip=flag)
    F.adam_ema_(ref['p'], ref['g'], ref['m'], ref['v'], ref['ema'], 0.0, 0.5, 0.9, 0, 1e-8, 0.5, 0.99, lr_dev=lr_t)
    for k in b:
        assert torch.equal(b[k], ref[k]), k


def test_guarded_adam_ok_skip_ok_equals_two_updates():
    """Bias correction counts APPLIED updates: [ok, skip, ok] == the unguarded updates at t = 1, 2."""
    from saragan_amd import functional as F
    b1, b2, lr = 0.5, 0.9, 1e-3
    b = _bufs(3, ('m', 'v'))
    ref = _clone(b)
    g1, g3 = b['g'].clone(), torch.randn(N, device='cuda')
    g2 = g1.clone()
    g2[N - 1] = float('inf')
    flag, t = _flag(), torch.zeros(1, dtype=torch.int64, device='cuda')
    cnt, lr_t = torch.zeros(3, dtype=torch.int64, device='cuda'), torch.zeros(1, device='cuda')
    for g in (g1, g2, g3):
        F.nonfinite_flag_(flag, g)
        F.guard_step_(flag, t, cnt, lr, lr_t, adam=(b1, b2))
        F.adam_ema_(b['p'], g, b['m'], b['v'], b['ema'], 0.0, b1, b2, 0, 1e-8, 1.0, 0.99, lr_dev=lr_t, skip=flag)
        if g is g2:
            assert cnt.tolist() == [1, 1, 1] and int(t) == 1
    assert int(t) == 2 and cnt.tolist() == [1, 0, 1]
    assert lr_t.item() == np.float32(F.adam_step_size(lr, b1, b2, 2))     # double arithmetic, then one rounding
    F.adam_ema_(ref['p'], g1, ref['m'], ref['v'], ref['ema'], lr, b1, b2, 1, 1e-8, 1.0, 0.99)
    F.adam_ema_(ref['p'], None, None, None, ref['ema'], lr, b1, b2, 1, ema_decay=0.99)          # the skipped step's EMA
    F.adam_ema_(ref['p'], g3, ref['m'], ref['v'], ref['ema'], lr, b1, b2, 2, 1e-8, 1.0, 0.99)
    for k in ('p', 'm', 'v', 'ema'):
        assert torch.equal(b[k], ref[k]), k


@pytest.mark.parametrize('kind,slots,hyper', [('SGD', (), dict(h=0.0, eps=0.0, nesterov=False)),
                                              ('MOMENTUM', ('accum',), dict(h=0.9, eps=0.0, nesterov=True)),
                                              ('ADADELTA', ('accum', 'accum_update'), dict(h=0.95, eps=1e-7, nesterov=False))])
def test_guarded_fused_rules(kind, slots, hyper):
    from saragan_amd import _lib
    from saragan_amd import functional as F
    k = getattr(_lib, f'SG_OPT_{kind}')
    s = lambda d, i: d[slots[i]] if len(slots) > i else None
    lr = 0.01
    # flag clear: the bookkeeping thread writes (float)lr, the guarded launch == the _dev launch with that step size
    b = _bufs(4, slots)
    ref = _clone(b)
    flag, t = _flag(), torch.zeros(1, dtype=torch.int64, device='cuda')
    cnt, lr_t = torch.zeros(3, dtype=torch.int64, device='cuda'), torch.zeros(1, device='cuda')
    F.nonfinite_flag_(flag, b['g'])
    F.guard_step_(flag, t, cnt, lr, lr_t)
    assert lr_t.item() == np.float32(lr) and int(t) == 1
    F.optim_step_(k, b['p'], b['g'], s(b, 0), s(b, 1), b['ema'], 0.0, gscale=0.5, ema_decay=0.99, lr_dev=lr_t, skip=flag,
                  **hyper)
    F.optim_step_(k, ref['p'], ref['g'], s(ref, 0), s(ref, 1), ref['ema'], 0.0, gscale=0.5, ema_decay=0.99, lr_dev=lr_t,
                  **hyper)
    for key in b:
        assert torch.equal(b[key], ref[key]), key
    # flag set: parameters and slots untouched, the EMA as the existing EMA-only launch makes it
    b = _bufs(5, slots)
    b['g'][N - 2] = float('-inf')
    ref = _clone(b)
    F.nonfinite_flag_(flag, b['g'])
    F.guard_step_(flag, t, cnt, lr, lr_t)
    assert int(t) == 1 and cnt.tolist() == [1, 1, 1]
    F.optim_step_(k, b['p'], b['g'], s(b, 0), s(b, 1), b['ema'], 0.0, ema_decay=0.99, lr_dev=lr_t, skip=flag, **hyper)
    for key in ('p', 'g') + slots:
        assert torch.equal(b[key], ref[key]), key
    F.adam_ema_(ref['p'], None, None, None, ref['ema'], 0.0, 0.0, 0.9, 1, ema_decay=0.99)
    assert torch.equal(b['ema'], ref['ema'])


# ---------------------------------------------------------------------------------------------------------------------
# 3.-4. whole steps
# ---------------------------------------------------------------------------------------------------------------------
def _steps(golden_dir, monkeypatch, dtype, guard, captured, bad, nsteps, clipping=False, bad_value=float('nan')):
    """nsteps simultaneous steps of the stored toy pgan (phase 3, Adam, EMA fused) from the fixture's weights, with a
    non-finite entry in the real batch of the (0-based) steps in `bad`.  Returns per-step snapshots."""
    import saragan_amd.optimization as opt
    from saragan_amd import functional as F
    from saragan_amd.ExtendedEMA import ExtendedEMA
    from saragan_amd.networks import loss as L
    from saragan_amd.networks.ops import ScalarVariable
    from saragan_amd.networks.pgan.discriminator import discriminator
    from saragan_amd.networks.pgan.generator import generator
    from saragan_amd.varstore import VariableStore, set_compute_dtype, use_store
    from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT, load_step_fixture
    fx = load_step_fixture(os.path.join(golden_dir, NAME), torch.float64)
    monkeypatch.setenv('SARAGAN_HIPGRAPH', '1' if captured else '0')
    monkeypatch.setenv('SARAGAN_NONFINITE_GUARD', '1' if guard else '0')
    set_compute_dtype(dtype)
    try:
        store = VariableStore('cuda', seed=0)
        L.set_random_source(L.RandomSource(1234, 'cuda'))
        g_lr, d_lr = ScalarVariable(1e-3, 'g_lr'), ScalarVariable(1e-3, 'd_lr')
        og, od = opt.AdamOptimizer(g_lr, 0.0, 0.9), opt.AdamOptimizer(d_lr, 0.0, 0.9)
        ph = opt.Placeholder([4, 1, 1, 1, 1])
        with use_store(store):
            tup = opt.optimize_step(og, od, generator, discriminator, ph, LATENT, ScalarVariable(0.0, 'alpha'), fx['phase'],
                                    BASE_SHAPE, KERNEL_SPEC, FILTER_SPEC, 'leaky_relu', 0.2, 'wgan', fx['cfg']['gp_weight'],
                                    'simultaneous', clipping, clipping, 0.01, None)
        store.load_state_dict(dict(fx['p0']), strict=True)
        graph = tup[0].graph
        assert (graph.guard is not None) == guard
        ema = ExtendedEMA(list(store.vars.keys()), 0.99, graph=graph)
        ema_op = ema.apply()
        sess = opt.Session('cuda')
        gen = torch.Generator().manual_seed(5)
        reals = [(fx['real'].float() + 0.1 * torch.randn(fx['real'].shape, generator=gen)).cuda() for _ in range(nsteps)]
        for i in bad:
            reals[i].view(-1)[3] = bad_value
        snaps = []
        for i in range(nsteps):
            g_lr.assign(1e-3 * (1.0 + 0.1 * i))          # a schedule: the base lr moves every step
            sess.run([tup[0], tup[1], tup[2], tup[3]], feed_dict={ph: reals[i]})
            sess.run(ema_op)
            torch.cuda.synchronize()
            graph.guard_report()
            snap = {k: v.detach().clone() for k, v in store.vars.items()}
            for net, o in (('generator', og), ('discriminator', od)):
                st = o.state[net + '/']
                snap[net + '/m'], snap[net + '/v'] = st['m'].clone(), st['v'].clone()
                snap[net + '/ema'] = ema.shadow_flat(net + '/').clone()
                snap[net + '/t'] = o.t            # (guard_report brought the host count in line with the device)
            snap['skipped'] = graph.skipped_steps
            snaps.append(snap)
        if captured:
            assert any('graph' in e for e in graph.__dict__.get('_captures', {}).values()), 'the step was not captured'
        return snaps
    finally:
        set_compute_dtype(torch.float32)
        F.clear_kept_workspaces()


def _net_keys(snap, net):
    return [k for k in snap if k.startswith(net + '/') and not k.endswith('/t')]


def _equal(a, b, keys):
    for k in keys:
        assert (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]), k


@pytest.fixture
def deterministic(sg_env):
    from saragan_amd import functional as F
    F.clear_kept_workspaces()
    sg_env(SG_DETERMINISTIC=1)
    yield
    F.clear_kept_workspaces()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_nan_batch_skips_the_discriminator(golden_dir, monkeypatch, deterministic, dtype):
    guarded = _steps(golden_dir, monkeypatch, dtype, guard=True, captured=False, bad=[1], nsteps=4)
    plain = _steps(golden_dir, monkeypatch, dtype, guard=False, captured=False, bad=[1], nsteps=2)
    s1, s2 = guarded[0], guarded[1]
    # D: parameters, slots and step count as after step 1 (the EMA still moved: it is not compared)
    _equal(s2, s1, [k for k in _net_keys(s1, 'discriminator') if not k.endswith('/ema')])
    assert (s1['discriminator/t'], s2['discriminator/t'], guarded[3]['discriminator/t']) == (1, 1, 3)
    assert (s2['generator/t'], guarded[3]['generator/t']) == (2, 4)
    # G: bit-identical to the unguarded run through step 2 (its update read D's pre-step weights)
    _equal(s2, plain[1], _net_keys(s2, 'generator'))
    _equal(s1, plain[0], list(s1.keys() - {'skipped'}))
    assert guarded[3]['skipped'] == {'generator': 0, 'discriminator': 1}
    for k in _net_keys(guarded[3], 'discriminator') + _net_keys(guarded[3], 'generator'):
        assert torch.isfinite(guarded[3][k]).all(), k
    # without the guard the same batch poisons the discriminator
    assert not all(bool(torch.isfinite(plain[1][k]).all()) for k in _net_keys(plain[1], 'discriminator'))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_captured_guarded_step_equals_eager(golden_dir, monkeypatch, deterministic, dtype):
    """The sequence above with the step forced into a hipGraph (steps 3 and 4 are replays): bit-identical."""
    eager = _steps(golden_dir, monkeypatch, dtype, guard=True, captured=False, bad=[1], nsteps=4)
    graph = _steps(golden_dir, monkeypatch, dtype, guard=True, captured=True, bad=[1], nsteps=4)
    for i, (a, b) in enumerate(zip(eager, graph)):
        assert a['skipped'] == b['skipped'], i
        _equal(a, b, [k for k in a if k != 'skipped'])
    assert graph[-1]['skipped'] == {'generator': 0, 'discriminator': 1}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_skip_decided_inside_a_replay(golden_dir, monkeypatch, deterministic, dtype):
    """A NaN batch at step 4, a replay: D is skipped there, from the flag the graph itself computed."""
    bad = [1, 3]
    graph = _steps(golden_dir, monkeypatch, dtype, guard=True, captured=True, bad=bad, nsteps=5)
    assert graph[-1]['skipped']['discriminator'] == 2 and graph[-1]['discriminator/t'] == 3
    _equal(graph[3], graph[2], [k for k in _net_keys(graph[2], 'discriminator') if not k.endswith('/ema')])
    for k in _net_keys(graph[-1], 'discriminator') + _net_keys(graph[-1], 'generator'):
        assert torch.isfinite(graph[-1][k]).all(), k
    if dtype == torch.float32:      # and the replayed run is the eager one, bit for bit
        eager = _steps(golden_dir, monkeypatch, dtype, guard=True, captured=False, bad=bad, nsteps=5)
        for i, (a, b) in enumerate(zip(eager, graph)):
            assert a['skipped'] == b['skipped'], i
            _equal(a, b, [k for k in a if k != 'skipped'])
        assert graph[-1]['skipped'] == {'generator': 0, 'discriminator': 2} and graph[-1]['generator/t'] == 5


def test_clipping_with_an_inf_skips_without_nan(golden_dir, monkeypatch, deterministic):
    snaps = _steps(golden_dir, monkeypatch, torch.float32, guard=True, captured=False, bad=[1], nsteps=3, clipping=True,
                   bad_value=float('inf'))
    assert snaps[-1]['skipped'] == {'generator': 0, 'discriminator': 1}
    _equal(snaps[1], snaps[0], [k for k in _net_keys(snaps[0], 'discriminator') if not k.endswith('/ema')])
    for s in snaps:
        for k, v in s.items():
            if torch.is_tensor(v):
                assert torch.isfinite(v).all(), k


# ---------------------------------------------------------------------------------------------------------------------
# 5. the training loop stops after N consecutive skips and keeps the last good checkpoint
# ---------------------------------------------------------------------------------------------------------------------
def test_consecutive_skips_stop_the_run(tmp_path):
    from saragan_amd.optimization import NonFiniteStepsError
    from saragan_amd.train import run_training
    from tests.test_train_gpu import _args
    data, logdir = tmp_path / 'data', tmp_path / 'log'
    d = data / '4x4'
    d.mkdir(parents=True)
    for i in range(8):
        v = np.random.default_rng(i).normal(1024, 512, (1, 4, 4)).astype(np.float32)
        v[0, 1, 2] = np.nan                                    # every file of the phase is poisoned
        np.save(d / f'{i:04d}.npy', v)
    args = _args(data, logdir, ending_phase=1, skip_nonfinite_steps=True, max_consecutive_nonfinite=2)
    with pytest.raises(NonFiniteStepsError, match=r'discriminator.*global_step 8'):
        run_training(args)
    assert not any(f.startswith('model_1') for f in os.listdir(logdir))


# ---------------------------------------------------------------------------------------------------------------------
# 6. two data-parallel ranks (gloo, both on cuda:0), a NaN in rank 0's half of the batch only
# ---------------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, golden, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      SARAGAN_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', SARAGAN_NONFINITE_GUARD='1',
                      SARAGAN_HIPGRAPH='0')
    import saragan_amd.optimization as opt
    from saragan_amd import parallel
    from saragan_amd.ExtendedEMA import ExtendedEMA
    from saragan_amd.networks import loss as L
    from saragan_amd.networks.ops import ScalarVariable
    from saragan_amd.networks.pgan.discriminator import discriminator
    from saragan_amd.networks.pgan.generator import generator
    from saragan_amd.varstore import VariableStore, set_compute_dtype, use_store
    from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT, load_step_fixture
    parallel.init_distributed()
    fx = load_step_fixture(os.path.join(golden, NAME), torch.float64)
    n = fx['real'].shape[0] // world
    sl = slice(rank * n, (rank + 1) * n)
    set_compute_dtype(torch.float32)
    store = VariableStore('cuda', seed=100 + rank)
    L.set_random_source(L.InjectedRandom({k: v[sl].float() for k, v in fx['rnd'].items()}))
    og = parallel.DistributedOptimizer(opt.AdamOptimizer(ScalarVariable(1e-3), 0.0, 0.9))
    od = parallel.DistributedOptimizer(opt.AdamOptimizer(ScalarVariable(1e-3), 0.0, 0.9))
    ph = opt.Placeholder([n, 1, 1, 1, 1])
    with use_store(store):
        tup = opt.optimize_step(og, od, generator, discriminator, ph, LATENT, ScalarVariable(fx['alpha']), fx['phase'],
                                BASE_SHAPE, KERNEL_SPEC, FILTER_SPEC, 'leaky_relu', 0.2, fx['loss_fn'], fx['cfg']['gp_weight'],
                                'simultaneous', False, False, 0.01, None)
    if rank == 0:
        store.load_state_dict(fx['p0'], strict=True)
    graph = tup[0].graph
    ema = ExtendedEMA(list(store.vars), 0.99, graph=graph)
    graph._ensure_flat()
    parallel.broadcast_global_variables(store, 0)
    ema.reset_to_variables()
    before = {k: v.detach().cpu().numpy().copy() for k, v in store.vars.items()}
    real = fx['real'][sl].float().clone()
    if rank == 0:
        real.view(-1)[0] = float('nan')
    sess = opt.Session('cuda')
    sess.run([tup[0], tup[1]], feed_dict={ph: real})
    sess.run(ema.apply())
    torch.cuda.synchronize()
    rep = graph.guard_report()
    q.put((rank, dict(vars={k: v.detach().cpu().numpy() for k, v in store.vars.items()}, before=before, report=rep,
                      t=(og.t, od.t))))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_skip_together(golden_dir):
    from tests.test_dp_gpu import _free_port
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, golden_dir, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for r in range(world):
        assert res[r]['report']['discriminator'][0] == 1 and res[r]['report']['generator'][0] == 0, r
        assert res[r]['t'] == (1, 0), r
        for k, v in res[r]['vars'].items():
            assert np.isfinite(v).all(), (r, k)
            if k.startswith('discriminator/'):
                np.testing.assert_array_equal(v, res[r]['before'][k], err_msg=f'rank {r} {k}')
    for k in res[0]['vars']:
        np.testing.assert_array_equal(res[0]['vars'][k], res[1]['vars'][k], err_msg=k)
