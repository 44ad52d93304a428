"""Host side of spectral normalisation (--d_spectral_norm; networks.ops.set_spectral_norm): the fp64 statement of tests/snref.py
against torch autograd, the row-block table against a brute-force enumeration, the variable store's non-trainable state and
effective-weight buffers, the flags and the refused combinations."""
import types

import numpy as np
import pytest
import torch

from tests import snref
from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT


def _torch_spectral_norm(w, u, iteration=1):
    """The definition in torch (double), u and v detached: what autograd differentiates."""
    with torch.no_grad():
        for _ in range(iteration):
            v_ = u @ w.t()
            v = v_ / torch.sqrt(torch.clamp((v_ * v_).sum(), min=1e-12))
            u_ = v @ w
            u = u_ / torch.sqrt(torch.clamp((u_ * u_).sum(), min=1e-12))
    sigma = (v @ w @ u.t()).reshape(())
    return w / sigma, u, v, sigma


@pytest.mark.parametrize('shape', [(1, 16), (512, 1), (81, 5)])
@pytest.mark.parametrize('iteration', [1, 3])
def test_pullback_equals_double_autograd_through_the_definition(shape, iteration):
    gen = torch.Generator().manual_seed(shape[0] + iteration)
    w = torch.randn(shape, dtype=torch.float64, generator=gen, requires_grad=True)
    u0 = torch.randn(1, shape[1], dtype=torch.float64, generator=gen)
    g = torch.randn(shape, dtype=torch.float64, generator=gen)
    wbar, u, v, sigma = _torch_spectral_norm(w, u0, iteration)
    (want,) = torch.autograd.grad(wbar, w, grad_outputs=g)
    ref = snref.refresh(w.detach().numpy(), u0.numpy(), iteration)
    for key, t in (('u', u), ('v', v), ('sigma', sigma), ('wbar', wbar)):
        np.testing.assert_allclose(ref[key], t.detach().numpy().reshape(np.shape(ref[key])), rtol=1e-12, atol=0)
    got = snref.pullback(g.numpy(), ref['wbar'], ref['u'], ref['v'], ref['sigma'])
    scale = float(want.abs().max())
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-12, atol=1e-12 * scale)      # fp64 round-off only


def test_refresh_honours_the_clamps():
    ref = snref.refresh(np.zeros((3, 2)), np.ones(2), 1)
    assert (ref['u'] == 0).all() and (ref['v'] == 0).all() and ref['sigma'] == 0.0
    tiny = snref.refresh(np.full((1, 1), 1e-9), np.ones(1), 1)       # sum v_^2 = 1e-18 < 1e-12: divided by 1e-6, not by |v_|
    np.testing.assert_allclose(tiny['v'], [1e-3], rtol=1e-12)


LAYERS = [(1, 16), (512, 1), (81, 5), (864, 32), (4096, 600), (3, 9000), (20, 4100)]


def test_row_block_table_covers_every_element_once_and_no_padding():
    from saragan_amd import _lib
    from saragan_amd.functional import spectral_rows_per_block, spectral_table_arrays
    chunk = _lib.SG_SEG_CHUNK
    starts, total = [], 0
    for r, c in LAYERS:
        starts.append(total)
        total += (r * c + 3) // 4 * 4 + 4
    segs, blocks, ulen, vlen, collen = spectral_table_arrays([(s, r, c) for s, (r, c) in zip(starts, LAYERS)], total)
    hits = np.zeros(total, np.int64)
    per_seg = [0] * len(segs)
    for b, (s, rb) in enumerate(blocks):
        start, rows, cols, first, rpb = segs[s][:5]
        assert 1 <= rpb <= chunk and rpb == spectral_rows_per_block(rows, cols)
        assert first + rb == b                                           # a segment's blocks are consecutive from `first`
        r0, r1 = rb * rpb, min(rows, (rb + 1) * rpb)
        assert r0 < r1
        for r in range(r0, r1):                                          # brute force: every row of the block, whole rows only
            hits[start + r * cols:start + (r + 1) * cols] += 1
        per_seg[s] += 1
    want = np.zeros(total, np.int64)
    for s, (r, c) in zip(starts, LAYERS):
        want[s:s + r * c] = 1
    assert (hits == want).all()                                          # every element once, no padding element
    # the state and workspace regions are disjoint and inside their buffers
    for field, length, size in ((5, ulen, lambda e: e[2]), (6, vlen, lambda e: e[1]),
                                (7, collen, lambda e: -(-e[1] // e[4]) * e[2])):
        end = 0
        for e in segs:
            assert e[field] >= end and e[field] % 4 == 0
            end = e[field] + size(e)
        assert end <= length
    for e, n in zip(segs, per_seg):
        assert n == -(-e[1] // e[4])
    assert segs[4][4] == 32 and segs[5][4] == 3 and segs[1][4] == 512    # at most 128 blocks; never more rows than there are
    assert spectral_rows_per_block(200, 600) == 16 and spectral_rows_per_block(10 ** 6, 8) == chunk
    for bad in ([(2, 3, 3)], [(0, 3, 3), (8, 2, 2)], [(0, 0, 3)], [(0, 3, 0)], [(0, 4, total)], []):
        with pytest.raises(ValueError):
            spectral_table_arrays(bad, total)


def _phase_graph(spectral, phase=2, adasum=False):
    import saragan_amd.optimization as opt
    from saragan_amd.networks import ops as nops
    from saragan_amd.networks.ops import ScalarVariable
    from saragan_amd.networks.pgan.discriminator import discriminator
    from saragan_amd.networks.pgan.generator import generator
    from saragan_amd.varstore import VariableStore, use_store
    store = VariableStore('cpu', seed=0)
    og, od = opt.AdamOptimizer(ScalarVariable(1e-3), 0.0, 0.9), opt.AdamOptimizer(ScalarVariable(1e-3), 0.0, 0.9)
    if adasum:
        od.distributed = types.SimpleNamespace(delta_form=True)
    prev = nops.set_spectral_norm(('discriminator/',) if spectral else (), 2 if spectral else 1)
    try:
        with use_store(store):
            tup = opt.optimize_step(og, od, generator, discriminator, opt.Placeholder([4, 1, 1, 1, 1]), LATENT,
                                    ScalarVariable(0.5), phase, BASE_SHAPE, KERNEL_SPEC, FILTER_SPEC, 'leaky_relu', 0.2, 'wgan',
                                    10.0, 'simultaneous', False, False, 0.01)
    finally:
        nops.set_spectral_norm(*prev)
    return store, tup[0].graph


def test_defaults_add_no_state_and_no_effective_buffers():
    store, graph = _phase_graph(False)
    assert not store.state and not store.effective
    assert not any(k.endswith('/u') for k in store.state_dict())
    graph._ensure_flat()
    for flat in store.flat.values():
        assert 'eff' not in flat and 'spectral' not in flat
    assert graph.cfg['sn_iterations'] == 1


def test_normalised_weights_are_state_not_parameters():
    off, _ = _phase_graph(False)
    store, graph = _phase_graph(True)
    d_weights = [k for k in store.vars if k.startswith('discriminator/') and k.endswith('/weight')]
    assert list(store.effective) == d_weights and d_weights
    assert sorted(store.state) == sorted(k[:-len('weight')] + 'u' for k in d_weights)
    for k in d_weights:
        assert tuple(store.state[store.u_name(k)].shape) == (1, store.vars[k].shape[-1])
        leaf = store.effective[k]
        assert leaf.is_leaf and leaf.requires_grad and leaf.shape == store.vars[k].shape
    for prefix in ('', 'generator/', 'discriminator/'):
        assert store.count_parameters(prefix) == off.count_parameters(prefix)
        assert [k for k, _ in store.trainable(prefix)] == [k for k, _ in off.trainable(prefix)]
    for k in off.vars:                                                  # creating u after the variables leaves their draws alone
        assert torch.equal(store.vars[k], off.vars[k]), k
    sd = store.state_dict()
    assert set(sd) == set(store.vars) | set(store.state)
    assert graph.cfg['sn_iterations'] == 2
    graph._ensure_flat()
    flat = store.flat['discriminator/']
    assert 'eff' not in store.flat['generator/']
    assert flat['eff'].numel() == flat['param'].numel() == flat['total'] and flat['normalised'] == d_weights
    assert 'discriminator/' in store.rewritten
    for s, k in enumerate(flat['normalised']):
        o, n = flat['offsets'][k]
        assert store.effective[k].data_ptr() == flat['eff'][o:o + n].data_ptr()
        assert store.state[store.u_name(k)].data_ptr() == flat['spectral'].views(s)[0].data_ptr()
        assert torch.equal(store.state[store.u_name(k)], sd[store.u_name(k)])
        assert k not in [n_ for n_ in flat['offsets'] if n_.endswith('/u')]
    assert not any(k.endswith('/u') for k in flat['offsets'])           # u is in no flat parameter / gradient buffer
    # a checkpoint without u loads (non-strict) and leaves u fresh; one with u restores it
    missing = store.load_state_dict({k: v for k, v in sd.items() if not k.endswith('/u')})
    assert sorted(missing) == sorted(store.state)
    name = store.u_name(d_weights[0])
    sd[name] = sd[name] + 1.0
    store.load_state_dict(sd, strict=True)
    assert torch.equal(store.state[name], sd[name])
    store.drop([d_weights[0]])
    assert d_weights[0] not in store.effective and name not in store.state and not store.flat


def test_only_discriminator_weights_and_current_values():
    """get_weight(use_spectral_norm=True) outside the discriminator is refused (nothing would refresh it); an effective weight
    whose raw weights were rewritten and not refreshed is refused at the forward; the 2-D conv refuses before it registers."""
    from saragan_amd.networks import ops as nops
    from saragan_amd.networks2d import ops as ops2d
    from saragan_amd.varstore import VariableStore, use_store, variable_scope
    store = VariableStore('cpu', seed=0)
    with use_store(store), variable_scope('generator'), variable_scope('to_rgb_1'):
        with pytest.raises(ValueError, match='discriminator only'):
            nops.get_weight([1, 1, 1, 4, 1], 'linear', use_spectral_norm=True)
    assert not store.effective and not store.state
    with use_store(store), variable_scope('discriminator'), variable_scope('dense_2'):
        with pytest.raises(RuntimeError, match='not current'):       # registered, but never flattened or refreshed
            nops.get_weight([8, 1], 'linear', use_spectral_norm=True)
    assert list(store.effective) == ['discriminator/dense_2/weight']
    graph_store, graph = _phase_graph(True)
    graph._ensure_flat()
    name = 'discriminator/from_rgb_2/weight'
    with pytest.raises(RuntimeError, match='not current'):           # flat, rewritten (created), not refreshed
        graph_store.effective_weight(name)
    graph_store.rewritten.discard('discriminator/')                  # (what a refresh leaves)
    assert graph_store.effective_weight(name) is graph_store.effective[name]
    graph_store.load_state_dict({})
    with pytest.raises(RuntimeError, match='not current'):
        graph_store.effective_weight(name)
    prev = nops.set_spectral_norm(('discriminator/',))
    try:
        store2 = VariableStore('cpu', seed=0)
        with use_store(store2), variable_scope('discriminator'), variable_scope('conv_1'):
            with pytest.raises(NotImplementedError, match='2-D'):
                ops2d.conv2d(torch.zeros(1, 4, 8, 8), 4, (3, 3), 'leaky_relu', param=0.2)
        assert not store2.vars and not store2.effective and not store2.state
    finally:
        nops.set_spectral_norm(*prev)


def test_refused_combinations_raise():
    from saragan_amd.main import build_parser, finalize_args
    from saragan_amd.networks import ops as nops
    base = ['pgan', '/data/', '--start_shape', '(1, 5, 16, 16)', '--final_shape', '(1, 160, 512, 512)', '--starting_phase', '1',
            '--ending_phase', '4', '--latent_dim', '128', '--network_size', 's', '--noise_stddev', '0.01']
    a = finalize_args(build_parser().parse_args(base))
    assert a.d_spectral_norm is False and a.sn_iterations == 1
    a = finalize_args(build_parser().parse_args(base + ['--d_spectral_norm', '--sn_iterations', '3']))
    assert a.d_spectral_norm is True and a.sn_iterations == 3
    for bad in (['--sn_iterations', '2'], ['--d_spectral_norm', '--sn_iterations', '0'], ['--d_spectral_norm', '--use_adasum']):
        with pytest.raises(SystemExit):
            finalize_args(build_parser().parse_args(base + bad))
    with pytest.raises(ValueError):
        nops.set_spectral_norm(('generator/',))
    with pytest.raises(ValueError):
        nops.set_spectral_norm(('discriminator/',), iterations=0)
    assert nops.spectral_norm_settings() == ((), 1)
    with pytest.raises(NotImplementedError, match='get_weight'):
        nops.spectral_norm(torch.zeros(3, 3))
    with pytest.raises(ValueError, match='Adasum'):
        _phase_graph(True, adasum=True)
    _phase_graph(False, adasum=True)                                    # (Adasum alone is no business of this check)
    from saragan_amd.varstore import use_store, variable_scope
    graph_store, graph = _phase_graph(False)
    graph._ensure_flat()
    with use_store(graph_store), variable_scope('discriminator'), variable_scope('from_rgb_2'):
        with pytest.raises(RuntimeError, match='before the step graph'):
            nops.get_weight(list(graph_store.vars['discriminator/from_rgb_2/weight'].shape), 'linear', use_spectral_norm=True)
