"""The non-finite step guard's switches, without a GPU: the command-line flags (off by default, the limit only with the
guard), saragan_amd.set_nonfinite_guard / SARAGAN_NONFINITE_GUARD=1 as read when a StepGraph is built, and the refusal of
the guard together with Adasum."""
import types

import pytest


def _parse(extra):
    from saragan_amd.main import build_parser, finalize_args
    argv = ['pgan', 'data/', '--start_shape', '(1, 1, 4, 4)', '--final_shape', '(1, 4, 16, 16)', '--starting_phase', '1',
            '--ending_phase', '2', '--latent_dim', '16', '--noise_stddev', '0.01', '--network_size', 'xs'] + extra
    args, _ = build_parser().parse_known_args(argv)
    return finalize_args(args)


def _graph():
    from saragan_amd.optimization import StepGraph
    return StepGraph(store=None, cfg={})


@pytest.fixture
def guard_env(monkeypatch):
    monkeypatch.delenv('SARAGAN_NONFINITE_GUARD', raising=False)
    monkeypatch.delenv('SARAGAN_NONFINITE_MAX_CONSECUTIVE', raising=False)
    return monkeypatch


def test_flags_default_off():
    args = _parse([])
    assert args.skip_nonfinite_steps is False and args.max_consecutive_nonfinite is None


def test_flags_parse():
    args = _parse(['--skip_nonfinite_steps', '--max_consecutive_nonfinite', '3'])
    assert args.skip_nonfinite_steps is True and args.max_consecutive_nonfinite == 3


def test_limit_without_the_guard_is_rejected():
    with pytest.raises(SystemExit, match='skip_nonfinite_steps'):
        _parse(['--max_consecutive_nonfinite', '3'])
    with pytest.raises(SystemExit):
        _parse(['--skip_nonfinite_steps', '--max_consecutive_nonfinite', '0'])


def test_step_graph_has_no_guard_by_default(guard_env):
    g = _graph()
    assert g.guard is None
    assert g.skipped_steps == {'generator': 0, 'discriminator': 0}


def test_environment_variable_is_honoured(guard_env):
    guard_env.setenv('SARAGAN_NONFINITE_GUARD', '1')
    g = _graph()
    assert g.guard is not None and g.guard.max_consecutive is None
    assert g.skipped_steps == {'generator': 0, 'discriminator': 0}      # nothing ran: no device read
    guard_env.setenv('SARAGAN_NONFINITE_GUARD', '0')
    assert _graph().guard is None


def test_set_nonfinite_guard(guard_env):
    import saragan_amd
    saragan_amd.set_nonfinite_guard(True, max_consecutive=4)
    g = _graph()
    assert g.guard is not None and g.guard.max_consecutive == 4
    saragan_amd.set_nonfinite_guard(False)
    assert _graph().guard is None
    with pytest.raises(ValueError):
        saragan_amd.set_nonfinite_guard(False, max_consecutive=4)


def test_configure_guard_before_the_first_step(guard_env):
    g = _graph()
    g.configure_guard(True, 2)
    assert g.guard.max_consecutive == 2
    g.configure_guard(False)
    assert g.guard is None
    g._stepped = True
    with pytest.raises(RuntimeError):
        g.configure_guard(True)


def test_guard_with_adasum_is_refused(guard_env):
    from saragan_amd import optimization as opt
    adasum = types.SimpleNamespace(delta_form=True)     # what parallel.AdasumReducer marks itself with
    o = opt.AdamOptimizer(1e-3, 0.0, 0.9)
    o.distributed = adasum
    guard_env.setenv('SARAGAN_NONFINITE_GUARD', '1')
    with pytest.raises(ValueError, match='Adasum'):
        _graph().add_train('discriminator', o, [], False)
    guard_env.setenv('SARAGAN_NONFINITE_GUARD', '0')
    g = _graph()
    g.add_train('discriminator', o, [], False)           # without the guard Adasum is as it was
    with pytest.raises(ValueError, match='Adasum'):
        g.configure_guard(True)


def test_max_consecutive_check_names_the_network(guard_env):
    from saragan_amd.optimization import NonFiniteStepsError
    g = _graph()
    g.configure_guard(True, 2)
    g.check_nonfinite(10, {'generator': (0, 0, 0), 'discriminator': (1, 1, 1)})
    with pytest.raises(NonFiniteStepsError, match=r'discriminator.*global_step 12'):
        g.check_nonfinite(12, {'generator': (0, 0, 0), 'discriminator': (2, 2, 2)})
