"""python -m saragan_amd.generate: a checkpoint becomes a directory of typed volumes.  The checkpoint recipe is
tests/test_generate_gpu.py's (phase 3, f32, 4 x 16 x 16, 5 samples in batches of 2); every volume is compared with the CPU oracle
generator on the latents the manifest's rule replays, within that test's own tolerance e = 2e-2 + 1e-4 |ref| in data units: the
stored integer is within one count of trunc(ref) everywhere and EQUAL wherever ref is farther than e from an integer and from
both clip bounds.  Then shards, --resume, the refusal to overwrite, the manifest against the files, NRRD, a conditional
checkpoint and the tools that read the directory."""
import io
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import pgan_oracle as O
from tests import condref as CR
from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT

pytestmark = pytest.mark.gpu

PHASE, COUNT, SEED, MEAN, STD = 3, 5, 7, 1024.0, 1024.0
NAMES = [f'{i:07d}.npy' for i in range(COUNT)]


def gen(argv):
    """One run of the tool in this process: (manifest, what it printed)."""
    from saragan_amd import generate as G
    text = io.StringIO()
    manifest = G.run(G.build_parser().parse_args(argv), out=text)
    return manifest, text.getvalue()


def save_params(p, path):
    from saragan_amd.utils import save_checkpoint
    from saragan_amd.varstore import VariableStore
    store = VariableStore('cuda', seed=0)
    for k, v in p.items():                      # a training-side checkpoint: G and D variables, TF names
        store.get(k, tuple(v.shape), 'zeros')
    store.load_state_dict(p, strict=True)
    save_checkpoint(store, path)
    return path


def latents(indices=range(COUNT)):
    from saragan_amd import generate as G
    return torch.from_numpy(G.latent_rows(SEED, list(indices), LATENT)).double()


def check_against(ref, stored, lo, hi, rint=False):
    """ref: the oracle's volume in data units (float64); stored: the file's integers; [lo, hi]: the clip range.  The stored value
    can differ from the oracle's only where ref is within e of a point at which the rounding jumps: an integer (trunc) or a tie
    k + 0.5 (rint), or of a clip bound."""
    e = 2e-2 + 1e-4 * np.abs(ref)
    want = (np.rint if rint else np.trunc)(np.clip(ref, lo, hi))
    got = stored.astype(np.float64)
    assert np.abs(got - want).max() <= 1
    jump = np.floor(ref) + 0.5 if rint else np.rint(ref)
    sure = (np.abs(ref - jump) > e) & (np.abs(ref - lo) > e) & (np.abs(ref - hi) > e)
    assert sure.mean() > 0.1                    # (the comparison below is not empty)
    assert np.array_equal(got[sure], want[sure])


@pytest.fixture(scope='module')
def ckpt(tmp_path_factory):
    root = tmp_path_factory.mktemp('generate_dataset')
    p = O.init_params(PHASE, BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC, seed=4, bias_std=0.1)
    spec = root / 'spec.json'
    spec.write_text(json.dumps(dict(kernel_spec=KERNEL_SPEC, filter_spec=FILTER_SPEC)))
    ref = O.generator(p, latents(), 0.0, PHASE, BASE_SHAPE, 'leaky_relu', KERNEL_SPEC, FILTER_SPEC, 0.2).numpy() * STD + MEAN
    return dict(root=root, params=p, spec=str(spec), model=save_params(p, str(root / 'model_3')), ref=ref[:, 0])


def argv_for(ckpt, out_dir, *more, model=None):
    return ['pgan', '--start_shape', str(BASE_SHAPE), '--final_shape', '(1, 4, 16, 16)', '--kernel_spec', ckpt['spec'], '--filter_spec',
            ckpt['spec'], '--network_size', 'xs', '--latent_dim', str(LATENT), '--output_dir', str(out_dir), '--model_path',
            model or ckpt['model'], '--num_samples', str(COUNT), '--batch_size', '2', '--phase', str(PHASE), '--data_mean', str(MEAN),
            '--data_stddev', str(STD), '--seed', str(SEED), '--dtype', 'f32', *more]


@pytest.fixture(scope='module')
def single(ckpt):
    """The whole set in one run, with the sheet."""
    out = ckpt['root'] / 'single'
    manifest, text = gen(argv_for(ckpt, out, '--png', '--preview_samples', '3'))
    return dict(dir=str(out / f'generated_{PHASE}'), manifest=manifest, text=text,
                vols=[np.load(out / f'generated_{PHASE}' / n) for n in NAMES])


def test_files_latents_and_oracle(ckpt, single):
    from saragan_amd import generate as G
    listing = sorted(os.listdir(single['dir']))
    assert listing == NAMES + ['manifest_0of1.json', 'preview_0of1.png']
    m = json.load(open(os.path.join(single['dir'], 'manifest_0of1.json')))
    assert m['files'] == single['manifest']['files'] and m['pooled'] == single['manifest']['pooled']
    assert m['latent'] == G.LATENT_RULE and (m['seed'], m['latent_dim'], m['shard']) == (SEED, LATENT, [0, 1])
    assert [(r['index'], r['name']) for r in m['files']] == list(enumerate(NAMES)) and m['skipped'] == []
    assert m['dtype'] == 'uint16' and m['shape'] == [4, 16, 16] and m['clip'] == [0, 65535] and m['rounding'] == 'trunc'
    assert 'two roundings' in m['definition'] and m['arguments']['batch_size'] == 2
    rows = np.stack([np.random.default_rng([m['seed'], r['index']]).standard_normal(m['latent_dim'], dtype=np.float32) for r in m['files']])
    assert np.array_equal(rows, latents().numpy().astype(np.float32))      # the rule, replayed from the manifest alone
    for i, v in enumerate(single['vols']):
        assert v.dtype == np.uint16 and v.shape == (4, 16, 16)
        check_against(ckpt['ref'][i], v, 0, 65535)
    assert set(m['seconds']) == {'generation', 'store', 'download', 'save', 'wall'} and all(s >= 0 for s in m['seconds'].values())


def test_manifest_statistics_equal_the_files(single):
    m = single['manifest']
    voxels = 4 * 16 * 16
    for r, v in zip(m['files'], single['vols']):
        a = [int(x) for x in v.reshape(-1)]
        mean = Fraction(sum(a), voxels)
        var = Fraction(sum(x * x for x in a), voxels) - mean * mean
        assert (r['min'], r['max'], r['mean'], r['stddev']) == (min(a), max(a), float(mean), math.sqrt(var))
        assert r['nan'] == 0 and 0 <= r['below'] <= sum(x == 0 for x in a) and 0 <= r['above'] <= sum(x == 65535 for x in a)
    every = [int(x) for v in single['vols'] for x in v.reshape(-1)]
    mean = Fraction(sum(every), len(every))
    var = Fraction(sum(x * x for x in every), len(every)) - mean * mean
    p = m['pooled']
    assert (p['files'], p['voxels'], p['min'], p['max'], p['mean'], p['stddev']) == (COUNT, len(every), min(every), max(every), float(mean),
                                                                                      math.sqrt(var))
    assert p['below'] == sum(r['below'] for r in m['files']) and p['clipped_share'] == (p['below'] + p['above'] + p['nan']) / p['voxels']


def test_shards_resume_and_refusal(ckpt, single):
    from saragan_amd import generate as G
    out = ckpt['root'] / 'sharded'
    d = out / f'generated_{PHASE}'
    m0, _ = gen(argv_for(ckpt, out, '--shard', '0/2'))
    m1, _ = gen(argv_for(ckpt, out, '--shard', '1/2', '--batch_size', '3'))
    assert [r['index'] for r in m0['files']] == [0, 2, 4] and [r['index'] for r in m1['files']] == [1, 3]
    assert sorted(os.listdir(d)) == NAMES + ['manifest_0of2.json', 'manifest_1of2.json']
    for i, n in enumerate(NAMES):                # another batch composition, another batch size: the same sample
        v, ref = np.load(d / n).astype(np.int64), ckpt['ref'][i]
        sure = np.abs(ref - np.rint(ref)) > 2e-2 + 1e-4 * np.abs(ref)
        assert np.abs(v - single['vols'][i].astype(np.int64))[sure].max() <= 1
    # RANK / WORLD_SIZE of a launcher are the default shard
    assert G.plan(G.build_parser().parse_args(argv_for(ckpt, out)), env={'RANK': '1', 'WORLD_SIZE': '2'})['indices'] == [1, 3]
    # an existing file, no flag: an error before anything is written
    before = {n: (os.stat(d / n).st_mtime_ns, open(d / n, 'rb').read()) for n in sorted(os.listdir(d))}
    with pytest.raises(SystemExit, match='exists.*--resume.*--overwrite'):
        G.main(argv_for(ckpt, out))
    os.remove(d / NAMES[1])
    os.remove(d / NAMES[4])
    with pytest.raises(SystemExit, match='exists'):      # three are still there
        G.main(argv_for(ckpt, out))
    assert sorted(os.listdir(d)) == sorted(set(before) - {NAMES[1], NAMES[4]})
    assert all(os.stat(d / n).st_mtime_ns == before[n][0] for n in os.listdir(d))
    # --resume writes the two that are missing and touches nothing else
    m, _ = gen(argv_for(ckpt, out, '--resume'))
    assert [r['index'] for r in m['files']] == [1, 4] and m['skipped'] == [NAMES[0], NAMES[2], NAMES[3]]
    assert sorted(os.listdir(d)) == sorted(list(before) + ['manifest_0of1.json'])
    for n in before:
        rewritten = n in (NAMES[1], NAMES[4])
        assert (os.stat(d / n).st_mtime_ns == before[n][0]) == (not rewritten), n
        assert rewritten or open(d / n, 'rb').read() == before[n][1], n
    for i in (1, 4):                             # the sample again, from its index alone
        check_against(ckpt['ref'][i], np.load(d / NAMES[i]), 0, 65535)


def test_nrrd_uint8_and_the_clipping_warning(ckpt, single):
    from saragan_amd import nrrd_io
    out = ckpt['root'] / 'nrrd'
    m, text = gen(argv_for(ckpt, out, '--format', 'nrrd', '--spacing', '2.5,0.75,0.5', '--out_dtype', 'int16', '--name_prefix', 'fake_',
                           '--num_samples', '3'))
    d = out / f'generated_{PHASE}'
    assert sorted(os.listdir(d)) == ['fake_0000000.nrrd', 'fake_0000001.nrrd', 'fake_0000002.nrrd', 'manifest_0of1.json']
    for i in range(3):
        arr, h = nrrd_io.read(d / f'fake_{i:07d}.nrrd')
        assert arr.dtype == np.int16 and arr.shape == (4, 16, 16) and tuple(h.spacing) == (2.5, 0.75, 0.5)
        # int16 clips at 32767 and keeps what uint16 clipped at 0
        assert np.array_equal(np.clip(arr, 0, None), np.clip(single['vols'][i], None, 32767))
        check_against(ckpt['ref'][i], arr, -32768, 32767)
    # a window that most of the data misses: the warning names the flag to change
    m, text = gen(argv_for(ckpt, ckpt['root'] / 'u8', '--out_dtype', 'uint8', '--rounding', 'rint', '--num_samples', '2'))
    assert m['pooled']['clipped_share'] > 0.5 and 'warning' in text and '--clip' in text and '--out_dtype' in text
    assert 'warning' not in single['text'] or single['manifest']['pooled']['clipped_share'] > 0.01
    v = np.load(ckpt['root'] / 'u8' / f'generated_{PHASE}' / NAMES[0])
    assert v.dtype == np.uint8
    check_against(ckpt['ref'][0], v, 0, 255, rint=True)


def test_conditional_checkpoint_takes_row_i_for_sample_i(ckpt):
    p = CR.init_params(PHASE, BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC, 3, seed=5)
    model = save_params(p, str(ckpt['root'] / 'cond_model_3'))
    table = np.eye(3, dtype=np.float32)[[0, 2, 1, 1, 0]] * np.float32(1.5)
    path = ckpt['root'] / 'labels.npy'
    np.save(path, table)
    out = ckpt['root'] / 'cond'
    m, _ = gen(argv_for(ckpt, out, '--conditioning_path', str(path), '--out_dtype', 'int16', model=model))
    ref = CR.generator(p, latents(), torch.from_numpy(table).double(), 0.0, PHASE, BASE_SHAPE, 'leaky_relu', KERNEL_SPEC, FILTER_SPEC,
                       0.2).numpy()[:, 0] * STD + MEAN
    vols = [np.load(out / f'generated_{PHASE}' / n) for n in NAMES]
    for i in range(COUNT):
        check_against(ref[i], vols[i], -32768, 32767)
    assert not np.array_equal(vols[0], vols[4])      # (the same label row, other latents)
    with pytest.raises(ValueError, match='--conditioning'):
        gen(argv_for(ckpt, ckpt['root'] / 'cond2', model=model))


def test_metric_and_preview_tools_read_the_directory(single, tmp_path):
    from saragan_amd import preview
    from saragan_amd.metrics import sample_metrics
    vols = sample_metrics.load_dir(single['dir'])
    assert vols.shape == (COUNT, 4, 16, 16) and np.array_equal(vols, np.stack(single['vols']).astype(np.float32))
    loaded = preview.load_volumes(single['dir'])
    assert loaded.dtype == np.uint16 and loaded.shape == (COUNT, 4, 16, 16)
    png = preview.main([single['dir'], '--window=0,3072', '--max_samples', '5', '--out', str(tmp_path / 'sheet.png')])
    assert open(png, 'rb').read(8) == b'\x89PNG\r\n\x1a\n'
    sheet = open(os.path.join(single['dir'], 'preview_0of1.png'), 'rb').read()
    assert sheet[:8] == b'\x89PNG\r\n\x1a\n'
