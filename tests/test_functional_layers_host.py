"""functional.py's layers (its docstring has the map): the weight-image cache against a stub library, every module below functional
importable on its own, and every name anybody reads from functional still there.  Host only."""
import pathlib
import re
import subprocess
import sys

import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent


# ---- the weight-image cache against a stub library ------------------------------------------------------------------------------
class StubLib:
    """Records the pack entry points' calls; sizes are 64 bytes, return codes 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.endswith('packed_bytes'):
            return lambda shp, dt: 64
        if not name.endswith(('pack', 'pack_weights', 'pack_weights_batch')):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry

    def named(self, name):
        return [a for n, a in self.calls if n == name]


def _shape(cin=8, cout=8, k=3):
    from saragan_amd._lib import ConvShape
    return ConvShape(1, 4, 4, 4, cin, cout, k, k, k, 0)


def _weight(cin=8, cout=8, k=3):
    return torch.randn(k, k, k, cin, cout).requires_grad_(True)


@pytest.fixture
def images():
    from saragan_amd._weight_images import WeightImages
    return WeightImages()


def test_stale_images_are_refreshed_in_one_batch_and_dead_ones_dropped(images):
    from saragan_amd import _lib
    lib, shp = StubLib(), _shape()
    live, dead = _weight(), _weight()
    wp_live = images.fragment(live, 0.5, False, shp, _lib.SG_BF16, lib, None)
    images.fragment(dead, 0.25, True, shp, _lib.SG_BF16, lib, None)
    assert images.stats == {'single': 2, 'batches': 0, 'batched': 0} and len(images.live()) == 2
    with torch.no_grad():
        dead.add_(1.0)                  # rewritten through torch: its version counter moved, the image's key is dead
    images.mark_stale()
    assert images.stale is True
    other = _weight()
    images.fragment(other, 1.0, False, shp, _lib.SG_BF16, lib, None)      # the next lookup refreshes first
    batches = lib.named('sg_conv3d_pack_weights_batch')
    assert len(batches) == 1
    n, ws, coefs, flips, wps, shapes, dt, st = batches[0]
    assert n == 1 and ws[0] == live.data_ptr() and coefs[0] == 0.5 and flips[0] == 0 and wps[0] == wp_live.data_ptr()
    assert (shapes[0].cin, shapes[0].cout, shapes[0].kd) == (8, 8, 3) and dt == _lib.SG_BF16
    assert images.stats == {'single': 3, 'batches': 1, 'batched': 1} and images.stale is False
    assert sorted(k.ptr for k in images._entries) == sorted([live.data_ptr(), other.data_ptr()])
    assert images.fragment(live, 0.5, False, shp, _lib.SG_BF16, lib, None) is wp_live and images.stats['single'] == 3


def test_refresh_is_one_batch_per_dtype(images):
    from saragan_amd import _lib
    lib, shp = StubLib(), _shape()
    a, b, c = _weight(), _weight(), _weight()
    images.fragment(a, 1.0, False, shp, _lib.SG_BF16, lib, None)
    images.fragment(b, 1.0, False, shp, _lib.SG_BF16, lib, None)
    images.fragment(c, 1.0, False, shp, _lib.SG_F32, lib, None)
    images.mark_stale()
    images.fragment(a, 1.0, False, shp, _lib.SG_BF16, lib, None)
    batches = lib.named('sg_conv3d_pack_weights_batch')
    assert sorted((args[6], args[0]) for args in batches) == sorted([(_lib.SG_BF16, 2), (_lib.SG_F32, 1)])
    assert images.stats == {'single': 3, 'batches': 2, 'batched': 3}


def test_mark_stale_drops_the_matrices_and_sub_pixel_images_and_keeps_the_fragments(images):
    from saragan_amd import _lib
    from saragan_amd import _weight_images as WI
    lib, shp = StubLib(), _shape()
    w, w_rgb = _weight(), torch.randn(1, 1, 1, 8, 1).requires_grad_(True)
    frag = images.fragment(w, 1.0, False, shp, _lib.SG_BF16, lib, None)
    sub = images.subpixel(w, 1.0, shp, _lib.SG_BF16, lib, None)
    subd = images.subpixel(w, 1.0, shp, _lib.SG_BF16, lib, None, dgrad=True)
    mat = images.rgb_matrix(w_rgb, 0.5, torch.bfloat16)
    assert [n for n, a in lib.calls] == ['sg_conv3d_pack_weights', 'sg_upconv3d_subpixel_pack', 'sg_upconv3d_subpixel_dgrad_pack']
    assert torch.equal(mat, (w_rgb.detach().reshape(8, 1) * 0.5).to(torch.bfloat16).float().t()) and mat.shape == (1, 8)
    assert images.subpixel(w, 1.0, shp, _lib.SG_BF16, lib, None) is sub                  # all four are cached ...
    assert images.subpixel(w, 1.0, shp, _lib.SG_BF16, lib, None, dgrad=True) is subd
    assert images.rgb_matrix(w_rgb, 0.5, torch.bfloat16) is mat and len(lib.calls) == 3
    assert sorted(k.kind.name for k in images._entries) == ['fragment', 'rgb_matrix', 'subpixel_dgrad', 'subpixel_fwd']
    listed = images.live()                                                               # ... a captured step's list has no sub-pixel image
    assert len(listed) == 2 and any(t is frag for t in listed) and any(t is mat for t in listed)
    images.mark_stale()
    assert [k.kind for k in images._entries] == [WI.FRAGMENT] and images.stale is True
    assert len(images.live()) == 1 and images.live()[0] is frag
    assert images.stats == {'single': 1, 'batches': 0, 'batched': 0}                     # only fragment packs are counted


def test_mark_stale_with_drop_all_empties_the_cache(images):
    from saragan_amd import _lib
    lib, shp = StubLib(), _shape()
    w = _weight()
    images.fragment(w, 1.0, False, shp, _lib.SG_BF16, lib, None)
    images.subpixel(w, 1.0, shp, _lib.SG_BF16, lib, None)
    images.rgb_matrix(torch.randn(1, 1, 1, 8, 1), 1.0, torch.float32)
    images.mark_stale(drop_all=True)
    assert not images._entries and images.live() == [] and images.stale is False
    images.fragment(w, 1.0, False, shp, _lib.SG_BF16, lib, None)
    assert not lib.named('sg_conv3d_pack_weights_batch') and images.stats['single'] == 2


def test_functional_mark_packs_stale_reads_the_switch_of_the_moment(monkeypatch):
    """The launches below functional report rewritten parameters through IMAGES.params_rewritten: that is functional's
    mark_packs_stale, which reads NO_PACK_BATCH when it is called."""
    from saragan_amd import _lib, functional as F, optim_launch
    assert F.IMAGES.params_rewritten is F.mark_packs_stale and optim_launch.IMAGES is F.IMAGES
    lib, shp = StubLib(), _shape()
    w = _weight()
    F.clear_pack_cache()
    try:
        F.IMAGES.fragment(w, 1.0, False, shp, _lib.SG_BF16, lib, None)
        monkeypatch.setattr(F, '_NO_PACK_BATCH', False)
        F.IMAGES.params_rewritten()
        assert F.IMAGES.stale is True and len(F.live_packs()) >= 1
        monkeypatch.setattr(F, '_NO_PACK_BATCH', True)
        F.IMAGES.params_rewritten()
        assert F.IMAGES.stale is False and not F.IMAGES._entries
    finally:
        F.clear_pack_cache()


def test_only_images_of_long_lived_weights_are_kept(images):
    from saragan_amd import _lib
    lib, shp = StubLib(), _shape()
    leaf = _weight()
    transient = leaf * 2.0                          # a non-leaf that requires grad: a gradient of the double backward, say
    images.fragment(transient, 1.0, False, shp, _lib.SG_BF16, lib, None)
    images.subpixel(transient, 1.0, shp, _lib.SG_BF16, lib, None)
    assert not images._entries and len(lib.calls) == 2
    images.fragment(leaf, 1.0, False, shp, _lib.SG_BF16, lib, None)
    (ent,) = images._entries.values()
    assert ent.weight is leaf
    images.clear()
    flat = torch.randn(3, 3, 8, 8).requires_grad_(True)       # the 2-D networks' filters reach the kernels as views
    shp2 = _shape(k=3)
    shp2.kd = 1
    view = flat.unsqueeze(0)
    assert not view.is_leaf and view.requires_grad
    wp = images.fragment(view, 1.0, False, shp2, _lib.SG_BF16, lib, None)
    ((key, ent),) = images._entries.items()
    assert key.ptr == flat.data_ptr() and ent.image is wp
    assert ent.weight is not view and ent.weight.data_ptr() == flat.data_ptr()       # the detached alias: same storage and
    assert ent.weight.grad_fn is None and not ent.weight.requires_grad               # version counter, no autograd node
    assert ent.weight._version == flat._version
    assert images.fragment(flat.unsqueeze(0), 1.0, False, shp2, _lib.SG_BF16, lib, None) is wp      # the next step's view hits
    images.clear()
    half = _weight().detach().to(torch.bfloat16)    # not f32: the batch launch could not read it in place -- packed, not kept
    images.fragment(half, 1.0, False, shp, _lib.SG_BF16, lib, None)
    assert not images._entries
    view3 = torch.randn(27, 8, 8).requires_grad_(True).view(3, 3, 3, 8, 8)      # each kind has its own rule: the sub-pixel kinds
    images.subpixel(view3, 1.0, shp, _lib.SG_BF16, lib, None)                    # keep parameters themselves only,
    images.subpixel(view3, 1.0, shp, _lib.SG_BF16, lib, None, dgrad=True)
    assert not images._entries
    images.rgb_matrix(torch.randn(1, 1, 1, 8, 1).requires_grad_(True) * 2.0, 1.0, torch.float32)      # a matrix is kept always
    assert [k.kind.name for k in images._entries] == ['rgb_matrix']


def test_the_fragment_key_takes_host_numbers_as_they_come(images):
    """The hot lookup does not normalise coef / flip: whatever hashes and compares like the stored float / bool hits the same
    entry, and a value that cannot (it would miss, and pack, on every call) is refused where the image is built."""
    import numpy as np
    from saragan_amd import _lib
    from saragan_amd._scalars import DevCoef
    lib, shp = StubLib(), _shape()
    w = _weight()
    wp = images.fragment(w, DevCoef(0.5, torch.zeros(2), 1), 0, shp, _lib.SG_BF16, lib, None)
    ((key, _),) = images._entries.items()
    assert type(key.coef) is float and key.flip is False
    for coef, flip in ((0.5, False), (np.float32(0.5), 0), (np.float64(0.5), np.bool_(False))):
        assert images.fragment(w, coef, flip, shp, _lib.SG_BF16, lib, None) is wp
    assert images.stats['single'] == 1
    with pytest.raises(TypeError):
        images.fragment(w, torch.tensor(0.5), False, shp, _lib.SG_BF16, lib, None)


def test_below_functional_rewritten_parameters_mark_the_images_stale_without_a_switch():
    """Before functional is imported IMAGES.params_rewritten is the plain mark_stale (the switches live in functional)."""
    code = ('import sys\n'
            'from saragan_amd import optim_launch\n'
            'im = optim_launch.IMAGES\n'
            'assert "saragan_amd.functional" not in sys.modules and im.params_rewritten == im.mark_stale\n'
            'import saragan_amd.functional as F\n'
            'assert im.params_rewritten is F.mark_packs_stale\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- import order ---------------------------------------------------------------------------------------------------------------
BELOW = {'_launch': 'ndhwc', '_scalars': 'DevScalars', '_grad_dest': '_GRAD_DEST', '_consumers': 'BackInfo', '_weight_images': 'IMAGES',
         'loss_ops': 'sumsq_keep_w', 'augment': 'augment_draw', 'mbstd': 'mbstd_stat', 'cond': 'cond_embed',
         'optim_launch': 'SegmentTable', 'spectral': 'spectral_refresh_', 'guard': 'guard_step_', 'table_ops': 'gather_rows'}


def test_every_module_of_the_package_below_functional_is_listed():
    src = (ROOT / 'saragan_amd' / 'functional.py').read_text()
    assert set(re.findall(r'^from \.(\w+) import', src, re.M)) - {'_lib'} == set(BELOW)


@pytest.mark.parametrize('module', sorted(BELOW))
def test_module_below_functional_imports_first(module):
    """In a fresh interpreter the module is imported before anything else of the package's Python: it must not need functional,
    and functional's name is the module's object."""
    name = BELOW[module]
    code = (f'import sys, importlib\n'
            f'm = importlib.import_module("saragan_amd.{module}")\n'
            f'assert "saragan_amd.functional" not in sys.modules, "imports functional"\n'
            f'import saragan_amd.functional as F\n'
            f'assert F.{name} is m.{name}\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_no_module_below_functional_names_it_in_an_import():
    for module in BELOW:
        src = (ROOT / 'saragan_amd' / f'{module}.py').read_text()
        assert not re.search(r'^\s*(from|import)\s.*\bfunctional\b', src, re.M), module


# ---- re-export completeness -----------------------------------------------------------------------------------------------------
READ = re.compile(r'(?<![\w.])(?:F|functional|saragan_amd\.functional)\.([A-Za-z_]\w*)')


def _names_read_from_functional():
    files = [ROOT / 'bench.py']
    for top in ('saragan_amd', 'benchlib', 'oracle', 'tests', 'tools'):
        files += [p for p in sorted((ROOT / top).rglob('*.py')) if 'archive' not in p.relative_to(ROOT).parts[:2]]
    names = set()
    for p in files:
        src = p.read_text()
        if re.search(r'torch\.nn(\.| import )functional as F\b', src) or not re.search(r'\bfunctional\b', src):
            continue       # (another F)
        names.update(READ.findall(src))
    return names


def test_every_name_read_from_functional_is_there():
    """The expectation was collected at the commit before functional.py was split into layers (every name that was then read
    AND was an attribute), so the test cannot pass by both sides losing a name.  _PACK_CACHE and _PACK_STATE, which only
    test_packed_image_cache_states read, went with the loose dicts that test used to plant tuples in."""
    from saragan_amd import functional as F
    expected = set((ROOT / 'tests' / 'golden' / 'functional_names.txt').read_text().split())
    assert len(expected) > 100
    missing = sorted(n for n in expected if not hasattr(F, n))
    assert not missing, missing
    stray = {'py', '_NO_'}      # (prose: 'functional.py', 'F._NO_...')
    unknown = sorted(n for n in _names_read_from_functional() - expected - stray if not hasattr(F, n))
    assert not unknown, unknown
