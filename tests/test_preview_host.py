"""CPU tests of the sample previews (saragan_amd/preview.py, functional.render_view's argument checks, the --preview_* flags):
the stdlib PNG encoder against a decoder that checks signature, CRCs and IHDR; the sheet and grid geometry against
tests/viewref.py; the parser's defaults and refusals; the wrapper's errors, raised before the library is loaded."""
import numpy as np
import pytest
import torch

from tests import viewref


# ---- PNG
@pytest.mark.parametrize('shape', [(1, 1), (1, 7), (5, 1), (33, 257), (2048, 2048)])
def test_png_bytes_decode_back_to_the_array(shape):
    from saragan_amd.preview import png_bytes
    a = np.random.default_rng(shape[0] * 4099 + shape[1]).integers(0, 256, shape, dtype=np.uint8)
    got, text = viewref.decode_png(png_bytes(a))
    assert got.shape == a.shape and (got == a).all() and text == {}


def test_png_text_chunks_round_trip(tmp_path):
    from saragan_amd.preview import png_bytes, write_png
    a = np.arange(12, dtype=np.uint8).reshape(3, 4)
    text = dict(phase=3, step=4096, views='slice_d,max_h', window='-1024.0,2048.0', seed=42, weights='EMA')
    got, back = viewref.decode_png(png_bytes(a, text))
    assert (got == a).all() and back == {k: str(v) for k, v in text.items()}
    path = write_png(tmp_path / 'a.png', a, text)
    assert open(path, 'rb').read() == png_bytes(a, text)


def test_png_refuses_what_it_cannot_encode():
    from saragan_amd.preview import png_bytes
    for bad in (np.zeros((2, 2), np.int16), np.zeros((2,), np.uint8), np.zeros((0, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)):
        with pytest.raises(ValueError, match='png_bytes'):
            png_bytes(bad)
    with pytest.raises(ValueError, match='keyword'):
        png_bytes(np.zeros((1, 1), np.uint8), {'k' * 80: 'v'})


def test_png_opens_with_pillow():
    Image = pytest.importorskip('PIL.Image')
    import io
    from saragan_amd.preview import png_bytes
    a = np.random.default_rng(5).integers(0, 256, (33, 257), dtype=np.uint8)
    im = Image.open(io.BytesIO(png_bytes(a, dict(phase=2))))
    assert im.mode == 'L' and im.size == (257, 33) and (np.asarray(im) == a).all()


# ---- views, layout
def test_view_names():
    from saragan_amd.preview import parse_view, parse_views, parse_window, default_window
    assert parse_view('slice_d') == ('slice', 0, None) and parse_view('slice_w:7') == ('slice', 2, 7)
    assert parse_view('max_h') == ('max', 1, None) and parse_view('mean_w') == ('mean', 2, None)
    assert parse_views('slice_d,slice_h,max_h') == [viewref.parse_view(v) for v in ('slice_d', 'slice_h', 'max_h')]
    for bad in ('slice', 'slice_x', 'min_d', 'max_d:3', 'slice_d:-1', 'slice_d:a', 'slice_d:', ''):
        with pytest.raises(ValueError):
            parse_views(bad) if bad == '' else parse_view(bad)
    assert parse_window('-1000,400.5') == (-1000.0, 400.5)
    for bad in ('1,1', '2,1', '1', '1,2,3', 'a,b', 'nan,1', '0,inf'):
        with pytest.raises(ValueError):
            parse_window(bad)
    assert default_window() == (-1.0, 2.0) and default_window(1024.0, 512.0) == (512.0, 2048.0)


@pytest.mark.parametrize('dims,views,zoom_d', [((4, 8, 16), ('slice_d', 'slice_h', 'max_w'), 1), ((4, 8, 16), ('max_w', 'mean_d'), 3),
                                               ((5, 7, 3), ('slice_h:2', 'slice_d', 'mean_w'), 2), ((1, 6, 9), ('slice_d',), 4)])
def test_sheet_layout_is_viewrefs(dims, views, zoom_d):
    """Mixed tile sizes: the layout preview.sheet hands the kernel equals the one viewref.sheet pastes with."""
    from saragan_amd.preview import parse_views, sheet_layout, view_zoom
    from saragan_amd.table_ops import view_tile
    x = np.random.default_rng(3).normal(0, 1, (3,) + dims).astype(np.float32)
    want = viewref.sheet(x, views, (-1.0, 2.0), zoom_d=zoom_d)
    parsed = parse_views(','.join(views))
    tops, heights, col_w = sheet_layout(dims, parsed, zoom_d)
    assert (sum(heights), 3 * col_w) == want.shape and tops == [sum(heights[:i]) for i in range(len(heights))]
    got = np.zeros_like(want)
    for (mode, axis, index), top, v in zip(parsed, tops, views):
        t = viewref.tiles(x, axis, mode, index, (-1.0, 2.0), zoom=view_zoom(axis, zoom_d))
        assert t.shape[1:] == view_tile(dims, axis, view_zoom(axis, zoom_d))
        viewref.place(got, t, origin=(top, 0), pitch=(t.shape[1], col_w))
    assert (got == want).all()


def test_grid_columns_are_the_references():
    from saragan_amd.preview import grid_cols_of
    assert [grid_cols_of(d) for d in (1, 2, 3, 4, 5, 15, 16, 17, 32, 64, 128)] == [1, 1, 1, 2, 2, 2, 4, 4, 4, 8, 8]
    x0 = np.arange(5 * 2 * 3, dtype=np.float32).reshape(5, 2, 3)
    g = viewref.slice_grid(x0, (0.0, 255.0))
    assert g.shape == (3 * 2, 2 * 3) and (g[2:4, 3:6] == x0[3]).all() and not g[4:6, 3:6].any()


def test_slerp_ends_and_arc():
    from saragan_amd.preview import slerp
    g = torch.Generator().manual_seed(1)
    z0, z1 = torch.randn(16, generator=g), torch.randn(16, generator=g)
    z = slerp(z0, z1, 5)
    assert z.shape == (5, 16) and torch.allclose(z[0], z0, atol=1e-6) and torch.allclose(z[-1], z1, atol=1e-6)
    norms, want = z.norm(dim=1), torch.linspace(float(z0.norm()), float(z1.norm()), 5)
    assert torch.allclose(norms, want, atol=1e-5)


# ---- parser
def _parse(extra):
    from saragan_amd.main import build_parser, finalize_args
    argv = ['pgan', '/data/', '--start_shape', '(1, 4, 4, 4)', '--final_shape', '(1, 32, 32, 32)', '--starting_phase', '2',
            '--ending_phase', '3', '--base_batch_size', '8', '--latent_dim', '16', '--network_size', 'xxs',
            '--noise_stddev', '0.01', '--mixing_nimg', '16', '--stabilizing_nimg', '16', '--loss_fn', 'logistic', '--gp_weight', '1']
    args, unknown = build_parser().parse_known_args(argv + extra)
    assert not unknown
    return finalize_args(args)


def test_parser_defaults_leave_previews_off():
    args = _parse([])
    assert args.preview_every_nsteps == 0 and args.preview_samples == 8 and args.preview_interp == 0
    assert args.preview_views == 'slice_d,slice_h,max_h' and args.preview_window is None and args.preview_zoom_d == 1


def test_parser_parses_views_and_window():
    args = _parse(['--preview_every_nsteps', '64'])
    assert args.preview_views == [('slice', 0, None), ('slice', 1, None), ('max', 1, None)] and args.preview_window == (-1.0, 2.0)
    args = _parse(['--preview_every_nsteps', '64', '--data_mean', '1024', '--data_stddev', '512'])
    assert args.preview_window == (512.0, 2048.0)
    args = _parse(['--preview_every_nsteps', '64', '--preview_window=-1000,400', '--preview_views', 'mean_w,slice_d:1',
                   '--preview_interp', '4', '--preview_zoom_d', '4', '--preview_samples', '3'])
    assert args.preview_window == (-1000.0, 400.0) and args.preview_views == [('mean', 2, None), ('slice', 0, 1)]
    assert (args.preview_interp, args.preview_zoom_d, args.preview_samples) == (4, 4, 3)


@pytest.mark.parametrize('extra,match', [
    (['--preview_every_nsteps', '16', '--preview_views', 'slice_q'], 'preview_views'),
    (['--preview_every_nsteps', '16', '--preview_views', ''], 'preview_views'),
    (['--preview_every_nsteps', '16', '--preview_window', '5,5'], 'preview_window'),
    (['--preview_every_nsteps', '16', '--preview_window', '5'], 'preview_window'),
    (['--preview_every_nsteps', '16', '--preview_samples', '0'], 'preview_samples'),
    (['--preview_every_nsteps', '16', '--preview_interp', '1'], 'preview_interp'),
    (['--preview_every_nsteps', '16', '--preview_interp', '-2'], 'preview_interp'),
    (['--preview_every_nsteps', '16', '--preview_interp', '4', '--preview_samples', '1'], 'preview_samples'),
    (['--preview_every_nsteps', '16', '--preview_zoom_d', '0'], 'preview_zoom_d'),
    (['--preview_every_nsteps', '-1'], 'preview_every_nsteps'),
    (['--preview_interp', '4'], 'preview_interp'),
])
def test_parser_refusals(extra, match):
    with pytest.raises(SystemExit, match=match):
        _parse(extra)


# ---- wrapper: every argument error is raised before the library is loaded
def test_render_view_argument_errors_need_no_library(monkeypatch):
    from saragan_amd import _lib, functional as F

    def no_library():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', no_library)
    x = torch.zeros(2, 3, 4, 5)
    with pytest.raises(TypeError, match='render_view: expected a tensor'):
        F.render_view(np.zeros((1, 2, 3, 4), np.float32), 0, 'max')
    with pytest.raises(TypeError, match='render_view: inputs are'):
        F.render_view(x.double(), 0, 'max')
    with pytest.raises(ValueError, match='render_view: expected \\[n, d, h, w\\]'):
        F.render_view(torch.zeros(3, 4, 5), 0, 'max')
    with pytest.raises(ValueError, match='contiguous'):
        F.render_view(torch.zeros(2, 3, 4, 10)[..., ::2], 0, 'max')
    for kw, match in ((dict(axis=3, mode='max'), 'axis'), (dict(axis=0, mode='min'), 'mode'),
                      (dict(axis=0, mode='slice', index=3), 'slice 3'), (dict(axis=2, mode='slice', index=-1), 'slice -1'),
                      (dict(axis=0, mode='max', index=1), 'index belongs to slices'),
                      (dict(axis=0, mode='max', window=(1.0, 1.0)), 'window'),
                      (dict(axis=0, mode='max', window=(0.0, float('inf'))), 'window'),
                      (dict(axis=0, mode='max', scale=float('nan')), 'scale'),
                      (dict(axis=0, mode='max', zoom=(0, 1)), 'zoom'), (dict(axis=0, mode='max', channel=1), 'channel'),
                      (dict(axis=0, mode='max', grid_cols=0), 'grid_cols'),
                      (dict(axis=0, mode='max', origin=(-1, 0)), 'origin'),
                      (dict(axis=0, mode='max', grid_cols=1, pitch=(3, 5)), 'pitch'),
                      (dict(axis=0, mode='max', canvas=torch.zeros(4, 9, dtype=torch.uint8)), 'outside the canvas'),
                      (dict(axis=0, mode='max', canvas=torch.zeros(4, 10, dtype=torch.uint8), origin=(1, 0)), 'outside the canvas'),
                      (dict(axis=0, mode='max', canvas=torch.zeros(4, 10)), 'canvas must be'),
                      (dict(axis=0, mode='max'), 'device tensor')):
        with pytest.raises(ValueError, match=match):
            F.render_view(x, **kw)
    with pytest.raises(ValueError, match='sheet'):
        from saragan_amd.preview import sheet
        sheet(x, 'slice_d', zoom_d=0)


# ---- command line: everything but the launches (the sheet itself: tests/test_render_view_gpu.py)
def test_command_line_reads_volumes_in_their_own_dtype(tmp_path, monkeypatch, capsys):
    from saragan_amd import preview
    rng = np.random.default_rng(2)
    vols = rng.integers(-1000, 3000, (5, 4, 6, 8)).astype(np.int16)
    (tmp_path / 'd').mkdir()
    for i, v in enumerate(vols):
        np.save(tmp_path / 'd' / f'{i:03d}.npy', v)
    np.save(tmp_path / 'batch.npy', vols[:, None].astype(np.float32))
    seen = []

    def fake_sheet(x, views, window, scale, shift, zoom_d):
        seen.append((x.dtype, tuple(x.shape), views, window, scale, shift, zoom_d))
        return viewref.sheet(x.numpy(), [preview._view_name(v) for v in views], window, scale, shift, zoom_d)
    monkeypatch.setattr(preview, 'sheet', fake_sheet)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    out = preview.main([str(tmp_path / 'd'), '--window=-500,2000', '--max_samples', '3', '--views', 'mean_w,slice_d:1', '--zoom_d', '2',
                        '--scale', '1.5', '--shift', '-10'], device='cpu')
    assert out == str(tmp_path / 'd' / 'preview.png') and 'Wrote' in capsys.readouterr().out
    assert seen[0] == (torch.int16, (3, 4, 6, 8), [('mean', 2, None), ('slice', 0, 1)], (-500.0, 2000.0), 1.5, -10.0, 2)
    img, text = viewref.decode_png(open(out, 'rb').read())
    assert (img == viewref.sheet(vols[:3], ('mean_w', 'slice_d:1'), (-500.0, 2000.0), 1.5, -10.0, 2)).all() and text['window'] == '-500,2000'
    out = preview.main([str(tmp_path / 'batch.npy'), '--window', '0,1', '--out', str(tmp_path / 'b.png')], device='cpu')
    assert out == str(tmp_path / 'b.png') and seen[1][:2] == (torch.float32, (5, 4, 6, 8))
    for argv in (['--window', '3,1'], ['--window', '0,1', '--views', 'slice_q'], ['--window', '0,1', '--max_samples', '0']):
        with pytest.raises(SystemExit, match='preview'):
            preview.main([str(tmp_path / 'd')] + argv, device='cpu')
