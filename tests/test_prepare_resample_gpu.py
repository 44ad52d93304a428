"""python -m saragan_amd.prepare_data --spacing on the device against its own numpy path: the four sources of
tests/test_resample_host.py (two NRRD spacings, a permuted and flipped NRRD frame, a `.npy` with a spacing table) give
byte-identical `.npy` files and an identical stats.json with --device cuda and with --device cpu."""
import os

import pytest

from tests.test_pyramid_host import run_tool
from tests.test_resample_host import FOUR_ARGS, write_four

pytestmark = pytest.mark.gpu


def tree(root):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), 'rb').read() for dp, _, fs in os.walk(root) for f in fs}


@pytest.mark.parametrize('interp', ('linear', 'antialias'))
def test_the_device_run_writes_the_bytes_of_the_cpu_run(tmp_path, interp):
    src = str(tmp_path / 'src')
    _, table = write_four(src)
    trees = {}
    for device in ('cuda', 'cpu'):
        dst = str(tmp_path / device)
        r = run_tool(src, dst, *FOUR_ARGS, '--spacing_table', table, '--interp', interp, '--device', device)
        assert r.returncode == 0, r.stderr
        assert 'files 4 / discarded 0' in r.stdout and '--data_mean' in r.stdout
        trees[device] = tree(dst)
    assert sorted(trees['cuda']) == sorted(trees['cpu']) and len(trees['cuda']) == 2 * 4 + 1
    assert 'stats.json' in trees['cuda'] and b'"resample"' in trees['cuda']['stats.json']
    for name, data in trees['cuda'].items():
        assert data == trees['cpu'][name], name
