"""python -m saragan_amd.prepare_data on the device against its own numpy path: the six files of tests/test_pyramid_host.py give
byte-identical `.npy` files and an identical stats.json with --device cuda and with --device cpu."""
import os

import pytest

from tests.test_pyramid_host import SIX, TOOL_ARGS, run_tool, write_six

pytestmark = pytest.mark.gpu


def tree(root):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), 'rb').read() for dp, _, fs in os.walk(root) for f in fs}


def test_the_device_run_writes_the_bytes_of_the_cpu_run(tmp_path):
    src = str(tmp_path / 'src')
    write_six(src)
    trees = {}
    for device in ('cuda', 'cpu'):
        dst = str(tmp_path / device)
        r = run_tool(src, dst, *TOOL_ARGS, '--device', device)
        assert r.returncode == 0, r.stderr
        assert 'padded 6 / cropped 6 / files 6' in r.stdout and '--data_mean' in r.stdout
        trees[device] = tree(dst)
    assert sorted(trees['cuda']) == sorted(trees['cpu']) and len(trees['cuda']) == 3 * len(SIX) + 1
    assert 'stats.json' in trees['cuda']
    for name, data in trees['cuda'].items():
        assert data == trees['cpu'][name], name
