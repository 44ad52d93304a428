"""saragan_amd.nrrd_io: write -> read round trips over every supported type, encoding, byte order, attached and detached data,
`spacings` and `space directions`; hand-written headers (field order, blank lines, comments, byte skip: -1); and every rejected
field, which must be named together with the file.  No GPU."""
import gzip

import numpy as np
import pytest

TYPES = ('int8', 'uint8', 'int16', 'uint16', 'float32')


def volume(dtype, shape=(3, 4, 5), seed=0):
    rng = np.random.default_rng(seed)
    if dtype == 'float32':
        return rng.standard_normal(shape).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max + 1, shape).astype(dtype)


@pytest.mark.parametrize('dtype', TYPES)
@pytest.mark.parametrize('encoding', ('raw', 'gzip'))
@pytest.mark.parametrize('endian', ('little', 'big'))
@pytest.mark.parametrize('detached', (False, True))
def test_round_trip(tmp_path, dtype, encoding, endian, detached):
    from saragan_amd import nrrd_io
    a = volume(dtype)
    spacing = (3.0, 0.9765625, 0.7)
    path = str(tmp_path / ('v.nhdr' if detached else 'v.nrrd'))
    # `spacings`
    nrrd_io.write(path, a, spacing, encoding=encoding, endian=endian, data_file='v.bin' if detached else None)
    got, h = nrrd_io.read(path)
    assert got.dtype == a.dtype and got.dtype.isnative and got.flags.c_contiguous and np.array_equal(got, a)
    assert h.shape == a.shape and h.dtype == dtype and h.spacing == spacing and h.directions is None and h.origin is None
    assert h.space is None and h.encoding == encoding and h.endian == endian
    assert (h.data_file == str(tmp_path / 'v.bin')) if detached else (h.data_file is None)
    assert nrrd_io.read_header(path) == h
    # `space directions`, a flipped and permuted frame, an origin
    dirs = ((0.0, 0.0, -3.0), (0.5, 0.0, 0.0), (0.0, 0.25, 0.0))
    nrrd_io.write(path, a, None, origin=(1.5, -2.0, 10.0), directions=dirs, encoding=encoding, endian=endian,
                  data_file='v.bin' if detached else None)
    got, h = nrrd_io.read(path)
    assert np.array_equal(got, a) and h.directions == dirs and h.spacing == (3.0, 0.5, 0.25) and h.origin == (1.5, -2.0, 10.0)
    assert h.space == 'left-posterior-superior'
    # the default frame of a spacing and an origin: the array's z, y, x along the world's
    nrrd_io.write(path, a, spacing, origin=(0.0, 0.0, 0.0), encoding=encoding, endian=endian, data_file='v.bin' if detached else None)
    h = nrrd_io.read_header(path)
    assert h.directions == ((0.0, 0.0, 3.0), (0.0, 0.9765625, 0.0), (0.7, 0.0, 0.0)) and h.spacing == spacing


def test_the_array_is_the_files_sizes_reversed(tmp_path):
    from saragan_amd import nrrd_io
    a = np.arange(2 * 3 * 4, dtype=np.int16).reshape(2, 3, 4)      # x is the fastest axis: 4 voxels
    path = str(tmp_path / 'v.nrrd')
    nrrd_io.write(path, a, (1, 1, 1), encoding='raw')
    head = open(path, 'rb').read().split(b'\n\n')[0].decode()
    assert 'sizes: 4 3 2' in head and 'type: short' in head
    assert nrrd_io.read(path)[0][1, 2, 3] == 23


def handwritten(tmp_path, header, data, name='h.nrrd'):
    path = str(tmp_path / name)
    with open(path, 'wb') as f:
        f.write(header.encode('ascii') + data)
    return path


def test_handwritten_headers(tmp_path):
    from saragan_amd import nrrd_io
    a = volume('int16', (2, 3, 4))
    raw = a.astype('<i2').tobytes()
    # another field order, comments, a key/value pair, spellings of the type and of `byte skip`
    text = ('NRRD0005\n# a comment\nencoding: raw\nendian: little\nsizes: 4 3 2\n# another\ndimension: 3\ntype: signed short int\n'
            'kinds: domain domain domain\nmodality:=CT\nspace dimension: 3\nspace directions: (0.5,0,0) (0,0.5,0) (0,0,2)\n'
            'space origin: (1,2,3)\n\n')
    got, h = nrrd_io.read(handwritten(tmp_path, text, raw))
    assert np.array_equal(got, a) and h.spacing == (2.0, 0.5, 0.5) and h.origin == (1.0, 2.0, 3.0) and h.space is None
    # byte skip: -1 -- the data are the last bytes, whatever lies between
    text = 'NRRD0004\ntype: int16\ndimension: 3\nsizes: 4 3 2\nendian: little\nencoding: raw\nbyte skip: -1\nspacings: 0.5 0.5 2\n\n'
    got, h = nrrd_io.read(handwritten(tmp_path, text, b'junk before the data\n\n\x00\x01' + raw))
    assert np.array_equal(got, a) and h.byte_skip == -1 and h.spacing == (2.0, 0.5, 0.5)
    # a positive byte skip, big endian, `byteskip` in one word, CRLF line ends
    text = 'NRRD0004\r\ntype: ushort\r\ndimension: 3\r\nsizes: 4 3 2\r\nendian: big\r\nencoding: raw\r\nbyteskip: 5\r\n\r\n'
    b = volume('uint16', (2, 3, 4), seed=1)
    got, h = nrrd_io.read(handwritten(tmp_path, text, b'12345' + b.astype('>u2').tobytes()))
    assert np.array_equal(got, b) and h.endian == 'big' and h.spacing is None
    # gz, a one-byte type without `endian`, the skip applied to the decompressed stream
    c = volume('uint8', (2, 3, 4), seed=2)
    text = 'NRRD0004\ntype: unsigned char\ndimension: 3\nsizes: 4 3 2\nencoding: gz\nbyte skip: 3\n\n'
    got, h = nrrd_io.read(handwritten(tmp_path, text, gzip.compress(b'abc' + c.tobytes())))
    assert np.array_equal(got, c) and h.encoding == 'gzip' and h.endian is None
    # a detached header without the blank line
    with open(tmp_path / 'd.raw', 'wb') as f:
        f.write(raw)
    text = 'NRRD0004\ntype: short\ndimension: 3\nsizes: 4 3 2\nendian: little\nencoding: raw\ndata file: d.raw\n'
    got, h = nrrd_io.read(handwritten(tmp_path, text, b'', 'd.nhdr'))
    assert np.array_equal(got, a) and h.data_file == str(tmp_path / 'd.raw')


BASE = {'type': 'short', 'dimension': '3', 'sizes': '4 3 2', 'endian': 'little', 'encoding': 'raw'}
REJECTED = [
    ('dimension', {'dimension': '4', 'sizes': '4 3 2 1'}),
    ('type', {'type': 'int'}), ('type', {'type': 'double'}), ('type', {'type': 'unsigned int'}), ('type', {'type': 'block'}),
    ('encoding', {'encoding': 'ascii'}), ('encoding', {'encoding': 'bzip2'}), ('encoding', {'encoding': 'hex'}),
    ('data file', {'data file': 'LIST'}), ('data file', {'data file': 'slice%03d.raw 1 10 1'}), ('data file', {'data file': '/abs/v.raw'}),
    ('data file', {'data file': '../v.raw'}),
    ('sizes', {'sizes': '4 3'}), ('sizes', {'sizes': '4 0 2'}), ('endian', {'endian': 'middle'}), ('endian', {'endian': None}),
    ('line skip', {'line skip': '1'}), ('byte skip', {'byte skip': '-2'}), ('byte skip', {'byte skip': '-1', 'encoding': 'gzip'}),
    ('space directions', {'space dimension': '3', 'space directions': '(1,0,0) (0,1,0)'}),
    ('space directions', {'space dimension': '3', 'space directions': 'none (1,0,0) (0,1,0)'}),
    ('space directions', {'space directions': '(1,0,0) (0,1,0) (0,0,1)'}),
    ('space dimension', {'space dimension': '2'}), ('spacings', {'spacings': '1 1'}), ('spacings', {'spacings': '1 0 1'}),
    ('type', {'type': None}), ('encoding', {'encoding': None}), ('frobnicate', {'frobnicate': '1'}),
]


@pytest.mark.parametrize('field,change', REJECTED, ids=[f'{f}-{k}' for k, (f, _) in enumerate(REJECTED)])
def test_rejected_fields_name_the_file_and_the_field(tmp_path, field, change):
    from saragan_amd import nrrd_io
    fields = dict(BASE)
    fields.update(change)
    text = 'NRRD0004\n' + ''.join(f'{k}: {v}\n' for k, v in fields.items() if v is not None) + '\n'
    path = handwritten(tmp_path, text, bytes(48))
    with pytest.raises(ValueError) as e:
        nrrd_io.read(path)
    assert path in str(e.value) and repr(field) in str(e.value)
    with pytest.raises(ValueError):
        nrrd_io.read_header(path)


def test_other_failures(tmp_path):
    from saragan_amd import nrrd_io
    with pytest.raises(ValueError, match='magic'):
        nrrd_io.read(handwritten(tmp_path, 'NOPE\n\n', b''))
    text = 'NRRD0004\n' + ''.join(f'{k}: {v}\n' for k, v in BASE.items()) + '\n'
    with pytest.raises(ValueError, match='48 bytes'):
        nrrd_io.read(handwritten(tmp_path, text, bytes(47)))
    with pytest.raises(ValueError, match='encoding'):
        nrrd_io.read(handwritten(tmp_path, text.replace('raw', 'gzip'), b'not a gzip stream'))
    a = volume('int16')
    for bad in (dict(array=a[0]), dict(array=a.astype(np.int32)), dict(array=a.astype(np.float64)), dict(encoding='bzip2'),
                dict(endian='middle'), dict(spacing=(1, 1)), dict(spacing=None), dict(data_file='sub/v.raw'),
                dict(directions=((1, 0, 0), (0, 1, 0)))):
        kw = dict(array=a, spacing=(1, 1, 1))
        kw.update(bad)
        with pytest.raises(ValueError):
            nrrd_io.write(str(tmp_path / 'w.nrrd'), kw.pop('array'), kw.pop('spacing'), **kw)
