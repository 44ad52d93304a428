"""Reading and writing 3-D NRRD volumes (`.nrrd`, or a `.nhdr` header with a detached data file) in pure Python: zlib and numpy.

    array, header = read(path)        header = read_header(path)        write(path, array, spacing, ...)

The array comes back as [z, y, x] -- the file's `sizes` reversed, the fastest file axis last -- exactly as
sitk.GetArrayFromImage returns it: nothing is re-oriented, flipped or scaled.  Everything in the header record is given in the
ARRAY's axis order (z, y, x) too: `spacing[a]` is the voxel spacing along array axis a, `directions[a]` the world-space vector
(its x, y, z components, as the file writes them) of one step along array axis a.

Supported: `dimension: 3`; `type` int8, uint8, int16, uint16 or float in any of the format's spellings (`short`, `unsigned short`,
`uchar`, ...); `encoding` raw, gzip or gz; `endian`; `space directions` (with `space` / `space dimension: 3` and an optional
`space origin`) or `spacings`; a detached `data file:` with a plain relative name; `byte skip` (>= 0, or -1 for raw encoding: the
data are the file's last bytes).  Anything else that changes what the bytes mean -- 4-D files, `int`, `double`, `ascii`, `hex`,
`bzip2`, file lists, `line skip` -- is a ValueError naming the file and the field.  Descriptive fields and key/value pairs are
ignored."""
import os
import sys
import zlib
from collections import namedtuple

import numpy as np

MAGIC = b'NRRD000'
TYPES = {}
for _np, _names in (('int8', ('signed char', 'int8', 'int8_t')), ('uint8', ('uchar', 'unsigned char', 'uint8', 'uint8_t')),
                    ('int16', ('short', 'short int', 'signed short', 'signed short int', 'int16', 'int16_t')),
                    ('uint16', ('ushort', 'unsigned short', 'unsigned short int', 'uint16', 'uint16_t')), ('float32', ('float',))):
    for _n in _names:
        TYPES[_n] = _np
TYPE_OUT = {'int8': 'int8', 'uint8': 'uint8', 'int16': 'short', 'uint16': 'ushort', 'float32': 'float'}
ENCODINGS = {'raw': 'raw', 'gzip': 'gzip', 'gz': 'gzip'}
# fields that describe the data without changing how the bytes are read
IGNORED = {'content', 'number', 'kinds', 'labels', 'units', 'space units', 'thicknesses', 'axis mins', 'axismins', 'axis maxs',
           'axismaxs', 'centers', 'centerings', 'measurement frame', 'min', 'max', 'old min', 'oldmin', 'old max', 'oldmax',
           'sample units', 'sampleunits', 'block size', 'blocksize'}
ALIASES = {'byteskip': 'byte skip', 'lineskip': 'line skip', 'datafile': 'data file'}

Header = namedtuple('Header', 'dtype shape spacing directions origin space encoding endian data_file byte_skip data_offset fields')
Header.__doc__ = """dtype: a numpy dtype name; shape: the array's (z, y, x); spacing: (sz, sy, sx), the direction vectors' lengths or
`spacings`, None where the file gives neither; directions: three world vectors (x, y, z components), one per ARRAY axis, or None;
origin: the world position of voxel [0, 0, 0] or None; space: the `space` name or None; data_file: the detached file's path or
None; data_offset: where the data start in an attached file; fields: every `field: value` of the header as written."""


def _fail(path, field, why):
    raise ValueError(f'{path}: field {field!r}: {why}')


def _vector(path, field, text):
    t = text.strip()
    if not (t.startswith('(') and t.endswith(')')):
        _fail(path, field, f'expected a vector (a,b,c), got {text!r}')
    try:
        v = tuple(float(p) for p in t[1:-1].split(','))
    except ValueError:
        _fail(path, field, f'expected a vector of numbers, got {text!r}')
    if len(v) != 3:
        _fail(path, field, f'expected three components, got {text!r}')
    return v


def _parse(path, raw):
    """The header of the file's leading bytes `raw`: (fields, the offset behind the blank line or None if the file ended first)."""
    if not raw.startswith(MAGIC):
        _fail(path, 'magic', 'the file does not start with NRRD000x')
    fields, at, offset = {}, 0, None
    first = True
    while at < len(raw):
        end = raw.find(b'\n', at)
        if end < 0:
            line, nxt = raw[at:], len(raw)
        else:
            line, nxt = raw[at:end], end + 1
        at = nxt
        text = line.decode('ascii', 'replace').rstrip('\r')
        if first:
            first = False
            continue
        if text.strip() == '':
            offset = at
            break
        if text.startswith('#'):
            continue
        if ':=' in text and (': ' not in text or text.index(':=') < text.index(': ')):
            continue      # a key/value pair
        if ':' not in text:
            _fail(path, text, 'not a `field: value` line')
        name, value = text.split(':', 1)
        name = name.strip().lower()
        name = ALIASES.get(name, name)
        if name in fields:
            _fail(path, name, 'given twice')
        fields[name] = value.strip()
    return fields, offset


def _header_bytes(path):
    with open(path, 'rb') as f:
        raw = f.read(1 << 16)
        while b'\n\n' not in raw and b'\n\r\n' not in raw:
            more = f.read(1 << 16)
            if not more:
                break
            raw += more
    return raw


def read_header(path):
    """The Header record of an NRRD file; ValueError for anything this reader does not support."""
    path = os.fspath(path)
    fields, offset = _parse(path, _header_bytes(path))
    known = {'type', 'dimension', 'sizes', 'encoding', 'endian', 'space', 'space dimension', 'space directions', 'space origin',
             'spacings', 'data file', 'byte skip', 'line skip'}
    for name in fields:
        if name not in known and name not in IGNORED:
            _fail(path, name, 'not a field this reader knows')
    for need in ('type', 'dimension', 'sizes', 'encoding'):
        if need not in fields:
            _fail(path, need, 'missing')
    if fields['dimension'] != '3':
        _fail(path, 'dimension', f'{fields["dimension"]}; only 3-D volumes are read')
    tname = ' '.join(fields['type'].lower().split())
    if tname not in TYPES:
        _fail(path, 'type', f'{fields["type"]!r}; supported are int8, uint8, int16 (short), uint16 (ushort) and float')
    dtype = TYPES[tname]
    try:
        sizes = tuple(int(p) for p in fields['sizes'].split())
    except ValueError:
        sizes = ()
    if len(sizes) != 3 or min(sizes) < 1:
        _fail(path, 'sizes', f'{fields["sizes"]!r}; expected three positive integers')
    enc = fields['encoding'].lower()
    if enc not in ENCODINGS:
        _fail(path, 'encoding', f'{fields["encoding"]!r}; supported are raw and gzip')
    enc = ENCODINGS[enc]
    endian = None
    if 'endian' in fields:
        endian = fields['endian'].lower()
        if endian not in ('little', 'big'):
            _fail(path, 'endian', f'{fields["endian"]!r}; expected little or big')
    elif np.dtype(dtype).itemsize > 1:
        _fail(path, 'endian', f'missing for the {np.dtype(dtype).itemsize}-byte type {dtype}')
    if fields.get('line skip', '0') != '0':
        _fail(path, 'line skip', 'not supported')
    try:
        skip = int(fields.get('byte skip', '0'))
    except ValueError:
        _fail(path, 'byte skip', f'{fields["byte skip"]!r}; expected an integer')
    if skip < -1 or (skip == -1 and enc != 'raw'):
        _fail(path, 'byte skip', f'{skip} with encoding {enc}; -1 goes with raw encoding only')
    space = fields.get('space')
    if 'space dimension' in fields and fields['space dimension'] != '3':
        _fail(path, 'space dimension', f'{fields["space dimension"]}; expected 3')
    directions = spacing = origin = None
    if 'space directions' in fields:
        if 'spacings' in fields:
            _fail(path, 'spacings', 'given together with space directions')
        if space is None and 'space dimension' not in fields:
            _fail(path, 'space directions', 'given without space or space dimension')
        parts = fields['space directions'].replace(') (', ')|(').replace(')(', ')|(').split('|')
        parts = [p for chunk in parts for p in ([chunk] if '(' in chunk else chunk.split())]
        if len(parts) != 3:
            _fail(path, 'space directions', f'{fields["space directions"]!r}; expected three vectors')
        if any(p.strip().lower() == 'none' for p in parts):
            _fail(path, 'space directions', 'an axis without a direction (none); only spatial axes are read')
        vecs = [_vector(path, 'space directions', p) for p in parts]
        directions = tuple(reversed(vecs))      # file axes x, y, z -> array axes z, y, x
        spacing = tuple(float(np.sqrt(sum(c * c for c in v))) for v in directions)
        if min(spacing) <= 0 or not all(np.isfinite(spacing)):
            _fail(path, 'space directions', f'{fields["space directions"]!r}; a direction of length 0 or not finite')
    elif 'spacings' in fields:
        try:
            sp = tuple(float(p) for p in fields['spacings'].split())
        except ValueError:
            sp = ()
        if len(sp) != 3 or not all(np.isfinite(sp)) or 0.0 in sp:
            _fail(path, 'spacings', f'{fields["spacings"]!r}; expected three finite numbers, none 0')
        spacing = tuple(reversed(sp))
    if 'space origin' in fields:
        origin = _vector(path, 'space origin', fields['space origin'])
    data_file = None
    if 'data file' in fields:
        name = fields['data file']
        if name.upper().startswith('LIST') or '%' in name or len(name.split()) != 1:
            _fail(path, 'data file', f'{name!r}; file lists and numbered files are not supported')
        if os.path.isabs(name) or '..' in name.replace('\\', '/').split('/') or '\\' in name:
            _fail(path, 'data file', f'{name!r}; expected a plain relative name')
        data_file = os.path.join(os.path.dirname(path), name)
    elif offset is None:
        _fail(path, 'data file', 'the header ends without a blank line and names no data file')
    return Header(dtype, tuple(reversed(sizes)), spacing, directions, origin, space, enc, endian, data_file, skip, offset, fields)


def read(path):
    """(array [z, y, x] in native byte order, Header)."""
    path = os.fspath(path)
    h = read_header(path)
    src = h.data_file if h.data_file is not None else path
    with open(src, 'rb') as f:
        if h.data_file is None:
            f.seek(h.data_offset)
        blob = f.read()
    dt = np.dtype(h.dtype)
    count = h.shape[0] * h.shape[1] * h.shape[2]
    need = count * dt.itemsize
    if h.encoding == 'gzip':
        try:
            blob = zlib.decompress(blob, 16 + zlib.MAX_WBITS)
        except zlib.error as e:
            _fail(path, 'encoding', f'the gzip stream does not decompress: {e}')
        blob = blob[h.byte_skip:]
    elif h.byte_skip == -1:
        blob = blob[-need:] if len(blob) >= need else blob
    else:
        blob = blob[h.byte_skip:]
    if len(blob) < need:
        _fail(path, 'sizes', f'{h.shape[::-1]} of {h.dtype} need {need} bytes of data, the file holds {len(blob)}')
    order = '<' if (h.endian or sys.byteorder) == 'little' else '>'
    arr = np.frombuffer(blob, dtype=dt.newbyteorder(order) if dt.itemsize > 1 else dt, count=count).reshape(h.shape)
    return arr.astype(dt, copy=True), h


def _fmt(v):
    return repr(float(v))


def write(path, array, spacing, origin=None, directions=None, encoding='gzip', endian='little', data_file=None):
    """Writes array [z, y, x] (int8, uint8, int16, uint16 or float32).  spacing: (sz, sy, sx) along the ARRAY's axes.  Without
    origin and directions the header carries `spacings`; with either it carries `space: left-posterior-superior`, `space
    directions` (directions: three world vectors, one per array axis, whose lengths are then the spacing -- `spacing` may be
    None; default: the array's z, y, x along the world's z, y, x) and `space origin` (default 0).  encoding: raw or gzip.
    data_file: a plain relative name -- the data go there, next to `path`, and `path` is the detached header (`.nhdr`)."""
    path = os.fspath(path)
    a = np.asarray(array)
    if a.ndim != 3:
        raise ValueError(f'nrrd_io.write: a 3-D array [z, y, x], got {a.shape}')
    if a.dtype.name not in TYPE_OUT:
        raise ValueError(f'nrrd_io.write: int8, uint8, int16, uint16 or float32, got {a.dtype}')
    if encoding not in ENCODINGS:
        raise ValueError(f'nrrd_io.write: encoding is raw or gzip, got {encoding!r}')
    if endian not in ('little', 'big'):
        raise ValueError(f'nrrd_io.write: endian is little or big, got {endian!r}')
    enc = ENCODINGS[encoding]
    lines = ['NRRD0004', '# written by saragan_amd.nrrd_io', f'type: {TYPE_OUT[a.dtype.name]}', 'dimension: 3']
    if origin is None and directions is None:
        if spacing is None or len(spacing) != 3:
            raise ValueError('nrrd_io.write: spacing is (sz, sy, sx)')
        lines += ['sizes: ' + ' '.join(str(s) for s in a.shape[::-1]), 'spacings: ' + ' '.join(_fmt(s) for s in reversed(spacing))]
    else:
        if directions is None:
            if spacing is None or len(spacing) != 3:
                raise ValueError('nrrd_io.write: spacing is (sz, sy, sx)')
            directions = ((0.0, 0.0, spacing[0]), (0.0, spacing[1], 0.0), (spacing[2], 0.0, 0.0))
        if len(directions) != 3 or any(len(v) != 3 for v in directions):
            raise ValueError('nrrd_io.write: directions are three world vectors (x, y, z), one per array axis')
        origin = (0.0, 0.0, 0.0) if origin is None else origin
        vec = lambda v: '(' + ','.join(_fmt(c) for c in v) + ')'      # noqa: E731
        lines += ['space: left-posterior-superior', 'sizes: ' + ' '.join(str(s) for s in a.shape[::-1]),
                  'space directions: ' + ' '.join(vec(v) for v in reversed(directions)), 'kinds: domain domain domain',
                  'space origin: ' + vec(origin)]
    lines += [f'endian: {endian}', f'encoding: {enc}']
    if data_file is not None:
        if os.path.isabs(data_file) or os.path.basename(data_file) != data_file:
            raise ValueError(f'nrrd_io.write: data_file is a plain name next to the header, got {data_file!r}')
        lines.append(f'data file: {data_file}')
    blob = np.ascontiguousarray(a).astype(a.dtype.newbyteorder('<' if endian == 'little' else '>'), copy=False).tobytes()
    if enc == 'gzip':
        co = zlib.compressobj(6, zlib.DEFLATED, 16 + zlib.MAX_WBITS)
        blob = co.compress(blob) + co.flush()
    head = ('\n'.join(lines) + '\n').encode('ascii')
    if data_file is None:
        with open(path, 'wb') as f:
            f.write(head + b'\n' + blob)
    else:
        with open(os.path.join(os.path.dirname(path), data_file), 'wb') as f:
            f.write(blob)
        with open(path, 'wb') as f:
            f.write(head)
