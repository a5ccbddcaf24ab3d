"""Calibration-file and L1/L2 file access for the host side.

The reference opens every file with ``asdf.open(path)`` and indexes ``f["roman"][...]``
(e.g. ``utils/ipc_linearity.py:170,183,324``, ``utils/fitting.py:201,207``).  ``open_tree`` gives the
same mapping for
  * a ``dict`` (already in memory: ``{"roman": {...}}`` or the ``roman`` branch itself),
  * an ``.npz`` mirror written by ``save_npz_tree`` (keys are '/'-joined paths),
  * an ``.asdf`` file: through the ``asdf`` package when it is installed, otherwise through the small
    reader below (ASDF 1.x: YAML tree + binary blocks, uncompressed / zlib / bzip2 blocks, ndarray
    tags with ``source``/``datatype``/``byteorder``/``shape``[/``offset``/``strides``], inline arrays).
``write_asdf`` writes such files (uncompressed blocks) so that synthetic CALDIR sets and L2 products
can be exchanged with the reference tooling.  ``parse_fits_header`` reads the FITS header text of an exposure's WCS
(``config["FITSWCS"]``, ``gen_cal_image.py:64-87``) without astropy; ``read_fits_image`` maps the image of one HDU of a FITS file
(the dark exposures and noise summaries of ``calfiles/make_dark_file.py``).  ``fits_header`` and ``write_fits`` write image HDUs
(the mask files, ``FITSOUT`` and the display dumps of the calibration-file scripts): the header on the host, the data units put
into FITS storage order on the GPU (``rip_stage_fits_encode``).  ``write_png`` writes an 8-bit RGB picture (``utils/fpaplot.py``), ``write_pdf_image`` the same raster as a one-page PDF (``utils/visualize.py``).
"""

import bz2
import contextlib
import hashlib
import io
import json
import os
import re
import struct
import zlib

import numpy as np
import yaml

_BLOCK_MAGIC = b"\xd3BLK"
_YAML_END = b"\n...\n"

_DT = {
    "int8": "i1", "int16": "i2", "int32": "i4", "int64": "i8", "uint8": "u1", "uint16": "u2", "uint32": "u4",
    "uint64": "u8", "float16": "f2", "float32": "f4", "float64": "f8", "complex64": "c8", "complex128": "c16",
    "bool8": "b1",
}
_DT_INV = {np.dtype(v).name: k for k, v in _DT.items()}
_DT_INV["bool"] = "bool8"


# ------------------------------------------------------------------------------- reading
class _Loader(yaml.SafeLoader):
    pass


class _NDArrayNode(dict):
    """mapping of an ndarray tag, resolved against the block list after the YAML pass"""


def _construct_any(loader, suffix, node):
    is_nd = "core/ndarray" in suffix or "core/ndarray" in getattr(node, "tag", "")
    if isinstance(node, yaml.MappingNode):
        m = loader.construct_mapping(node, deep=True)
        return _NDArrayNode(m) if is_nd else m
    if isinstance(node, yaml.SequenceNode):
        seq = loader.construct_sequence(node, deep=True)
        return _NDArrayNode({"data": seq}) if is_nd else seq
    return loader.construct_scalar(node)


_Loader.add_multi_constructor("", _construct_any)
_Loader.add_multi_constructor("!", _construct_any)
_Loader.add_multi_constructor("tag:", _construct_any)


def _read_blocks(buf, pos):
    blocks = []
    n = len(buf)
    while True:
        pos = buf.find(_BLOCK_MAGIC, pos)
        if pos < 0 or pos + 6 > n:
            break
        (hsize,) = struct.unpack(">H", buf[pos + 4 : pos + 6])
        hdr = buf[pos + 6 : pos + 6 + hsize]
        flags, comp, alloc, used, dsize = struct.unpack(">I4sQQQ", hdr[:32])
        start = pos + 6 + hsize
        raw = bytes(buf[start : start + used])
        comp = comp.rstrip(b"\0 ")
        if comp == b"zlib":
            raw = zlib.decompress(raw)
        elif comp == b"bzp2":
            raw = bz2.decompress(raw)
        elif comp not in (b"",):
            raise NotImplementedError(f"ASDF block compression {comp!r} is not supported by the in-repo reader")
        blocks.append(raw)
        pos = start + alloc
    return blocks


def _resolve(node, blocks):
    if isinstance(node, _NDArrayNode):
        dt = node.get("datatype", "float64")
        if not isinstance(dt, str):
            raise NotImplementedError("structured ASDF datatypes are not supported by the in-repo reader")
        dtype = np.dtype(_DT[dt]).newbyteorder("<" if node.get("byteorder", "little") == "little" else ">")
        if "source" in node:
            raw = blocks[int(node["source"])]
            shape = tuple(int(s) for s in node.get("shape", [len(raw) // dtype.itemsize]))
            off = int(node.get("offset", 0))
            if "strides" in node:
                arr = np.ndarray(shape, dtype=dtype, buffer=raw, offset=off, strides=tuple(node["strides"]))
            else:
                arr = np.frombuffer(raw, dtype=dtype, count=int(np.prod(shape, dtype=np.int64)), offset=off).reshape(shape)
            return arr.astype(dtype.newbyteorder("="), copy=False)
        return np.array(node["data"], dtype=dtype.newbyteorder("="))
    if isinstance(node, dict):
        return {k: _resolve(v, blocks) for k, v in node.items()}
    if isinstance(node, list):
        return [_resolve(v, blocks) for v in node]
    return node


def read_asdf(path):
    """Parse an ASDF file into nested dicts / lists / numpy arrays (in-repo reader)."""
    with open(path, "rb") as f:
        buf = f.read()
    if not buf.startswith(b"#ASDF"):
        raise ValueError(f"{path} is not an ASDF file")
    ystart = buf.find(b"%YAML")
    yend = buf.find(_YAML_END, ystart)
    if ystart < 0 or yend < 0:
        raise ValueError(f"{path}: no YAML tree found")
    tree = yaml.load(io.BytesIO(buf[ystart : yend + 1]), Loader=_Loader)  # noqa: S506 (SafeLoader subclass)
    blocks = _read_blocks(buf, yend + len(_YAML_END))
    return _resolve(tree, blocks)


# ------------------------------------------------------------------------------- writing
class _Dumper(yaml.SafeDumper):
    pass


class _ArrRef:
    def __init__(self, idx, arr):
        self.idx, self.arr = idx, arr


def _repr_arr(dumper, ref):
    a = ref.arr
    m = {"source": ref.idx, "datatype": _DT_INV[a.dtype.name], "byteorder": "little", "shape": [int(s) for s in a.shape]}
    return dumper.represent_mapping("!core/ndarray-1.0.0", m, flow_style=False)


_Dumper.add_representer(_ArrRef, _repr_arr)
_Dumper.add_representer(np.float64, lambda d, v: d.represent_float(float(v)))
_Dumper.add_representer(np.float32, lambda d, v: d.represent_float(float(v)))
_Dumper.add_representer(np.int64, lambda d, v: d.represent_int(int(v)))
_Dumper.add_representer(np.int32, lambda d, v: d.represent_int(int(v)))
_Dumper.add_representer(np.int16, lambda d, v: d.represent_int(int(v)))
_Dumper.add_representer(np.bool_, lambda d, v: d.represent_bool(bool(v)))


def _collect(node, blocks):
    if isinstance(node, np.ndarray):
        if node.ndim == 0:
            return node.item()
        a = np.ascontiguousarray(node)
        if a.dtype.byteorder == ">":
            a = a.astype(a.dtype.newbyteorder("<"))
        blocks.append(a)
        return _ArrRef(len(blocks) - 1, a)
    if isinstance(node, dict):
        return {str(k): _collect(v, blocks) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [_collect(v, blocks) for v in node]
    return node


def write_asdf(path, tree, checksum=False):
    """Write nested dicts / lists / scalars / numpy arrays as an ASDF 1.x file with uncompressed blocks.  ``checksum``: fill
    the optional MD5 field of every block header (the standard lets it be all zero = not verified; hashing a 4096 x 4096 x 8
    exposure's L2 tree costs 0.5 s, half of a whole ``calibrateimage`` call)."""
    blocks = []
    body = _collect(tree, blocks)
    text = yaml.dump(body, Dumper=_Dumper, default_flow_style=None, sort_keys=False)
    head = (b"#ASDF 1.0.0\n#ASDF_STANDARD 1.5.0\n%YAML 1.1\n%TAG ! tag:stsci.edu:asdf/\n--- !core/asdf-1.1.0\n")
    with open(path, "wb") as f:
        f.write(head)
        f.write(text.encode("utf-8"))
        f.write(b"...\n")
        for a in blocks:
            c = np.ascontiguousarray(a)
            raw = memoryview(c.reshape(-1).view(np.uint8)) if c.size else memoryview(b"")
            digest = hashlib.md5(raw).digest() if checksum else b"\0" * 16  # noqa: S324
            hdr = struct.pack(">I4sQQQ16s", 0, b"\0\0\0\0", raw.nbytes, raw.nbytes, raw.nbytes, digest)
            f.write(_BLOCK_MAGIC + struct.pack(">H", len(hdr)) + hdr)
            f.write(raw)


# ------------------------------------------------------------------------------- npz mirrors
def save_npz_tree(path, tree):
    """Flatten a nested dict of arrays/scalars into an .npz ('/'-joined keys)."""
    flat = {}

    def walk(prefix, node):
        if isinstance(node, dict):
            for k, v in node.items():
                walk(f"{prefix}/{k}" if prefix else str(k), v)
        elif isinstance(node, np.ndarray) or np.isscalar(node) and not isinstance(node, (str, bool)):
            flat[prefix] = np.asarray(node)
        else:  # lists (possibly ragged), strings, booleans, None: JSON text
            flat["json:" + prefix] = np.array(json.dumps(node))

    walk("", tree)
    np.savez(path, **flat)


def _load_npz_tree(path):
    tree = {}
    with np.load(path, allow_pickle=False) as f:
        for key in f.files:
            node = tree
            is_json = key.startswith("json:")
            parts = (key[5:] if is_json else key).split("/")
            for p in parts[:-1]:
                node = node.setdefault(p, {})
            v = f[key]
            node[parts[-1]] = json.loads(str(v)) if is_json else (v.item() if v.ndim == 0 else v)
    return tree


# ------------------------------------------------------------------------------- the one entry point
@contextlib.contextmanager
def open_tree(src):
    """Context manager yielding a mapping with a ``"roman"`` branch, like ``asdf.open(path)``."""
    if isinstance(src, dict):
        yield src if "roman" in src else {"roman": src}
        return
    path = os.fspath(src)
    if path.endswith(".npz"):
        t = _load_npz_tree(path)
        yield t if "roman" in t else {"roman": t}
        return
    try:
        import asdf  # noqa: PLC0415
    except ImportError:
        asdf = None
    if asdf is not None:
        with asdf.open(path) as f:
            yield f
        return
    yield read_asdf(path)


def roman_branch(src):
    """The ``roman`` branch with array leaves materialised as numpy arrays."""
    with open_tree(src) as f:
        return _materialise(f["roman"])


def _materialise(node):
    if isinstance(node, dict) or hasattr(node, "items"):
        return {k: _materialise(v) for k, v in node.items()}
    if hasattr(node, "shape") and hasattr(node, "dtype"):
        return np.asarray(node)
    return node


# ------------------------------------------------------------------------------- FITS header text
_FITS_INT = re.compile(r"[+-]?\d+\Z")
_FITS_FLOAT = re.compile(r"[+-]?(\d+\.?\d*|\.\d+)([EeDd][+-]?\d+)?\Z")


def _fits_value(key, text):
    """Value of a card's value field (the text after ``= ``): quoted string, logical, integer or float; None if empty."""
    s = text.lstrip()
    if s.startswith("'"):
        out, i = [], 1
        while True:
            j = s.find("'", i)
            if j < 0:
                raise ValueError(f"FITS header: unterminated string in {key}")
            out.append(s[i:j])
            if s[j + 1:j + 2] == "'":   # '' is a quote inside the string
                out.append("'")
                i = j + 2
                continue
            rest = s[j + 1:].strip()
            if rest and not rest.startswith("/"):
                raise ValueError(f"FITS header: text after the string of {key}: {rest!r}")
            return "".join(out).rstrip()
    token = s.split("/", 1)[0].strip()
    if token == "":
        return None
    if token in ("T", "F"):
        return token == "T"
    if _FITS_INT.match(token):
        return int(token)
    if _FITS_FLOAT.match(token):
        return float(token.replace("D", "E").replace("d", "e"))
    raise ValueError(f"FITS header: cannot read the value of {key}: {token!r}")


def parse_fits_header(text):
    """A FITS header given as text -> dict keyword -> value (str, bool, int, float or None), without astropy.

    Accepts what ``astropy.io.fits.Header.tofile`` writes (80-character cards with no separator, ``END``, blank padding to 2880
    bytes) and cards separated by newlines (what ``Header.fromstring(..., sep="\\n")`` reads).  Strings are unquoted (``''`` is a
    quote) with trailing blanks removed; ``/ comments`` are dropped; COMMENT, HISTORY, blank and other cards without a value
    indicator are skipped; a repeated keyword keeps its first value, as ``Header[key]`` does.  Reading stops at ``END``.  A value
    that is none of the above raises ValueError naming the keyword."""
    if isinstance(text, (bytes, bytearray)):
        text = text.decode("ascii")
    cards = []
    for line in text.splitlines():
        line = line.rstrip("\r")
        cards.extend(line[i:i + 80] for i in range(0, max(len(line), 1), 80))
    out = {}
    for card in cards:
        card = card.ljust(80)
        key = card[:8].strip().upper()
        if key == "END" and not card[8:].strip():
            break
        if key in ("", "COMMENT", "HISTORY") or card[8:10] != "= ":
            continue
        if key not in out:
            out[key] = _fits_value(key, card[10:])
    return out


# ------------------------------------------------------------------------------- FITS images
_FITS_BLOCK = 2880
_FITS_DTYPES = {16: ">i2", -32: ">f4", -64: ">f8"}


class FitsHeader(dict):
    """keyword -> value of one HDU (``parse_fits_header``); ``text`` is the header as stored, cards up to and including END"""

    text = ""


def read_fits_image(path, hdu=0, header_only=False):
    """``(header, data)`` of one HDU of a FITS file: the primary HDU (0) or an image extension, by index or by ``EXTNAME``.
    ``header`` is a dict (``FitsHeader``); ``data`` is a read-only memory map of the samples AS STORED -- big-endian int16,
    float32 or float64 (BITPIX 16 / -32 / -64), shape (NAXISn, ..., NAXIS1), ``BZERO`` / ``BSCALE`` not applied -- so that a 2 GB
    cube is not copied on the host; None for an HDU without data.  A last data block that is not padded to 2880 bytes is
    accepted.  Nothing else of FITS (tables, other BITPIX, compression, checksums) is read.  ``header_only``: ``(header, None)``
    whatever the HDU holds (a caller that wants to name what it refuses)."""
    path = os.fspath(path)
    size = os.path.getsize(path)
    want_name = hdu.strip().upper() if isinstance(hdu, str) else None
    with open(path, "rb") as f:
        pos, index = 0, 0
        while pos < size:
            f.seek(pos)
            raw = b""
            while True:
                block = f.read(_FITS_BLOCK)
                if len(block) < _FITS_BLOCK:
                    raise ValueError(f"{path}: the header of HDU {index} has no END card")
                raw += block
                cards = [block[i:i + 80] for i in range(0, _FITS_BLOCK, 80)]
                if any(c[:8] == b"END     " and not c[8:].strip() for c in cards):
                    break
            header = FitsHeader(parse_fits_header(raw))
            header.text = raw[:raw.find(b"END" + b" " * 77) + 80].decode("ascii")
            start = pos + len(raw)
            naxis = int(header.get("NAXIS", 0))
            shape = tuple(int(header[f"NAXIS{i}"]) for i in range(naxis, 0, -1))
            bitpix = int(header.get("BITPIX", 8))
            nbytes = abs(bitpix) // 8 * (int(header.get("PCOUNT", 0)) + int(np.prod(shape, dtype=np.int64))) * int(header.get("GCOUNT", 1)) \
                if naxis else 0
            if index == hdu if want_name is None else str(header.get("EXTNAME", "")).strip().upper() == want_name:
                if header_only or not naxis or not nbytes:
                    return header, None
                if index and header.get("XTENSION", "").strip() != "IMAGE":
                    raise ValueError(f"{path}: HDU {index} is not an image extension")
                if bitpix not in _FITS_DTYPES:
                    raise ValueError(f"{path}: BITPIX {bitpix} of HDU {index} is not supported (16, -32, -64)")
                if start + nbytes > size:
                    raise ValueError(f"{path}: HDU {index} needs {nbytes} bytes of data, the file ends after {size - start}")
                return header, np.memmap(path, dtype=_FITS_DTYPES[bitpix], mode="r", offset=start, shape=shape)
            pos = start + (nbytes + _FITS_BLOCK - 1) // _FITS_BLOCK * _FITS_BLOCK
            index += 1
    raise KeyError(f"{path}: no HDU {hdu!r}")


# ------------------------------------------------------------------------------- FITS output
# numpy dtype name -> (BITPIX, BZERO or None).  A BZERO type is stored with its most significant bit inverted.
_FITS_OUT = {"uint8": (8, None), "int8": (8, -128), "int16": (16, None), "uint16": (16, 32768), "int32": (32, None),
             "uint32": (32, 2147483648), "float32": (-32, None), "float64": (-64, None)}


def _fits_out_type(dtype):
    dtype = np.dtype(dtype)
    if dtype.name not in _FITS_OUT or not dtype.isnative:
        order = "" if dtype.isnative else " in non-native byte order"
        raise TypeError(f"FITS output: dtype {dtype.name}{order} is not supported ({', '.join(_FITS_OUT)}): cast the array first")
    return _FITS_OUT[dtype.name]


def _fits_card(key, value):
    """one fixed-format card without a comment: logicals, integers and floats right-justified to column 30, strings quoted,
    padded to eight characters, ``'`` doubled"""
    key = str(key)
    if not re.fullmatch(r"[A-Z0-9_-]{1,8}", key):
        raise ValueError(f"FITS output: {key!r} is not a keyword (1 to 8 of A-Z, 0-9, _ and -)")
    if isinstance(value, (bool, np.bool_)):
        text = f"{'T' if value else 'F':>20}"
    elif isinstance(value, (int, np.integer)):
        text = f"{int(value):>20d}"
    elif isinstance(value, (float, np.floating)):
        if not np.isfinite(value):
            raise ValueError(f"FITS output: {key} = {value!r} cannot be written as a number")
        text = f"{float(value)!r:>20}"
    elif isinstance(value, str):
        if not value.isascii() or not value.isprintable():
            raise ValueError(f"FITS output: the string of {key} is not printable ASCII")
        text = "'" + value.replace("'", "''").ljust(8) + "'"
    else:
        raise TypeError(f"FITS output: {key} = {value!r} is not a logical, an integer, a float or a string")
    card = f"{key:<8}= {text}"
    if len(card) > 80:
        raise ValueError(f"FITS output: the value of {key} does not fit into one card")
    return card.ljust(80)


def fits_header(shape, dtype, extension=False, extname=None, cards=()):
    """The header of one image HDU as bytes, a multiple of 2880: fixed-format cards without comments, so that the bytes are
    determined by the arguments -- SIMPLE (or XTENSION = 'IMAGE   '), BITPIX, NAXIS, NAXISn (NAXIS1 is the LAST numpy axis), EXTEND
    (primary) or PCOUNT and GCOUNT (extension), BSCALE = 1 and BZERO for uint16 / uint32 / int8, EXTNAME, then ``cards`` ((keyword,
    value) pairs: bool, int, float or str), END, blanks.  ``shape`` None: an HDU without data (BITPIX 8, NAXIS 0; ``dtype`` is not
    looked at).  Supported dtypes: uint8, int8, int16, uint16, int32, uint32, float32, float64 in native byte order; anything else
    (bool, float16, int64, ...) raises TypeError naming it -- the caller casts, as the reference's callers do.  Needs no GPU."""
    if shape is None:
        bitpix, bzero, shape = 8, None, ()
    else:
        bitpix, bzero = _fits_out_type(dtype)
        shape = tuple(int(s) for s in shape)
        if any(s < 0 for s in shape) or len(shape) > 999:
            raise ValueError(f"FITS output: shape {shape}")
    out = [_fits_card("XTENSION", "IMAGE") if extension else _fits_card("SIMPLE", True), _fits_card("BITPIX", bitpix),
           _fits_card("NAXIS", len(shape))]
    out += [_fits_card(f"NAXIS{i + 1}", s) for i, s in enumerate(shape[::-1])]
    out += [_fits_card("PCOUNT", 0), _fits_card("GCOUNT", 1)] if extension else [_fits_card("EXTEND", True)]
    if bzero is not None:
        out += [_fits_card("BSCALE", 1), _fits_card("BZERO", bzero)]
    if extname is not None:
        out.append(_fits_card("EXTNAME", str(extname)))
    out += [_fits_card(k, v) for k, v in cards]
    out.append("END".ljust(80))
    text = "".join(out)
    return (text + " " * (-len(text) % _FITS_BLOCK)).encode("ascii")


def _fits_unit(item, index):
    """one entry of ``write_fits``'s list -> (header bytes, data or None, on the device, mask or None, sense, fill)"""
    if item is None or hasattr(item, "dtype"):
        item = {"data": item}
    unknown = set(item) - {"data", "extname", "cards", "mask", "mask_sense", "fill"}
    if unknown:
        raise TypeError(f"write_fits: HDU {index}: unknown keys {sorted(unknown)}")
    data, mask = item.get("data"), item.get("mask")
    head = dict(extension=index > 0, extname=item.get("extname"), cards=item.get("cards", ()))
    if data is None:
        if mask is not None:
            raise ValueError(f"write_fits: HDU {index} has a mask and no data")
        return fits_header(None, None, **head), None, False, None, 0, 0.0
    on_device = not isinstance(data, np.ndarray)
    if not (hasattr(data, "ctypes") and hasattr(data, "shape")) or not data.flags.c_contiguous:
        raise ValueError(f"write_fits: HDU {index}: data must be a C-contiguous numpy array or a DevArray")
    header = fits_header(data.shape, data.dtype, **head)
    if mask is not None:
        if data.dtype != np.float32:
            raise TypeError(f"write_fits: HDU {index}: a mask goes with float32 data, not {data.dtype.name}")
        if (not isinstance(mask, np.ndarray)) != on_device:
            raise ValueError(f"write_fits: HDU {index}: data and mask must both be numpy arrays or both DevArrays")
        if mask.dtype not in (np.uint8, np.bool_) or tuple(mask.shape) != tuple(data.shape) or not mask.flags.c_contiguous:
            raise ValueError(f"write_fits: HDU {index}: the mask must be a C-contiguous uint8 or bool array of the data's shape")
    return header, data, on_device, mask, int(bool(item.get("mask_sense", 1))), float(item.get("fill", 0.0))


def write_fits(path, hdus, ctx=None, chunk_bytes=64 << 20):
    """Write a FITS file of image HDUs, replacing an existing one.  ``hdus``: a list whose entries are mappings with ``data``
    (None: no data unit; a numpy array; a ``DevArray``) and optionally ``extname``, ``cards`` (see ``fits_header``) and, for
    float32 data, ``mask`` (uint8 / bool, of the data's shape, living where the data live), ``mask_sense`` (default 1) and ``fill``:
    the sample is written as ``fill`` where ``(mask != 0) == bool(mask_sense)``.  A bare array or None stands for ``{"data": ...}``.
    The first entry is the primary HDU, the others are IMAGE extensions.

    Every data unit is put into FITS storage order on the GPU (``rip_stage_fits_encode``; there is no host fallback) in chunks of
    at most ``chunk_bytes``, each into one of two page-locked staging buffers; a writer thread puts chunk k into the file while
    chunk k + 1 is encoded and downloaded.  An array is therefore never held a second time in host memory, and an array in HBM
    comes to the host once, as the bytes of the file."""
    import queue
    import threading

    from . import _native

    units = [_fits_unit(item, i) for i, item in enumerate(hdus)]
    if not units:
        raise ValueError("write_fits: a FITS file has a primary HDU at least")
    ctx = ctx or _native.default_context()
    chunk = max(16, int(chunk_bytes) // 16 * 16)   # seams on 16-byte boundaries: the next chunk is as aligned as the array
    need = min(chunk, max([u[1].size * u[1].dtype.itemsize for u in units if u[1] is not None] + [16]))
    if ctx.fits_staging is None or ctx.fits_staging[0].nbytes < need:
        ctx.fits_staging = None   # (the old pair is returned before the new one is taken)
        ctx.fits_staging = [ctx.pinned_empty((need,), np.uint8) for _ in range(2)]
    staging = ctx.fits_staging
    todo, free, failed = queue.Queue(maxsize=4), queue.Queue(), []
    free.put(0)
    free.put(1)

    def writer(f):
        while True:
            job = todo.get()
            if job is None:
                return
            try:
                if not failed:
                    f.write(job if isinstance(job, bytes) else memoryview(staging[job[0]])[:job[1]])
            except Exception as e:   # noqa: BLE001 (handed to the caller; the queue is drained so that nobody waits for ever)
                failed.append(e)
            if not isinstance(job, bytes):
                free.put(job[0])

    with open(path, "wb") as f:
        thread = threading.Thread(target=writer, args=(f,), name="write_fits")
        thread.start()
        try:
            for header, data, on_device, mask, sense, fill in units:
                todo.put(header)
                if data is None or data.size == 0:
                    continue
                if on_device:
                    data.sync()
                bitpix, bzero = _fits_out_type(data.dtype)
                width = data.dtype.itemsize
                where = _native.location_of(data)
                step = chunk // width
                for first in range(0, data.size, step):
                    if failed:
                        break
                    n = min(step, data.size - first)
                    slot = free.get()
                    ctx.call("rip_stage_fits_encode", data.ctypes.data + first * width, bitpix, bzero is not None, n, where,
                             None if mask is None else mask.ctypes.data + first, sense, fill, staging[slot], _native.RIP_HOST)
                    todo.put((slot, n * width))
                todo.put(b"\0" * (-(data.size * width) % _FITS_BLOCK))
        finally:
            todo.put(None)
            thread.join()
    if failed:
        raise failed[0]


# ------------------------------------------------------------------------------- PNG
def write_png(path, arr, level=6):
    """An (ny, nx, 3) uint8 array as an 8-bit RGB PNG, rows in the order given (the picture of ``utils/fpaplot.py``; its script
    hands the rows over upside-down).  Unfiltered scanlines, deflated with the standard library's ``zlib``."""
    arr = np.asarray(arr)
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8 or arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError(f"write_png: expected a uint8 array (ny, nx, 3), got {arr.dtype}{arr.shape}")
    ny, nx, _ = arr.shape
    rows = np.zeros((ny, 1 + 3 * nx), np.uint8)   # every scanline starts with its filter type: 0, none
    rows[:, 1:] = arr.reshape(ny, 3 * nx)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", nx, ny, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + chunk(b"IEND", b""))


# ------------------------------------------------------------------------------- PDF
def write_pdf_image(path, arr, level=6):
    """An (ny, nx, 3) uint8 array as a one-page PDF 1.4 file that holds it as a single Flate-coded DeviceRGB image, rows in the
    order given (first row at the top), one pixel a point: what ``utils/visualize.py`` writes where the reference's command line
    names a ``.pdf``.  Host only (``zlib``)."""
    arr = np.asarray(arr)
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8 or arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError(f"write_pdf_image: expected a uint8 array (ny, nx, 3), got {arr.dtype}{arr.shape}")
    ny, nx, _ = arr.shape
    data = zlib.compress(np.ascontiguousarray(arr).tobytes(), level)
    draw = f"q {nx} 0 0 {ny} 0 0 cm /Im0 Do Q".encode("ascii")
    objects = [
        b"<< /Type /Catalog /Pages 2 0 R >>",
        b"<< /Type /Pages /Kids [3 0 R] /Count 1 >>",
        f"<< /Type /Page /Parent 2 0 R /MediaBox [0 0 {nx} {ny}] /Resources << /XObject << /Im0 4 0 R >> >> /Contents 5 0 R >>".encode("ascii"),
        (f"<< /Type /XObject /Subtype /Image /Width {nx} /Height {ny} /ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /FlateDecode "
         f"/Length {len(data)} >>\nstream\n").encode("ascii") + data + b"\nendstream",
        f"<< /Length {len(draw)} >>\nstream\n".encode("ascii") + draw + b"\nendstream",
    ]
    out, offsets = bytearray(b"%PDF-1.4\n%\xe2\xe3\xcf\xd3\n"), []
    for i, body in enumerate(objects):
        offsets.append(len(out))
        out += f"{i + 1} 0 obj\n".encode("ascii") + body + b"\nendobj\n"
    xref = len(out)
    out += f"xref\n0 {len(objects) + 1}\n".encode("ascii") + b"0000000000 65535 f \n"
    out += b"".join(f"{o:010d} 00000 n \n".encode("ascii") for o in offsets)
    out += f"trailer\n<< /Size {len(objects) + 1} /Root 1 0 R >>\nstartxref\n{xref}\n%%EOF".encode("ascii")
    with open(path, "wb") as f:
        f.write(out)
