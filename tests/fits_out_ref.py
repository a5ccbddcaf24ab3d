"""Independent numpy restatement of the FITS output (romanimpreprocess_amd/calio.py: fits_header, write_fits; device code:
csrc/fitsout.hip), from the fixed-format rules of the FITS standard (4.2.1 - 4.2.4: keyword in columns 1-8, "= " in 9-10, a
logical, an integer or a real right-justified to column 30, a string quoted from column 11, at least eight characters between
the quotes, a quote doubled) and its mandatory keywords (4.4.1.1 primary, 7.1.1 IMAGE extension; BZERO of the unsigned types:
table 11).  No comments are written, so the bytes are determined by the arguments.  astropy is not available here: these rules,
not its output, are the specification.  parse_hdus walks a file by 2880-byte blocks and returns the raw data bytes, so that the
tests read BITPIX 8 / 32 units without the package's own reader."""

import numpy as np
from darkstack_cases import _card

BLOCK = 2880
BITPIX = {"uint8": 8, "int8": 8, "int16": 16, "uint16": 16, "int32": 32, "uint32": 32, "float32": -32, "float64": -64}
# stored = value - BZERO, in the signed (for int8: unsigned) type of the same width
BZERO = {"uint16": (32768, ">i2"), "uint32": (2147483648, ">i4"), "int8": (-128, "u1")}
SUPPORTED = tuple(BITPIX)
REFUSED = ("bool", "float16", "int64", "uint64", "complex64", ">f4", ">i2", ">u4")


def header(shape, dtype, extension=False, extname=None, cards=()):
    """the header block(s) of one HDU as bytes; shape None: no data"""
    out = [_card("XTENSION", "IMAGE") if extension else _card("SIMPLE", True)]
    if shape is None:
        out += [_card("BITPIX", 8), _card("NAXIS", 0)]
    else:
        name = np.dtype(dtype).name
        out += [_card("BITPIX", BITPIX[name]), _card("NAXIS", len(shape))]
        out += [_card(f"NAXIS{i + 1}", int(n)) for i, n in enumerate(tuple(shape)[::-1])]
    out += [_card("PCOUNT", 0), _card("GCOUNT", 1)] if extension else [_card("EXTEND", True)]
    if shape is not None and np.dtype(dtype).name in BZERO:
        out += [_card("BSCALE", 1), _card("BZERO", BZERO[np.dtype(dtype).name][0])]
    if extname is not None:
        out.append(_card("EXTNAME", extname))
    out += [_card(k, v) for k, v in cards] + ["END".ljust(80)]
    assert all(len(c) == 80 for c in out)
    text = "".join(out)
    return (text + " " * (-len(text) % BLOCK)).encode("ascii")


def stored(arr):
    """the samples as FITS stores them, unpadded: the offset subtracted where the type has one, then big-endian"""
    arr = np.asarray(arr)
    if arr.dtype.name in BZERO:
        zero, kind = BZERO[arr.dtype.name]
        wide = arr.astype(np.int64) - zero
        assert wide.min(initial=0) >= np.iinfo(kind).min and wide.max(initial=0) <= np.iinfo(kind).max
        return wide.astype(kind).tobytes()
    return arr.astype(arr.dtype.newbyteorder(">")).tobytes()


def data_unit(arr):
    raw = stored(arr)
    return raw + b"\0" * (-len(raw) % BLOCK)


def hdu(arr, extension=False, extname=None, cards=(), mask=None, mask_sense=1, fill=0.0):
    """bytes of one HDU; with a mask, the float32 sample is `fill` where (mask != 0) == bool(mask_sense)"""
    if arr is None:
        return header(None, None, extension, extname, cards)
    arr = np.asarray(arr)
    if mask is not None:
        assert arr.dtype == np.float32
        arr = np.where((np.asarray(mask) != 0) == bool(mask_sense), np.float32(fill), arr)
    return header(arr.shape, arr.dtype, extension, extname, cards) + data_unit(arr)


def fits_file(items):
    """items: dicts with data / extname / cards / mask / mask_sense / fill, the first the primary HDU"""
    return b"".join(hdu(it.get("data"), extension=i > 0, extname=it.get("extname"), cards=it.get("cards", ()), mask=it.get("mask"),
                        mask_sense=it.get("mask_sense", 1), fill=it.get("fill", 0.0)) for i, it in enumerate(items))


# ---------------------------------------------------------------------------------------------- a tiny parser
def _value(field):
    s = field.strip()
    if s.startswith("'"):
        body = s[1:s.rindex("'")]
        return body.replace("''", "'").rstrip()
    if s in ("T", "F"):
        return s == "T"
    try:
        return int(s)
    except ValueError:
        return float(s)


def parse_hdus(raw):
    """[(header dict in card order, raw data bytes without the padding)] of a FITS file given as bytes: headers are read card by
    card up to END, the data unit is |BITPIX| / 8 * GCOUNT * (PCOUNT + NAXIS1 * ... * NAXISn) bytes, padded to a block"""
    assert len(raw) % BLOCK == 0, "a FITS file is a whole number of 2880-byte blocks"
    out, pos = [], 0
    while pos < len(raw):
        head, done = {}, False
        while not done:
            block = raw[pos:pos + BLOCK].decode("ascii")
            pos += BLOCK
            for i in range(0, BLOCK, 80):
                card = block[i:i + 80]
                if done:
                    assert card == " " * 80, "only blanks behind END"
                elif card[:8] == "END     ":
                    assert card[8:] == " " * 72
                    done = True
                else:
                    assert card[8:10] == "= ", card
                    head[card[:8].rstrip()] = _value(card[10:])
        naxis = head["NAXIS"]
        n = 0
        if naxis:
            n = abs(head["BITPIX"]) // 8 * head.get("GCOUNT", 1) * (head.get("PCOUNT", 0) + int(np.prod([head[f"NAXIS{i + 1}"] for i in range(naxis)], dtype=np.int64)))
        out.append((head, raw[pos:pos + n]))
        padded = n + (-n % BLOCK)
        assert raw[pos + n:pos + padded] == b"\0" * (padded - n), "the data unit is padded with zeros"
        pos += padded
    return out


def unit_array(head, raw):
    """the samples of a parsed HDU as stored (big-endian, offsets not applied), shape (NAXISn, ..., NAXIS1)"""
    kind = {8: "u1", 16: ">i2", 32: ">i4", -32: ">f4", -64: ">f8"}[head["BITPIX"]]
    return np.frombuffer(raw, dtype=kind).reshape([head[f"NAXIS{i}"] for i in range(head["NAXIS"], 0, -1)])
