"""FITS headers written on the host (romanimpreprocess_amd/calio.py: fits_header) against tests/fits_out_ref.py, byte for byte,
and the restatement's own offset convention against the dark-stack reference.  No GPU is needed: only write_fits's data units
are encoded on the device (tests/test_gpu_fits_out.py)."""

import darkstack_ref as dr
import fits_out_ref as fr
import numpy as np
import pytest

from romanimpreprocess_amd import calio

SHAPES = [(), (7,), (3, 5), (2, 3, 5), (2, 1, 3, 5)]   # 0 to 4 axes
EXTRA = (("CDS", 0), ("ACN", 1.25), ("GOOD", True), ("BAD", False), ("OBSERVER", "O'Neil"), ("SHORT", "ab"), ("LONGER", "nine char"),
         ("NEG", -17), ("SMALL", 1e-05), ("HY-PHEN_", "x"))


def _check(shape, dtype, **kw):
    got = calio.fits_header(shape, dtype, **kw)
    want = fr.header(shape, dtype, **kw)
    assert isinstance(got, bytes) and len(got) % 2880 == 0
    assert got == want, f"{shape} {dtype} {kw}:\n{got[:800]!r}\n{want[:800]!r}"
    # ... and the package's reader takes every header back
    back = calio.parse_fits_header(got)
    parsed = fr.parse_hdus(got + (fr.data_unit(np.zeros(shape, dtype)) if shape else b""))[0][0]   # (no axes: no data unit)
    assert back == parsed
    if shape is not None:
        assert back["BITPIX"] == fr.BITPIX[np.dtype(dtype).name] and back["NAXIS"] == len(shape)
        assert [back[f"NAXIS{i + 1}"] for i in range(len(shape))] == list(shape[::-1])
    if kw.get("extname") is not None:
        assert back["EXTNAME"] == kw["extname"].rstrip()
    for k, v in kw.get("cards", ()):
        assert back[k] == v and type(back[k]) is type(v)
    return got


@pytest.mark.parametrize("dtype", fr.SUPPORTED)
def test_headers_equal_the_restatement(dtype):
    for shape in SHAPES:
        for extension in (False, True):
            for extname in (None, "MASK"):
                for cards in ((), EXTRA):
                    _check(shape, np.dtype(dtype), extension=extension, extname=extname, cards=cards)


def test_header_cards_by_hand():
    """a few cards spelled out, so that the restatement is not the only witness"""
    h = calio.fits_header((3, 5), np.uint16, cards=[("OBSERVER", "O'Neil")]).decode("ascii")
    cards = [h[i:i + 80] for i in range(0, len(h), 80)]
    assert cards[0] == "SIMPLE  =                    T".ljust(80)
    assert cards[1] == "BITPIX  =                   16".ljust(80)
    assert cards[2] == "NAXIS   =                    2".ljust(80)
    assert cards[3] == "NAXIS1  =                    5".ljust(80) and cards[4] == "NAXIS2  =                    3".ljust(80)
    assert cards[5] == "EXTEND  =                    T".ljust(80)
    assert cards[6] == "BSCALE  =                    1".ljust(80) and cards[7] == "BZERO   =                32768".ljust(80)
    assert cards[8] == "OBSERVER= 'O''Neil '".ljust(80)
    assert cards[9] == "END".ljust(80) and set(cards[10:]) == {" " * 80} and len(cards) == 36
    e = calio.fits_header((4,), np.int8, extension=True, extname="MASK").decode("ascii")
    assert e[:80] == "XTENSION= 'IMAGE   '".ljust(80)
    assert "PCOUNT  =                    0".ljust(80) + "GCOUNT  =                    1".ljust(80) in e
    assert "BZERO   =                 -128".ljust(80) + "EXTNAME = 'MASK    '".ljust(80) in e
    assert "BZERO   =           2147483648".ljust(80) in calio.fits_header((4,), np.uint32).decode("ascii")


def test_header_without_data():
    for extension in (False, True):
        got = _check(None, None, extension=extension)
        assert b"BITPIX  =                    8" in got and b"NAXIS   =                    0" in got and b"BZERO" not in got
    _check(None, None, extension=True, extname="EMPTY", cards=EXTRA)


def test_block_boundary():
    """SIMPLE, BITPIX, NAXIS, NAXIS1, EXTEND + 30 cards + END = 36 cards = one block; one card more needs a second block"""
    full = [(f"KEY{i:03d}", i) for i in range(30)]
    assert len(_check((4,), np.float32, cards=full)) == 2880
    assert _check((4,), np.float32, cards=full)[2880 - 80:2880 - 77] == b"END"
    over = _check((4,), np.float32, cards=full + [("LAST", "x")])
    assert len(over) == 2 * 2880 and over[2880:2883] == b"END" and over[2960:] == b" " * (2880 - 80)


@pytest.mark.parametrize("dtype", fr.REFUSED)
def test_refused_dtypes(dtype):
    with pytest.raises(TypeError) as err:
        calio.fits_header((3, 5), np.dtype(dtype))
    assert np.dtype(dtype).name in str(err.value)
    if dtype.startswith(">"):
        assert "byte order" in str(err.value)


def test_refused_cards():
    for cards, exc in (([("TOOLONGKEY", 1)], ValueError), ([("lower", 1)], ValueError), ([("X", float("nan"))], ValueError),
                       ([("X", "y" * 70)], ValueError), ([("X", None)], TypeError), ([("X", "é")], ValueError)):
        with pytest.raises(exc):
            calio.fits_header((2,), np.float32, cards=cards)


def test_restated_offsets_match_the_darkstack_reference():
    """uint16 under BZERO = 32768 is what darkstack_ref.to_fits_be16 / from_fits_be16 state; uint32 and int8 follow the same rule"""
    u16 = np.array([0, 1, 32767, 32768, 65534, 65535, 0x1234], np.uint16)
    assert fr.stored(u16) == dr.to_fits_be16(u16).tobytes()
    assert np.array_equal(dr.from_fits_be16(np.frombuffer(fr.stored(u16), ">i2")), u16)
    u32 = np.array([0, 2**31 - 1, 2**31, 2**32 - 1, 0x12345678], np.uint32)
    assert np.array_equal(np.frombuffer(fr.stored(u32), ">i4").astype(np.int64) + 2147483648, u32)
    i8 = np.array([-128, -1, 0, 127], np.int8)
    assert np.array_equal(np.frombuffer(fr.stored(i8), "u1").astype(np.int64) - 128, i8)
    # inverting the most significant bit of the native sample is that subtraction
    assert fr.stored(u16) == (u16 ^ np.uint16(0x8000)).astype(">u2").tobytes()
    assert fr.stored(u32) == (u32 ^ np.uint32(0x80000000)).astype(">u4").tobytes()
    assert fr.stored(i8) == (i8.view(np.uint8) ^ np.uint8(0x80)).tobytes()


def test_parser_walks_the_restated_file():
    rng = np.random.default_rng(3)
    items = [{"data": None}, {"data": rng.standard_normal((2, 3, 5)).astype(np.float32)},
             {"data": rng.integers(0, 2**32, (4, 9), dtype=np.uint32), "extname": "DQ"},
             {"data": rng.standard_normal(360), "cards": [("K", 1)]}]
    hdus = fr.parse_hdus(fr.fits_file(items))
    assert [h["NAXIS"] for h, _ in hdus] == [0, 3, 2, 1] and hdus[2][0]["EXTNAME"] == "DQ" and hdus[3][0]["K"] == 1
    assert len(hdus[3][1]) == 2880
    assert np.array_equal(fr.unit_array(*hdus[1]), items[1]["data"])
    assert np.array_equal(fr.unit_array(*hdus[2]).astype(np.int64) + 2**31, items[2]["data"])
