"""numpy restatement of the two L2-output stage entries (csrc/l2out.hip) and of the members the reference adds to the L2 tree
after make_asdf.  Sources in the reference:
  L1_to_L2/gen_cal_image.py:653-662   make_asdf(slope[act], err_read[act] ** 2, err_poisson[act] ** 2, dq = pdq[act]); err of
                                      romanisim's make_asdf = sqrt(var_rnoise + var_poisson)
  L1_to_L2/oututils.py:46-49          border_ref_pix_left / _right / _top / _bottom = float32 edges of the Level-1 cube in the file
  L1_to_L2/oututils.py:52-55          dq_border_ref_pix_* = the same edges of the final pixel flags (full rows and columns)
  L1_to_L2/oututils.py:106-110        meta.calibration_software_name / _version
  utils/typefix.py:22-31              chisq, dumo: float16 zeros of data's shape, listed in meta.dummyfields
  utils/typefix.py:38-56              err, var_poisson, var_rnoise, var_flat as float16 (astype) where the schema asks for it
The reference writes 4 for the border; the entries take nb (slices written with explicit ends, so that nb = 0 gives empty strips).
"""

import numpy as np

SIDES = ("left", "right", "top", "bottom")
# what add_in_ref_data, add_in_provenance and typefix.fix add to `roman` (amp33 is copied by add_in_ref_data too; the tree had it)
REFERENCE_ADDED_ROMAN_KEYS = [
    "amp33", "border_ref_pix_left", "border_ref_pix_right", "border_ref_pix_top", "border_ref_pix_bottom",
    "dq_border_ref_pix_left", "dq_border_ref_pix_right", "dq_border_ref_pix_top", "dq_border_ref_pix_bottom", "chisq", "dumo"]
REFERENCE_ADDED_META_KEYS = ["calibration_software_name", "calibration_software_version", "dummyfields"]
SOFTWARE_NAME = "gen_cal_image / HLWAS PIT"
DUMMY_FIELDS = ["roman.chisq", "roman.dumo"]


def edges(a, nb):
    """(left, right, top, bottom) of the last two axes of ``a``: [..., :, :nb], [..., :, nx-nb:], [..., ny-nb:, :], [..., :nb, :]"""
    ny, nx = a.shape[-2:]
    return a[..., :, :nb], a[..., :, nx - nb:], a[..., ny - nb:, :], a[..., :nb, :]


def l2_planes(slope, err_read, err_poisson, pixeldq, nb, float16=False):
    ny, nx = slope.shape
    act = (slice(nb, ny - nb), slice(nb, nx - nb))
    with np.errstate(all="ignore"):
        var_r = np.multiply(err_read[act], err_read[act], dtype=np.float32)
        var_p = np.multiply(err_poisson[act], err_poisson[act], dtype=np.float32)
        err = np.sqrt(np.add(var_r, var_p, dtype=np.float32), dtype=np.float32)
        if float16:
            var_r, var_p, err = (a.astype(np.float16) for a in (var_r, var_p, err))
    out = {"data": slope[act].copy(), "dq": pixeldq[act].copy(), "var_rnoise": var_r, "var_poisson": var_p, "err": err}
    for side, strip in zip(SIDES, edges(pixeldq, nb)):
        out[f"dq_border_ref_pix_{side}"] = strip.copy()
    return out


def refpix_strips(cube, nb):
    return {f"border_ref_pix_{side}": np.ascontiguousarray(strip.astype(np.float32)) for side, strip in zip(SIDES, edges(cube, nb))}


def new_members(stored_cube, final_pixeldq, nb, data_shape, version):
    """(new members of roman, new members of roman.meta) for an exposure whose Level-1 cube is ``stored_cube`` in the file and
    whose final full-frame pixel flags are ``final_pixeldq``"""
    roman = refpix_strips(stored_cube, nb)
    for side, strip in zip(SIDES, edges(final_pixeldq, nb)):
        roman[f"dq_border_ref_pix_{side}"] = strip.copy()
    roman["chisq"] = np.zeros(data_shape, np.float16)
    roman["dumo"] = np.zeros(data_shape, np.float16)
    meta = {"calibration_software_name": SOFTWARE_NAME, "calibration_software_version": "romanimpreprocess_amd " + version,
            "dummyfields": list(DUMMY_FIELDS)}
    return roman, meta


def same_bits(got, want, what=""):
    """shape, dtype and bit patterns equal; NaNs compare by position, their sign and payload left open"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), f"{what}: NaNs at other positions ({gn.sum()} against {wn.sum()})"
        u = f"u{got.dtype.itemsize}"
        g, w = np.where(gn, 0, got.view(u)), np.where(wn, 0, want.view(u))
    else:
        g, w = got, want
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {np.unravel_index(bad[0], got.shape)}: " \
                          f"{got.reshape(-1)[bad[0]]!r} against {want.reshape(-1)[bad[0]]!r}"
