"""numpy restatement of the pixel-area map (test helper, not product code).

The arithmetic the kernel ``rip_stage_pixel_area`` (csrc/post.hip) implements, written out once more in numpy:
  * the WCS: 0-based pixel grid x = -1..nx, y = -1..ny (``coordutils.py:35``: ``np.linspace(-1, N, N+2)``), CRPIX as a 0-based
    pixel coordinate (``sim_to_isim.py:501-503``), SIP, CD, the zenithal projections of Calabretta & Greisen (2002) sect. 5.1
    and the spherical rotation of their eq. 2 -- what the reference gets from gwcs / astropy (``coordutils.py:37-55``);
  * the reference's own area arithmetic, line for line (``coordutils.py:57-81``): colatitude about the pole of the first grid
    point's hemisphere, ``rho = 2 sin(theta/2)``, ``u = rho cos(ra)``, ``v = rho sin(ra)``, central differences, ``|det|``.
``analytic_area`` is the closed form the restatement is checked against: the area element of each projection per unit
projection-plane area times |det CD| and the SIP Jacobian.
"""

import numpy as np

DEG = np.pi / 180.0


def sip_poly(coef, order, u, v):
    out = np.zeros_like(u)
    for p in range(order + 1):
        for q in range(order + 1 - p):
            if coef[p, q] != 0.0:
                out = out + coef[p, q] * (u**p * v**q)
    return out


def sip_jacobian(w, u, v):
    """d(u', v') / d(u, v) determinant of the SIP distortion (1 without SIP)"""
    if w.sip_order == 0:
        return np.ones_like(u)

    def d(coef, wrt):
        out = np.zeros_like(u)
        for p in range(w.sip_order + 1):
            for q in range(w.sip_order + 1 - p):
                c = coef[p, q]
                if c == 0.0:
                    continue
                if wrt == "u" and p > 0:
                    out = out + c * p * (u ** (p - 1) * v**q)
                if wrt == "v" and q > 0:
                    out = out + c * q * (u**p * v ** (q - 1))
        return out

    return (1.0 + d(w.sip_a, "u")) * (1.0 + d(w.sip_b, "v")) - d(w.sip_a, "v") * d(w.sip_b, "u")


def plane_coords(w, x, y):
    """(X, Y) in degrees on the projection plane, and (u, v) before SIP"""
    u, v = x - w.crpix[0], y - w.crpix[1]
    up, vp = u, v
    if w.sip_order > 0:
        up = u + sip_poly(w.sip_a, w.sip_order, u, v)
        vp = v + sip_poly(w.sip_b, w.sip_order, u, v)
    X = w.cd[0, 0] * up + w.cd[0, 1] * vp
    Y = w.cd[1, 0] * up + w.cd[1, 1] * vp
    return X, Y, u, v


def world(w, x, y):
    """(alpha, delta) in radians of 0-based pixel coordinates"""
    X, Y, _, _ = plane_coords(w, x, y)
    R = np.hypot(X, Y)
    phi = np.arctan2(X, -Y)
    theta = {
        "TAN": lambda: np.arctan2(180.0 / np.pi, R),
        "STG": lambda: np.pi / 2.0 - 2.0 * np.arctan(np.pi * R / 360.0),
        "ZEA": lambda: np.pi / 2.0 - 2.0 * np.arcsin(np.pi * R / 360.0),
        "ARC": lambda: (90.0 - R) * DEG,
        "SIN": lambda: np.arccos(np.pi * R / 180.0),
    }[w.projection]()
    d0, dphi = w.crval[1] * DEG, phi - w.lonpole * DEG
    delta = np.arcsin(np.sin(theta) * np.sin(d0) + np.cos(theta) * np.cos(d0) * np.cos(dphi))
    alpha = w.crval[0] * DEG + np.arctan2(-np.cos(theta) * np.sin(dphi),
                                          np.sin(theta) * np.cos(d0) - np.cos(theta) * np.sin(d0) * np.cos(dphi))
    return alpha, delta


def pixel_area(w, ny, nx, scale=1.0):
    """(ny, nx) f64 area / scale; ``coordutils.pixelarea(w, N)`` for ny = nx = N"""
    xx, yy = np.meshgrid(np.linspace(-1, nx, nx + 2), np.linspace(-1, ny, ny + 2))
    ra, dec = world(w, xx.ravel(), yy.ravel())
    # coordutils.py:61-81
    theta = np.pi / 2.0 + dec
    if dec[0] > 0:
        theta = np.pi / 2.0 - dec
    rho = 2.0 * np.sin(theta / 2.0)
    u = (rho * np.cos(ra)).reshape((ny + 2, nx + 2))
    v = (rho * np.sin(ra)).reshape((ny + 2, nx + 2))
    J11 = (u[1:-1, 2:] - u[1:-1, :-2]) / 2.0
    J12 = (u[2:, 1:-1] - u[:-2, 1:-1]) / 2.0
    J21 = (v[1:-1, 2:] - v[1:-1, :-2]) / 2.0
    J22 = (v[2:, 1:-1] - v[:-2, 1:-1]) / 2.0
    return np.abs(J11 * J22 - J21 * J12) / scale


def analytic_area(w, ny, nx, scale=1.0):
    """the exact solid angle per pixel (the Jacobian of pixel -> sphere at each pixel centre), / scale"""
    xx, yy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    X, Y, u, v = plane_coords(w, xx, yy)
    R = np.hypot(X, Y) * DEG   # radians
    element = {
        "TAN": lambda: (1.0 + R**2) ** -1.5,
        "STG": lambda: (1.0 + R**2 / 4.0) ** -2,
        "ZEA": lambda: np.ones_like(R),
        "ARC": lambda: np.where(R > 0, np.sin(R) / np.where(R > 0, R, 1.0), 1.0),
        "SIN": lambda: 1.0 / np.sqrt(1.0 - R**2),
    }[w.projection]()
    return element * abs(np.linalg.det(w.cd)) * DEG**2 * np.abs(sip_jacobian(w, u, v)) / scale


def fits_card(key, value):
    """one 80-character card as ``astropy.io.fits`` writes it"""
    if isinstance(value, str):
        v = "'" + value.replace("'", "''").ljust(8) + "'"
        s = f"{key:<8}= {v:<20}"
    elif isinstance(value, bool):
        s = f"{key:<8}= {('T' if value else 'F'):>20}"
    elif isinstance(value, int):
        s = f"{key:<8}= {value:>20d}"
    else:
        s = f"{key:<8}= {repr(float(value)).upper():>20}"
    return s.ljust(80)[:80]


def header_text(cards, layout="tofile"):
    """``cards``: list of (key, value) or raw card strings.  "tofile": 80-character cards, END, blanks to a multiple of 2880
    (``Header.tofile``); "lines": newline-separated cards"""
    lines = [c.ljust(80)[:80] if isinstance(c, str) else fits_card(*c) for c in cards]
    if layout == "lines":
        return "\n".join(ln.rstrip() for ln in lines + ["END"]) + "\n"
    text = "".join(lines) + "END".ljust(80)
    return text + " " * (-len(text) % 2880)


# the header the reference's workflow test writes (test_workflow.py:58-81), CRPIX moved to 0-based as sim_to_isim.py:501-503 does
WORKFLOW_N = 4088
WORKFLOW_CARDS = [
    ("SIMPLE", True), ("BITPIX", -64), ("NAXIS", 2), ("NAXIS1", 4088), ("NAXIS2", 4088), ("EXTEND", True),
    ("EXPTIME", 139.8), ("FILTER", "F184"),
    ("CRPIX1", (WORKFLOW_N + 1) / 2.0 - 1.0), ("CRPIX2", (WORKFLOW_N + 1) / 2.0 - 1.0),
    ("CD1_1", 3.0555555555555554e-05), ("CD1_2", 0.0), ("CD2_1", 0.0), ("CD2_2", 3.0555555555555554e-05),
    ("CTYPE1", "RA---TAN-SIP"), ("CTYPE2", "DEC--TAN-SIP"), ("CRVAL1", 37.0), ("CRVAL2", -20.0), ("LONPOLE", 215.0),
    ("A_ORDER", 2), ("A_0_2", 2.0e-6), ("A_1_1", -1.0e-6), ("A_2_0", 3.0e-6),
    ("B_ORDER", 2), ("B_0_2", 1.4e-5), ("B_1_1", -1.0e-5), ("B_2_0", 3.0e-7),
    ("RA_TARG", 37.0), ("DEC_TARG", -20.0), ("PA_OBSY", 185.0),
    "COMMENT truth wcs from sim_to_isim",
]


def simple_cards(proj, crval2, pixel_deg, n, sip=None, rot_deg=0.0, pc_form=False, lonpole=215.0, crval1=25.0):
    """cards of a zenithal WCS centred on an n x n frame: pixel scale ``pixel_deg``, rotation ``rot_deg`` (CD matrix, or the same
    as PC + CDELT with ``pc_form``), SIP terms ``sip`` = {"A_1_1": ..., ...} (order 2 .. 3)"""
    c, s = np.cos(rot_deg * DEG), np.sin(rot_deg * DEG)
    pc = np.array([[c, -s], [s, c]])
    cdelt = np.array([-pixel_deg, pixel_deg])
    suffix = "-SIP" if sip else ""
    lon, lat = ("RA---", "DEC--")
    cards = [("CTYPE1", f"{lon}{proj}{suffix}"), ("CTYPE2", f"{lat}{proj}{suffix}"),
             ("CRPIX1", (n - 1) / 2.0 + 3.25), ("CRPIX2", (n - 1) / 2.0 - 5.5),
             ("CRVAL1", crval1), ("CRVAL2", crval2), ("LONPOLE", lonpole), ("CUNIT1", "deg"), ("CUNIT2", "deg")]
    if pc_form:
        cards += [("CDELT1", cdelt[0]), ("CDELT2", cdelt[1])]
        cards += [(f"PC{i + 1}_{j + 1}", pc[i, j]) for i in range(2) for j in range(2)]
    else:
        cd = cdelt[:, None] * pc
        cards += [(f"CD{i + 1}_{j + 1}", cd[i, j]) for i in range(2) for j in range(2)]
    if sip:
        order = max(int(k.split("_")[1]) + int(k.split("_")[2]) for k in sip)
        cards += [("A_ORDER", order), ("B_ORDER", order)] + list(sip.items())
    return cards
