"""Coordinate-system utilities on the GPU -- same call surface as the reference's ``utils/coordutils.py``.

``pixelarea(inwcs, N)`` (:17-82) gives the solid angle of every pixel of an (N, N) frame from a WCS.  The reference evaluates an
astropy, GalSim or gwcs object on the host; ``calibrateimage`` hands it the exposure's ``FITSWCS`` header (gen_cal_image.py:64-87,
616-622).  Here the WCS is that header, parsed without astropy (``calio.parse_fits_header``) and validated by ``FitsWCS``; the map
itself comes from one HIP kernel (``rip_stage_pixel_area``, csrc/post.hip) in f64.

What is accepted: a celestial pair (``RA---``/``DEC--``, ``GLON``/``GLAT``, ``ELON``/``ELAT``, longitude on axis 1) of one zenithal
projection -- TAN, STG, ZEA, ARC or SIN -- optionally with ``-SIP`` (A/B orders up to 9), a CD matrix or CDELT (x PC), CUNIT
``deg``, LONPOLE (default 180).  Anything else (TPV, TNX, ``-TAB``, other projections, a linear WCS, other units, non-default
``PVi_m``, distortion tables) raises ValueError naming the keyword: no guessed substitute.

Conventions (unpinned): pixel coordinates are 0-based and the header's CRPIX is taken as a 0-based pixel
coordinate -- the gwcs convention ``sim_to_isim.py:501-503`` writes the header in ("offset from FITS -> GWCS convention").
"""

import hashlib

import numpy as np

from .. import _native, calio

_PROJECTIONS = {"TAN": _native.RIP_PROJ_TAN, "STG": _native.RIP_PROJ_STG, "ZEA": _native.RIP_PROJ_ZEA,
                "ARC": _native.RIP_PROJ_ARC, "SIN": _native.RIP_PROJ_SIN}
_PAIRS = {"RA--": "DEC-", "GLON": "GLAT", "ELON": "ELAT"}
_DISTORTION_KEYS = ("CPDIS1", "CPDIS2", "CQDIS1", "CQDIS2", "D2IMDIS1", "D2IMDIS2")


def _number(h, key, default=None):
    v = h.get(key, default)
    if v is None:
        raise ValueError(f"FITS WCS: {key} is missing")
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"FITS WCS: {key} = {v!r} is not a number")
    v = float(v)
    if not np.isfinite(v):
        raise ValueError(f"FITS WCS: {key} = {v!r} is not finite")
    return v


def _ctype(h, i):
    key = f"CTYPE{i}"
    c = h.get(key)
    if not isinstance(c, str):
        raise ValueError(f"FITS WCS: {key} is missing" if c is None else f"FITS WCS: {key} = {c!r} is not a string")
    c = c.strip().upper()
    if len(c) < 8 or c[4] != "-":
        raise ValueError(f"FITS WCS: {key} = {c!r} is not a celestial axis type (linear WCS not supported)")
    axis, proj, extra = c[:4], c[5:8], c[8:]
    if extra not in ("", "-SIP"):
        raise ValueError(f"FITS WCS: {key} = {c!r}: only the -SIP distortion is supported")
    if proj not in _PROJECTIONS:
        raise ValueError(f"FITS WCS: {key} = {c!r}: projection {proj} is not one of {', '.join(_PROJECTIONS)}")
    return axis, proj, extra == "-SIP"


def _sip_table(h, letter):
    okey = f"{letter}_ORDER"
    order = h.get(okey)
    if isinstance(order, bool) or not isinstance(order, int):
        raise ValueError(f"FITS WCS: {okey} is missing" if order is None else f"FITS WCS: {okey} = {order!r} is not an integer")
    if not 0 <= order <= _native.RIP_SIP_MAX_ORDER:
        raise ValueError(f"FITS WCS: {okey} = {order} outside 0..{_native.RIP_SIP_MAX_ORDER}")
    t = np.zeros((_native.RIP_SIP_MAX_ORDER + 1,) * 2)
    for key in h:
        parts = key.split("_")
        if len(parts) == 3 and parts[0] == letter and parts[1].isdigit() and parts[2].isdigit():
            p, q = int(parts[1]), int(parts[2])
            if p + q > order:
                raise ValueError(f"FITS WCS: {key} is above {okey} = {order}")
            t[p, q] = _number(h, key)
    return order, t


class FitsWCS:
    """A FITS celestial WCS of a zenithal projection (+SIP), parsed and validated: ``projection`` (TAN, STG, ZEA, ARC, SIN), ``crpix``
    (0-based), ``cd`` (2x2, degrees per pixel), ``crval``, ``lonpole`` (degrees), ``sip_order`` and the (10, 10) ``sip_a`` /
    ``sip_b`` tables indexed [p, q].  ``header``: the keyword dict it was made from."""

    def __init__(self, header):
        h = {str(k).upper(): v for k, v in dict(header).items()}
        self.header = h
        if h.get("WCSAXES", 2) != 2:
            raise ValueError(f"FITS WCS: WCSAXES = {h['WCSAXES']!r}: only two axes are supported")
        ax1, proj1, sip1 = _ctype(h, 1)
        ax2, proj2, sip2 = _ctype(h, 2)
        if _PAIRS.get(ax1) != ax2:
            raise ValueError(f"FITS WCS: CTYPE1 / CTYPE2 = {h['CTYPE1']!r} / {h['CTYPE2']!r} are not a longitude / latitude pair "
                             f"({', '.join(a + '/' + b for a, b in _PAIRS.items())})")
        if proj1 != proj2 or sip1 != sip2:
            raise ValueError(f"FITS WCS: CTYPE1 = {h['CTYPE1']!r} and CTYPE2 = {h['CTYPE2']!r} differ in projection")
        self.projection = proj1
        for i in (1, 2):
            unit = h.get(f"CUNIT{i}", "deg")
            if not isinstance(unit, str) or unit.strip().lower() not in ("deg", ""):
                raise ValueError(f"FITS WCS: CUNIT{i} = {unit!r}: only deg is supported")
        for key, v in h.items():
            if key.startswith(("PV", "PS")) and "_" in key and key[2:].split("_")[0].isdigit():
                if key == "PV1_2" and v == 90:   # theta_0 of a zenithal projection: the default
                    continue
                if key.startswith("PS") or v != 0:
                    raise ValueError(f"FITS WCS: {key} = {v!r}: projection parameters other than the defaults are not supported")
        for key in _DISTORTION_KEYS:
            if key in h:
                raise ValueError(f"FITS WCS: {key}: distortion tables are not supported")
        self.crpix = np.array([_number(h, "CRPIX1"), _number(h, "CRPIX2")])
        self.crval = np.array([_number(h, "CRVAL1"), _number(h, "CRVAL2")])
        if abs(self.crval[1]) > 90.0:
            raise ValueError(f"FITS WCS: CRVAL2 = {self.crval[1]} outside -90..90")
        self.lonpole = _number(h, "LONPOLE", 180.0)
        cd_keys = [f"CD{i}_{j}" for i in (1, 2) for j in (1, 2)]
        if any(k in h for k in cd_keys):
            self.cd = np.array([[_number(h, f"CD{i}_{j}", 0.0) for j in (1, 2)] for i in (1, 2)])
        else:
            if "CDELT1" not in h or "CDELT2" not in h:
                raise ValueError(f"FITS WCS: {'CDELT1' if 'CDELT1' not in h else 'CDELT2'} is missing (no CDi_j either)")
            for i in (1, 2):
                if h.get(f"CROTA{i}", 0) != 0:
                    raise ValueError(f"FITS WCS: CROTA{i}: the old rotation keyword is not supported (use PCi_j or CDi_j)")
            pc = np.array([[_number(h, f"PC{i}_{j}", 1.0 if i == j else 0.0) for j in (1, 2)] for i in (1, 2)])
            cdelt = np.array([_number(h, "CDELT1"), _number(h, "CDELT2")])
            self.cd = cdelt[:, None] * pc
        if np.linalg.det(self.cd) == 0.0:
            raise ValueError("FITS WCS: the CD matrix (CDi_j or CDELTi * PCi_j) is singular")
        self.sip_order = 0
        self.sip_a = np.zeros((_native.RIP_SIP_MAX_ORDER + 1,) * 2)
        self.sip_b = np.zeros_like(self.sip_a)
        if sip1:
            a_order, self.sip_a = _sip_table(h, "A")
            b_order, self.sip_b = _sip_table(h, "B")
            self.sip_order = max(a_order, b_order)
        elif "A_ORDER" in h or "B_ORDER" in h:
            raise ValueError(f"FITS WCS: {'A_ORDER' if 'A_ORDER' in h else 'B_ORDER'} is given but CTYPE1 = {h['CTYPE1']!r} has no -SIP")

    @classmethod
    def from_text(cls, text):
        return cls(calio.parse_fits_header(text))

    @classmethod
    def from_file(cls, path):
        with open(path, "rb") as f:
            return cls.from_text(f.read())

    def desc(self):
        """The ``rip_wcs_desc`` of this WCS (``_native.WcsDesc``)."""
        d = _native.WcsDesc()
        d.projection, d.sip_order = _PROJECTIONS[self.projection], int(self.sip_order)
        d.crpix[:] = self.crpix.tolist()
        d.crval[:] = self.crval.tolist()
        for i in range(2):
            d.cd[i][:] = self.cd[i].tolist()
        d.lonpole = float(self.lonpole)
        for p in range(_native.RIP_SIP_MAX_ORDER + 1):
            d.sip_a[p][:] = self.sip_a[p].tolist()
            d.sip_b[p][:] = self.sip_b[p].tolist()
        return d

    def digest(self):
        """sha256 of the descriptor: two headers that give the same map give the same digest."""
        return hashlib.sha256(bytes(self.desc())).hexdigest()


def as_wcs(inwcs):
    """``FitsWCS`` of a ``FitsWCS`` or of a header dict (``calio.parse_fits_header``); ValueError("Unrecognized WCS type") else,
    as the reference raises for an object it cannot evaluate (coordutils.py:55)."""
    if isinstance(inwcs, FitsWCS):
        return inwcs
    if isinstance(inwcs, dict):
        return FitsWCS(inwcs)
    raise ValueError("Unrecognized WCS type")


def pixelarea_map(inwcs, ny, nx, scale=1.0, device=False, ctx=None):
    """The (ny, nx) f64 map of pixel solid angles / ``scale`` (steradians for scale = 1; AreaFactor for ``pars.Omega_ideal``) on the
    grid x = -1..nx, y = -1..ny of 0-based pixel coordinates.  Equals the reference's ``pixelarea(w, N)`` for ny = nx = N.
    ``device=True``: a torch tensor on the context's GPU, complete when this returns; else a numpy array."""
    w = as_wcs(inwcs)
    ctx = ctx or _native.default_context()
    d = w.desc()
    if device:
        import torch

        dev = torch.device("cuda", ctx.device)
        out = torch.empty((int(ny), int(nx)), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()   # the library writes on its own stream
        ctx.call("rip_stage_pixel_area", d, ny, nx, scale, _native.RIP_DEVICE, out)
        ctx.synchronize()
        return out
    out = np.empty((int(ny), int(nx)), dtype=np.float64)
    ctx.call("rip_stage_pixel_area", d, ny, nx, scale, _native.RIP_HOST, out)
    return out


def pixelarea(inwcs, N=4088, ctx=None):
    """Generates an (N,N)-shaped array of the solid angles of the pixels in steradians (coordutils.py:17-82)."""
    return pixelarea_map(inwcs, N, N, ctx=ctx)
