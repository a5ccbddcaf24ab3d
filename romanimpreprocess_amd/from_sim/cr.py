"""Cosmic-ray hits -- the model of ``romanisim.cr`` with its function names and arguments, run on the device
(``csrc/cr.hip``: ``rip_synth_cr_tracks``, ``rip_synth_cr_deposit``).  romanisim is not part of the reference tree: the model is
restated from the published algorithm, every constant is a keyword, parity with romanisim is unpinned.
Within the model the arithmetic is exact given the deviates; the deviates come from the device's counter-based generator
(``rng``: an integer seed or a ``numpy.random.Generator`` as everywhere in ``from_sim``; without it, ``seed``).

``L1Synth.cosmic_rays`` (``sim_to_isim``) is the device-tensor way in; the two functions here take and return numpy arrays.
"""

import numpy as np

from .. import _native

# romanisim's keywords -> fields of rip_cr_params, with romanisim's defaults
DEFAULTS = {
    "flux": ("flux", 8.0), "area": ("area", 16.8), "conversion_factor": ("conversion_factor", 0.5),
    "pixel_size": ("pixel_size", 10.0), "pixel_depth": ("pixel_depth", 5.0),
    "min_dEdx": ("min_dedx", 10.0), "max_dEdx": ("max_dedx", 10000.0),
    "min_cr_len": ("min_len", 10.0), "max_cr_len": ("max_len", 2000.0), "grid_size": ("grid_size", 10000),
    "location": ("moyal_location", 120.0), "scale": ("moyal_scale", 50.0), "slope": ("len_slope", -4.33),
}


def params_from(crparam=None):
    """``_native.CrParams`` from a dict of any of the keywords of ``DEFAULTS`` (``{}`` or None: romanisim's defaults)."""
    crparam = dict(crparam or {})
    unknown = set(crparam) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown cosmic-ray parameter(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
    p = _native.CrParams()
    for key, (field, default) in DEFAULTS.items():
        v = crparam.get(key, default)
        setattr(p, field, int(v) if field == "grid_size" else float(v))
    return p


def capacity_for(par, nreads, read_time):
    """Rows for the tracks of ``nreads`` reads: the mean number plus ten sigma plus 64."""
    mean = nreads * par.flux * par.area * float(read_time)
    return int(mean + 10.0 * np.sqrt(mean) + 64.0)


def _seed(rng, seed):
    from .sim_to_isim import _seed_of

    return _seed_of(seed if rng is None else rng)


def _tracks(ctx, par, nreads, read_time, n_i, n_j, seed, counts, capacity):
    """(tracks (capacity, 6) f64, offsets (nreads+1,) i32) device tensors; ``counts``: tracks per read handed in, or None."""
    import torch

    dev = torch.device("cuda", ctx.device)
    tracks = torch.zeros((capacity, 6), dtype=torch.float64, device=dev)
    offsets = torch.zeros((nreads + 1,), dtype=torch.int32, device=dev)
    cnt = None if counts is None else torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(dev)
    torch.cuda.current_stream(dev).synchronize()   # torch's fills and copies are not on the context's stream
    ctx.call("rip_synth_cr_tracks", par, nreads, read_time, n_i, n_j, seed, cnt, None, capacity, tracks, offsets)
    ctx.synchronize()
    return tracks, offsets


def sample_cr_params(N_samples, N_i=4096, N_j=4096, min_dEdx=10, max_dEdx=10000, min_cr_len=10, max_cr_len=2000, grid_size=10000,
                     rng=None, seed=48, ctx=None):
    """``(cr_i, cr_j, cr_phi, cr_length, cr_dEdx)`` of ``N_samples`` tracks: start in pixels, direction in radians, length in
    micrometres, energy loss in eV per micrometre (``romanisim.cr.sample_cr_params``)."""
    ctx = ctx or _native.default_context()
    n = int(N_samples)
    if n < 1:
        return tuple(np.zeros(0) for _ in range(5))
    par = params_from({"min_dEdx": min_dEdx, "max_dEdx": max_dEdx, "min_cr_len": min_cr_len, "max_cr_len": max_cr_len,
                       "grid_size": grid_size})
    tracks, _ = _tracks(ctx, par, 1, 0.0, N_i, N_j, _seed(rng, seed), [n], n)
    t = tracks.cpu().numpy()
    return tuple(np.ascontiguousarray(t[:, q]) for q in range(1, 6))


def simulate_crs(image, time, flux=8, area=16.8, conversion_factor=0.5, pixel_size=10, pixel_depth=5, rng=None, seed=47, ctx=None):
    """Adds the cosmic-ray hits of ``time`` seconds to ``image`` (electrons; (N_i, N_j) numpy array) in place and returns it
    (``romanisim.cr.simulate_crs``)."""
    import torch

    ctx = ctx or _native.default_context()
    n_i, n_j = image.shape
    par = params_from({"flux": flux, "area": area, "conversion_factor": conversion_factor, "pixel_size": pixel_size,
                       "pixel_depth": pixel_depth})
    sd = _seed(rng, seed)
    tracks, offsets = _tracks(ctx, par, 1, time, n_i, n_j, sd, None, capacity_for(par, 1, time))
    dev = tracks.device
    added = torch.zeros((1, n_i, n_j), dtype=torch.int32, device=dev)
    first = torch.empty((n_i, n_j), dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    ctx.call("rip_synth_cr_deposit", par, 1, n_i, n_j, tracks, offsets, 1, sd, added, first, None)
    ctx.synchronize()
    image += added[0].cpu().numpy().astype(image.dtype)
    return image
