"""Drop-in for the ``test_run.py`` lines of the reference's ``runs/2026_July/make_sca_files_2026Jul.job`` (lines 48-64), i.e. for
``solid_waffle.correlation_run.run_ir_all``: the superpixel summary of gain and inter-pixel capacitance from a set of flats and
darks, the pair statistics on the GPU (``corrstack.py``, ``csrc/corrstat.hip``).

    python -m romanimpreprocess_amd.calfiles.correlation_run <config>

``<config>`` is the text ``write_solid-waffle_config.pl`` prints, one ``KEY: value`` a line: ``DETECTOR``; ``LIGHT:`` and ``DARK:``, each
followed by one file a line up to the next key; ``FORMAT`` (1: the ``2026_July`` cubes, 6: the ``summer2025`` ones, the two layouts
of ``make_dark_file._open_dark``); ``TIMEREF``; ``NBIN nx ny``; ``TIME a b c d`` (frames counted from 1); ``OUTPUT``; and ``CHAR``,
``FULLNL``, ``NLPOLY``, ``IPCSUB``, ``HOTPIX``, which are accepted because the job's configuration must work as typed, and printed as
not acted on: this is solid-waffle's ``CHAR: Basic`` level.  Exposures are paired in list order (1,2), (3,4),
...; an odd last one is left out and said so; every file is read once.  Written: ``<OUTPUT>_summary.txt``, which ``np.loadtxt``
reads back to the same float64, and ``<OUTPUT>_config.txt``, the configuration verbatim (``make_gain_file`` puts it into ``notes``).
solid-waffle's source is not part of the reference: the estimator is the one of ``corrstack.py``, parity is unpinned.
"""

import re
import sys
from collections import namedtuple

import numpy as np

from .. import pars
from . import make_gain_file
from .corrstack import NCOL, CorrStack, check_frames, check_geometry, solve_summary
from .make_dark_file import _dev_cube, _open_dark

FORMATS = {1: "2026_July", 6: "summer2025"}
LIST_KEYS = ("LIGHT", "DARK")
NOT_ACTED_ON = ("CHAR", "FULLNL", "NLPOLY", "IPCSUB", "HOTPIX")
KEYS = ("DETECTOR",) + LIST_KEYS + ("FORMAT", "TIMEREF", "NBIN", "TIME", "OUTPUT") + NOT_ACTED_ON
REQUIRED = LIST_KEYS + ("FORMAT", "NBIN", "TIME", "OUTPUT")
HEADER = "# X Y N graw g_linear g alphaH alphaV beta I alphaD"

Config = namedtuple("Config", "detector light dark layout timeref nbin frames output ignored text")
_KEY = re.compile(r"^([A-Z][A-Z0-9_]*):(.*)$")


def parse_config(text):
    """The configuration text as a ``Config``: ``frames`` 0-based, ``nbin`` ``(nbx, nby)``, ``ignored`` the (key, value) pairs that
    are accepted and not acted on, ``text`` the configuration itself.  ValueError naming the key for an unknown or repeated key, a
    missing one, a value that does not parse, a file line outside a list, fewer than 2 light or dark exposures."""
    values, files, current = {}, {k: [] for k in LIST_KEYS}, None
    for raw in text.splitlines():
        line = raw.strip()
        if not line or line.startswith("#"):
            continue
        m = _KEY.match(line)
        if m is None:
            if current is None:
                raise ValueError(f"correlation_run: the line {line!r} is neither a key nor a file of LIGHT or DARK")
            files[current].append(line)
            continue
        key, value = m.group(1), m.group(2).strip()
        if key not in KEYS:
            raise ValueError(f"correlation_run: unknown key {key} (known: {', '.join(KEYS)})")
        if key in values:
            raise ValueError(f"correlation_run: {key} is given twice")
        values[key] = value
        current = key if key in LIST_KEYS else None
        if current and value:
            files[current].append(value)
    for key in REQUIRED:
        if key not in values:
            raise ValueError(f"correlation_run: {key} is missing")

    def ints(key, n):
        try:
            v = [int(s) for s in values[key].split()]
        except ValueError:
            v = []
        if len(v) != n:
            raise ValueError(f"correlation_run: {key}: {values[key]!r} ({n} integer{'s' if n > 1 else ''} needed)")
        return v

    fmt = ints("FORMAT", 1)[0]
    if fmt not in FORMATS:
        raise ValueError(f"correlation_run: FORMAT {fmt} (known: {sorted(FORMATS)})")
    try:
        timeref = float(values.get("TIMEREF", "0"))
    except ValueError:
        raise ValueError(f"correlation_run: TIMEREF: {values['TIMEREF']!r} (a number needed)") from None
    nbin = tuple(ints("NBIN", 2))
    if min(nbin) < 1:
        raise ValueError(f"correlation_run: NBIN {nbin[0]} {nbin[1]} (positive counts needed)")
    try:
        frames = check_frames([t - 1 for t in ints("TIME", 4)])
    except ValueError as e:
        raise ValueError(f"correlation_run: {e}") from None
    for key in LIST_KEYS:
        if len(files[key]) < 2:
            raise ValueError(f"correlation_run: {key}: {len(files[key])} exposures (at least 2 needed: the statistics are of pairs)")
    if not values["OUTPUT"]:
        raise ValueError("correlation_run: OUTPUT is empty")
    ignored = [(k, values[k]) for k in NOT_ACTED_ON if k in values]
    return Config(values.get("DETECTOR", ""), files["LIGHT"], files["DARK"], FORMATS[fmt], timeref, nbin, frames, values["OUTPUT"], ignored,
                  text)


def format_summary(table):
    """the summary table as text: one row a line, every number as the shortest text that reads back to the same float64"""
    rows = [HEADER]
    for row in np.asarray(table, np.float64):
        rows.append(" ".join(repr(float(v)) for v in row))
    return "\n".join(rows) + "\n"


def write_outputs(cfg, table):
    """``<OUTPUT>_summary.txt`` and ``<OUTPUT>_config.txt``; returns the two paths"""
    summary, config = cfg.output + "_summary.txt", cfg.output + "_config.txt"
    with open(summary, "w") as f:
        f.write(format_summary(table))
    with open(config, "w") as f:
        f.write(cfg.text)
    return summary, config


def _stack(files, cfg, which, nside, nb, ctx):
    """the ``CorrStack`` of one list of exposures (paths, or ``DevArray`` cubes), paired in list order, each read once"""
    from ..devarray import is_dev

    if len(files) % 2:
        print(f"{which}: {len(files)} exposures: the last one, {files[-1] if isinstance(files[-1], str) else '(a cube)'}, has no "
              "partner and is left out")
    stack = None
    for j in range(0, len(files) - 1, 2):
        pair = []
        for f in files[j:j + 2]:
            pair.append(_dev_cube(f) if is_dev(f) else _open_dark(f, cfg.layout))
        fits = not is_dev(files[j])
        if is_dev(files[j]) != is_dev(files[j + 1]):
            raise TypeError(f"{which}: the exposures {j + 1} and {j + 2} are a file and a device cube: they are stored differently")
        if stack is None:
            nreads, ny, width = pair[0].shape
            nx = min(int(nside), width)
            try:
                check_frames(cfg.frames, nreads)
                check_geometry(ny, nx, cfg.nbin, nb)
            except ValueError as e:
                raise ValueError(f"correlation_run: {e}") from None
            stack = CorrStack(cfg.frames, ny, nx, cfg.nbin, nb=nb, ctx=ctx)
        print(which, "pair", j // 2 + 1, "of", len(files) // 2)
        sys.stdout.flush()
        stack.add_pair(pair[0], pair[1], fits_be16=fits)
    return stack


def run_ir_all(config_path, ctx=None, *, nside=pars.nside, nb=4, light=None, dark=None):
    """Write the summary of the configuration file ``config_path``; returns ``(summary path, config path)``.  ``nside``: the side
    of the detector, the columns of wider frames beyond it (the reference output) are left out (smaller frames: for tests).
    ``light``, ``dark``: lists of ``DevArray`` cubes (``frames_to_cube``) that stand in for the files of the configuration, read
    where they are."""
    with open(config_path) as f:
        cfg = parse_config(f.read())
    for key, value in cfg.ignored:
        print(f"{key}: {value} -- accepted, not acted on (CHAR: Basic level)")
    stacks = [_stack(cfg.light if light is None else list(light), cfg, "LIGHT", nside, nb, ctx),
              _stack(cfg.dark if dark is None else list(dark), cfg, "DARK", nside, nb, ctx)]
    if (stacks[0].ny, stacks[0].nx) != (stacks[1].ny, stacks[1].nx):
        raise ValueError(f"correlation_run: LIGHT frames are ({stacks[0].ny},{stacks[0].nx}), DARK frames ({stacks[1].ny},{stacks[1].nx})")
    table = solve_summary(stacks[0].table(), stacks[1].table(), cfg.frames, cfg.timeref)
    assert table.shape[1] == NCOL
    print("superpixels", cfg.nbin[0], cfg.nbin[1], "-->", np.count_nonzero(table[:, 2] > 0), "good")
    return write_outputs(cfg, table)


def gain_from_flats(configs, sca, outfile, ctx=None, *, nside=pars.nside, nb=4, ipc_dtype=np.float64):
    """The job's lines 48-71 in one call: ``run_ir_all`` on every configuration file of ``configs``, then ``make_gain_file.run`` on
    their summaries (listed in ``<outfile minus .asdf>_summaries.txt``).  Returns the paths of the gain and the ipc4d file."""
    summaries = [run_ir_all(c, ctx=ctx, nside=nside, nb=nb)[0] for c in configs]
    listing = (outfile[:-5] if outfile.endswith(".asdf") else outfile) + "_summaries.txt"
    with open(listing, "w") as f:
        f.write("".join(s + "\n" for s in summaries))
    with open(configs[0]) as f:
        cfg = parse_config(f.read())
    _, ny, width = _open_dark(cfg.light[0], cfg.layout).shape   # the frame the summaries were made of
    return make_gain_file.run(listing, sca, outfile, ipc_dtype=ipc_dtype, shape=(ny, min(int(nside), width)), ctx=ctx)


if __name__ == "__main__":
    run_ir_all(sys.argv[1])
