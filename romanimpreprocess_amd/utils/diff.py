"""Image differencing utility, for visualization -- the reference's ``utils/diff.py`` on the GPU: the difference of two groups
of a Level-1 cube as a float32 FITS image.  ``rip_view_plane_diff`` forms ``float32(data[group2]) - float32(data[group1])`` in
HBM (of a host cube only the two planes travel); the FITS data unit is encoded on the device and written by
``calio.write_fits``.

``python -m romanimpreprocess_amd.utils.diff <asdf in> <fits out> <group1> <group2>``
"""

import sys

import numpy as np

from .. import _native, calio
from ..devarray import DevArray, is_dev

USAGE = "Calling format: python diff.py <asdf in> <fits out> <group1> <group2>"


def group_difference(cube, group1, group2, ctx=None, out=None):
    """``cube[group2].astype(np.float32) - cube[group1]`` of a uint16 or float32 cube (ng, ny, nx), a numpy array or a
    ``DevArray``, as a float32 ``DevArray`` (ny, nx) in HBM (``out``: such an array, or a numpy array, to write into).  Negative
    groups count from the end, as numpy's; a group outside the cube raises ``IndexError``."""
    ctx = ctx or _native.default_context()
    if not is_dev(cube):
        cube = np.asarray(cube)
        cube = np.ascontiguousarray(cube if cube.dtype in (np.uint16, np.float32) else cube.astype(np.float32))
    if cube.ndim != 3 or cube.dtype not in (np.uint16, np.float32):
        raise ValueError(f"diff: the cube is {cube.dtype}{tuple(cube.shape)}, expected uint16 or float32 (ng, ny, nx)")
    ng, ny, nx = cube.shape
    groups = []
    for g in (int(group1), int(group2)):
        if not -ng <= g < ng:
            raise IndexError(f"index {g} is out of bounds for axis 0 with size {ng}")
        groups.append(g % ng)
    if out is None:
        import torch  # noqa: PLC0415

        out = DevArray(torch.empty((ny, nx), dtype=torch.float32, device=torch.device("cuda", ctx.device))).sync()
    if tuple(out.shape) != (ny, nx) or out.dtype != np.float32:
        raise ValueError(f"diff: out is {out.dtype}{tuple(out.shape)}, expected float32 {(ny, nx)}")
    ctx.call("rip_view_plane_diff", cube, _native.dtype_code(cube), _native.location_of(cube), ng, ny, nx, groups[0], groups[1], out,
             _native.location_of(out))
    return out


def diff(argv, ctx=None):
    """``argv``: [dummy, asdf in, fits out, group1, group2], as the reference's script"""
    if len(argv) < 5:
        print(USAGE)
        return
    with calio.open_tree(argv[1]) as f:
        data = f["roman"]["data"]
        g1, g2 = int(argv[3]), int(argv[4])
        ng = data.shape[0]
        if not (-ng <= g1 < ng and -ng <= g2 < ng):
            raise IndexError(f"groups {g1} and {g2} of a cube of {ng}")
        pair = np.stack([np.asarray(data[g1]), np.asarray(data[g2])])   # only the two planes are read and travel
    calio.write_fits(argv[2], [group_difference(pair, 0, 1, ctx=ctx)], ctx=ctx)


if __name__ == "__main__":
    diff(sys.argv)
