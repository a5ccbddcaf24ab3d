"""Grown pixel masks on the GPU -- same call surface as the reference's ``utils/maskhandling.py`` (``CombinedMask``,
``PixelMask1``).  ``build`` runs ``rip_stage_build_mask`` (bit-exact with the reference's per-bit convolutions);
``convert_file`` writes the mask file of an L2 file, the FITS form encoded on the device from the mask in HBM."""

import numpy as np

from .. import _native, calio
from ..devarray import DevArray, is_dev, to_device
from ..dqflags import pixel


class CombinedMask:
    """``maskdict``: flag name (or bit number) -> growth (1 copy, 5 plus-shaped, 9 3x3, 25 5x5), as
    ``maskhandling.py:38-58``."""

    def __init__(self, maskdict):
        self.array = np.zeros(32, dtype=np.uint8)
        for key, grow in maskdict.items():
            if isinstance(key, str):
                bit = int(getattr(pixel, key.upper())).bit_length() - 1
            else:
                bit = int(key)
            self.array[bit] = int(grow)

    def build(self, dq, ctx=None):
        """Boolean mask (True = masked) from a 2-D uint32 dq array (``maskhandling.py:82-117``)."""
        ctx = ctx or _native.default_context()
        dq = np.ascontiguousarray(dq, dtype=np.uint32)
        ny, nx = dq.shape
        out = np.empty((ny, nx), np.uint8)
        ctx.call("rip_stage_build_mask", dq, ny, nx, self.array, out)
        return out.astype(bool)

    def build_device(self, dq, ctx=None):
        """``build`` with the result left in HBM: a uint8 ``DevArray`` of 0 / 1.  ``dq`` (2-D uint32): a numpy array, which is
        uploaded, or a ``DevArray``, used where it is."""
        import torch

        ctx = ctx or _native.default_context()
        if not (is_dev(dq) and dq.dtype == np.uint32):
            dq = to_device(np.ascontiguousarray(dq, dtype=np.uint32), ctx.device)
        ny, nx = dq.shape
        mask = DevArray(torch.empty((ny, nx), dtype=torch.uint8, device=torch.device("cuda", ctx.device))).sync()
        ctx.call("rip_stage_build_mask", dq, ny, nx, self.array, mask)
        return mask

    def convert_file(self, file_in, file_mask, ctx=None):
        """Make a mask file from an L2 file (``maskhandling.py:119-149``).  ``file_mask`` ending in ``.asdf``: ``{"mask": boolean
        array}``; in ``.fits``: the image with -1000 in the masked pixels as float32 (primary HDU, for display) and the mask as
        int8 0 / 1 (extension ``MASK``); any other ending writes nothing.  ``dq`` is uploaded once; for the FITS file the mask
        stays in HBM and is handed to the encoder of the data units (``calio.write_fits``), it does not come to the host."""
        kind = file_mask[-5:]
        if kind not in (".asdf", ".fits"):
            return
        ctx = ctx or _native.default_context()
        with calio.open_tree(file_in) as f_in:
            dq = np.asarray(f_in["roman"]["dq"])
            data = np.ascontiguousarray(f_in["roman"]["data"], dtype=np.float32) if kind == ".fits" else None
        locmask = self.build_device(dq, ctx=ctx)
        if kind == ".asdf":
            calio.write_asdf(file_mask, {"mask": locmask.numpy().astype(bool)})
            return
        calio.write_fits(file_mask, [{"data": to_device(data, ctx.device), "mask": locmask, "mask_sense": 1, "fill": -1000.0},
                                     {"data": DevArray(locmask.t, np.int8), "extname": "MASK"}], ctx=ctx)


# the reference's standard choice (maskhandling.py:152-180)
PixelMask1 = CombinedMask({
    "DO_NOT_USE": 1, "JUMP_DET": 5, "DROPOUT": 25, "GW_AFFECTED_DATA": 1, "PERSISTENCE": 1, "AD_FLOOR": 5,
    "UNRELIABLE_ERROR": 1, "NON_SCIENCE": 1, "DEAD": 9, "HOT": 9, "WARM": 1, "LOW_QE": 9, "TELEGRAPH": 1,
    "NO_FLAT_FIELD": 9, "NO_GAIN_VALUE": 9, "NO_LIN_CORR": 9, "NO_SAT_CHECK": 9, "UNRELIABLE_BIAS": 1,
    "UNRELIABLE_DARK": 9, "UNRELIABLE_SLOPE": 9, "UNRELIABLE_FLAT": 9, "UNRELIABLE_RESET": 9, "OTHER_BAD_PIXEL": 9,
})
