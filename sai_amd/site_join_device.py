"""The device side of two joined inputs (DESIGN_INGEST.md, "Sources from a file of their own"): after
``site_join.join_host`` has named the rows of the common sites, every population of both inputs is re-tiled from those
rows of its reader's int8 [record][sample] block in ONE pass -- ``sai_tile_rows_from_site_major``
(sai_amd/csrc/join/tile_rows.hip), a row gather fused into the re-tiling, where ``index_select`` followed by
``sai_tile_from_site_major`` would move every genotype twice and hold a third copy of the block.

The two entry points are internal to the package: sai_amd/csrc/join/tile_rows.hip declares them itself, and this
module -- their only caller -- binds them, with a version number of their own.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._binding import extension

SAI_JOIN_DEVICE_ABI_VERSION = 1

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names sai_amd/csrc/join/tile_rows.hip declares
SIGNATURES = {
    "sai_join_device_abi_version": (C.c_int, []),
    "sai_tile_rows_from_site_major": (C.c_int, [_p, _p, _i64, _i32, _i64, _p, _i64, _p, _p, _p]),
}
HOST_SYMBOLS = ("sai_join_device_abi_version",)

load, load_host = extension("device join", "sai_amd/csrc/join/tile_rows.hip", "sai_join_device_abi_version", SAI_JOIN_DEVICE_ABI_VERSION,
                            SIGNATURES, HOST_SYMBOLS, built_from="join")  # fmt: skip


def upload_rows(eng, rows):
    """The int32 device copy of a host row list; None (the identity) stays None."""
    import torch

    if rows is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(eng.device)


class RowTiler:
    """Tiled blocks of selected rows of device int8 [record][sample] blocks.  Every ``tile`` enqueues one launch on the
    current stream and keeps the launch's count of row indices outside its block; ``check`` reads all the counts with
    one synchronisation and raises when one is not zero -- a row list that does not belong to the block it was used on,
    which is an error of this package, not of the input."""

    def __init__(self, eng):
        self.eng, self.lib, self._bad = eng, load(), []

    def tile(self, block, col0: int, n_ind: int, rows=None, n_rows=None):
        """``TiledPop`` of the columns [col0, col0 + n_ind) of ``block`` (a 2-D int8 device tensor whose rows are
        contiguous) at the rows ``rows`` (an int32 device tensor, in any order, repeats allowed); ``rows=None``: every
        row, byte for byte what ``Engine.tile_columns`` gives."""
        import torch

        from .engine import TiledPop

        if block.dtype != torch.int8 or block.dim() != 2 or (block.shape[1] > 1 and block.stride(1) != 1):
            raise TypeError("the block must be a 2-D int8 device tensor with contiguous rows")
        n_src_rows, width = int(block.shape[0]), int(block.shape[1])
        col0, n_ind = int(col0), int(n_ind)
        if col0 < 0 or n_ind < 0 or col0 + n_ind > width:
            raise ValueError(f"columns {col0} .. {col0 + n_ind} are not inside a block of {width}")
        if rows is not None and (rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous()):
            raise TypeError("rows must be a contiguous 1-D int32 device tensor")
        n_rows = (n_src_rows if rows is None else int(rows.numel())) if n_rows is None else int(n_rows)
        if rows is not None and n_rows > int(rows.numel()):
            raise ValueError("n_rows exceeds the row list")
        eng = self.eng
        stride = int(block.stride(0)) if n_src_rows > 1 else max(width, 1)
        dst = eng._empty((max(int(eng.lib.sai_tiled_bytes(n_rows, n_ind)), 0),), torch.int8)
        n_bad = eng._empty((1,), torch.int32)
        src = C.c_void_p(block.data_ptr() + col0) if block.numel() else C.c_void_p(0)
        _ffi.check(self.lib.sai_tile_rows_from_site_major(eng.ctx, src, n_src_rows, n_ind, stride, eng._ptr(rows) if rows is not None else None,
                                                          n_rows, eng._ptr(dst), C.c_void_p(n_bad.data_ptr()), eng._stream()), self.lib)  # fmt: skip
        self._bad.append(n_bad)
        return TiledPop(dst, n_rows, n_ind)

    def check(self) -> None:
        import torch

        counts, self._bad = self._bad, []
        if counts:
            bad = torch.cat(counts).cpu().numpy()
            if bad.any():
                raise RuntimeError(f"sai_tile_rows_from_site_major met {int(bad.sum())} row indices outside their block "
                                   f"(launch {int(np.flatnonzero(bad)[0])} of {bad.size}): the row list of a join was used on another block")  # fmt: skip
