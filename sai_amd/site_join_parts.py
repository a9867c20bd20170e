"""One tiled population from several device blocks (DESIGN_INGEST.md, "Several source files"): with more than one source
file, the individuals of a source population such as NEA = {Altai, Vindija} lie in different int8 [record][sample]
blocks, each with its own row list of the common sites.  ``sai_tile_rows_from_parts``
(sai_amd/csrc/join/tile_parts.hip) re-tiles them in ONE launch, every part gathered by its own list, where stacking the
columns, making the stack contiguous and tiling it moves every genotype three times and needs an ``index_select`` per
block in front of it.

The two entry points are internal to the package: sai_amd/csrc/join/tile_parts.hip declares them itself, and this
module -- their only caller -- binds them, with a version number of their own.
"""

from __future__ import annotations

import ctypes as C

from . import _ffi
from ._binding import extension

SAI_TILE_PARTS_ABI_VERSION = 1
SAI_TILE_MAX_PARTS = 16

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64


class TilePart(C.Structure):
    """``sai_tile_part`` of sai_amd/csrc/join/tile_parts.hip."""

    _fields_ = [("src", _p), ("n_src_rows", _i64), ("row_stride", _i64), ("rows", _p), ("ind0", _i32), ("n_ind", _i32)]


# name -> (restype, argtypes): the names sai_amd/csrc/join/tile_parts.hip declares
SIGNATURES = {
    "sai_tile_parts_abi_version": (C.c_int, []),
    "sai_tile_rows_from_parts": (C.c_int, [_p, _i32, C.POINTER(TilePart), _i64, _i32, _p, _p, _p]),
}
HOST_SYMBOLS = ("sai_tile_parts_abi_version",)

load, load_host = extension("tile parts", "sai_amd/csrc/join/tile_parts.hip", "sai_tile_parts_abi_version", SAI_TILE_PARTS_ABI_VERSION,
                            SIGNATURES, HOST_SYMBOLS, built_from="join")  # fmt: skip


def tile_parts(tiler, parts, n_rows=None):
    """``TiledPop`` of one population whose individuals come from ``parts``, in the order given: a sequence of ``(block,
    col0, n_ind, rows)`` -- the columns [col0, col0 + n_ind) of ``block`` (a 2-D int8 device tensor whose rows are
    contiguous) at the rows ``rows`` (an int32 device tensor, in any order, repeats allowed; None: every row of the
    block).  ``n_rows`` is the number of sites: by default the length of the row lists, which must agree, or the rows
    of the blocks where no part has a list.  One launch on the current stream; its count of row indices outside their
    block joins those of ``tiler`` (a ``site_join_device.RowTiler``), whose ``check`` reads them."""
    import torch

    from .engine import TiledPop

    eng, lib = tiler.eng, load()
    parts = list(parts)
    if not 1 <= len(parts) <= SAI_TILE_MAX_PARTS:
        raise ValueError(f"a population is tiled from 1 to {SAI_TILE_MAX_PARTS} parts, not {len(parts)}")
    sizes = {int(rows.numel()) if rows is not None else int(block.shape[0]) for block, _, _, rows in parts}
    if n_rows is None:
        if len(sizes) != 1:
            raise ValueError(f"the parts name different numbers of sites: {sorted(sizes)}")
        n_rows = sizes.pop()
    n_rows = int(n_rows)
    table, ind0, keep = (TilePart * len(parts))(), 0, []
    for k, (block, col0, n_ind, rows) in enumerate(parts):
        if block.dtype != torch.int8 or block.dim() != 2 or (block.shape[1] > 1 and block.stride(1) != 1):
            raise TypeError("the block must be a 2-D int8 device tensor with contiguous rows")
        n_src_rows, width = int(block.shape[0]), int(block.shape[1])
        col0, n_ind = int(col0), int(n_ind)
        if col0 < 0 or n_ind < 0 or col0 + n_ind > width:
            raise ValueError(f"columns {col0} .. {col0 + n_ind} are not inside a block of {width}")
        if rows is not None:
            if rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous():
                raise TypeError("rows must be a contiguous 1-D int32 device tensor")
            if n_rows > int(rows.numel()):
                raise ValueError("n_rows exceeds the row list")
        stride = int(block.stride(0)) if n_src_rows > 1 else max(width, 1)
        table[k] = TilePart(block.data_ptr() + col0 if block.numel() else None, n_src_rows, stride,
                            rows.data_ptr() if rows is not None and rows.numel() else None, ind0, n_ind)  # fmt: skip
        if rows is not None and not rows.numel() and n_rows == 0:  # an empty list is not the identity: no site, nothing is read
            table[k].n_src_rows = 0
        keep.append((block, rows))
        ind0 += n_ind
    dst = eng._empty((max(int(eng.lib.sai_tiled_bytes(n_rows, ind0)), 0),), torch.int8)
    n_bad = eng._empty((1,), torch.int32)
    _ffi.check(lib.sai_tile_rows_from_parts(eng.ctx, len(parts), table, n_rows, ind0, eng._ptr(dst), C.c_void_p(n_bad.data_ptr()),
                                            eng._stream()), lib)  # fmt: skip
    tiler._bad.append(n_bad)
    return TiledPop(dst, n_rows, ind0)
