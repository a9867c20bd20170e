"""DD for source populations of any size: one read of ref and tgt (sai_amd/csrc/dd_table/).

DD's per-site term of a source value ``v`` against a population, the sum over its individuals ``g`` of ``|v - g|``,
depends on ``v`` alone, and a sample read at ploidy 1 or 2 holds one of seven values in a block: -p .. p as read, up to
2p after an ancestral flip (p - d) -- ``DD_VALUES``.  ``site_absdiff_table`` streams a population once and writes the
term of every value per site (28 bytes per site); ``window_dd_table`` picks, per source individual and site, the entry
the source's byte names and forms DD with ``Engine.window_dd``'s arithmetic.  ``combination_dd`` is the route
``FeaturePreprocessor.score_windows`` takes for combinations with more source individuals than ride along the site
pass; ``Engine.site_absdiff`` + ``Engine.window_dd`` stay for sources of higher ploidy and for any population that
turns out to hold a byte outside the list.

The entry points are a group internal to the package: stated in csrc/dd_table/dd_table_host.cpp, bound HERE with
``_binding.extension`` (``load`` / ``load_host``: a library without them, or of another version, is refused), with a version
number of their own.  (They are no family with a header under include/, and this module lives beside ``engine.py`` and
not in it: the stored figures under profiles/ name the digest of the sources they were measured on --
``bench.source_digest``: saihip.h and ``engine.py`` among them -- and this route changes nothing those figures depend on.)
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Sequence

import numpy as np

from . import _ffi
from ._binding import extension

SAI_DD_TABLE_ABI_VERSION = 1
SAI_DD_TABLE_VALUES = 8  # values of one table at most

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
_pop_p, _values_p = C.POINTER(_ffi.SaiPop), C.POINTER(C.c_int8)

# name -> (restype, argtypes): the names csrc/dd_table/dd_table_host.cpp states
SIGNATURES = {
    "sai_dd_table_abi_version": (C.c_int, []),
    "sai_site_absdiff_table": (C.c_int, [_p, _i64, _pop_p, _i32, _values_p, _p, _p]),
    "sai_window_dd_table": (C.c_int, [_p, _i64, _pop_p, _i32, _values_p, _p, _i32, _p, _i32, _i32, _p, _p, _p, _p, _p, _p]),
    "sai_site_absdiff_table_host": (C.c_int, [_i64, _pop_p, _i32, _values_p, _p]),
    "sai_window_dd_table_host": (C.c_int, [_i64, _pop_p, _i32, _values_p, _p, _i32, _p, _i32, _i32, _p, _p, _p, _p, _p]),
}

# entry points that never touch the GPU (dd_table/dd_table_host.cpp)
HOST_SYMBOLS = ("sai_dd_table_abi_version", "sai_site_absdiff_table_host", "sai_window_dd_table_host")

load, load_host = extension("DD-table", "sai_amd/csrc/dd_table/dd_table_host.cpp", "sai_dd_table_abi_version", SAI_DD_TABLE_ABI_VERSION, SIGNATURES,
                            HOST_SYMBOLS, built_from="dd_table")  # fmt: skip

DD_VALUES = (-2, -1, 0, 1, 2, 3, 4)
MIN_ROWS_DEFAULT = 5  # source individuals of a combination from which the table route is taken: one more than ride along

# how often each step ran in this process (tests read and reset it)
CALLS = {"site_absdiff_table": 0, "window_dd_table": 0, "old_route": 0}


def reset_calls() -> None:
    for k in CALLS:
        CALLS[k] = 0


def _values_array(values):
    values = [int(v) for v in values]
    if not 1 <= len(values) <= SAI_DD_TABLE_VALUES:
        raise ValueError(f"a table holds 1..{SAI_DD_TABLE_VALUES} values")
    if any(not -128 <= v <= 127 for v in values):
        raise ValueError("values must be int8")
    return (C.c_int8 * len(values))(*values), len(values)


def _pop(t):
    p = _ffi.SaiPop()
    p.tiles, p.n_ind, p.ploidy = (t.tiles.data_ptr() if t.tiles.numel() else 0), t.n_ind, 1
    return p


def site_absdiff_table(eng, pop, values=DD_VALUES):
    """int32 [len(values)][n_sites] (the bits are uint32): per site and value v, the sum over ``pop``'s individuals of
    |v - g|."""
    import torch

    lib = load()
    arr, n = _values_array(values)
    table = torch.empty((n, pop.n_sites), dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_site_absdiff_table(eng.ctx, pop.n_sites, C.byref(_pop(pop)), n, arr, eng._ptr(table), eng._stream()), lib)
    CALLS["site_absdiff_table"] += 1
    return table


def window_dd_table(eng, src, table_ref, n_ref: int, table_tgt, n_tgt: int, lo, hi, values=DD_VALUES):
    """(dd f64 [n_windows], n_unlisted int32 [1]) on the device: DD of one source population from the tables of ref and
    tgt.  ``dd`` is to be discarded when ``n_unlisted`` is not zero: some byte of ``src`` is not in ``values``."""
    import torch

    lib = load()
    arr, n = _values_array(values)
    if tuple(table_ref.shape) != (n, src.n_sites) or tuple(table_tgt.shape) != (n, src.n_sites):
        raise ValueError("the tables must be [len(values)][n_sites] over the source's sites")
    if not (table_ref.is_contiguous() and table_tgt.is_contiguous() and lo.is_contiguous() and hi.is_contiguous()):
        raise ValueError("tables and window bounds must be contiguous")
    n_w = int(lo.numel())
    scratch = torch.empty((n_w, src.n_ind), dtype=torch.float64, device=eng.device)
    dd = torch.empty((n_w,), dtype=torch.float64, device=eng.device)
    n_unlisted = torch.empty((1,), dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_window_dd_table(eng.ctx, src.n_sites, C.byref(_pop(src)), n, arr, eng._ptr(table_ref), int(n_ref), eng._ptr(table_tgt),
                                       int(n_tgt), n_w, eng._ptr(lo), eng._ptr(hi), eng._ptr(scratch), eng._ptr(dd), eng._ptr(n_unlisted),
                                       eng._stream()), lib)  # fmt: skip
    CALLS["window_dd_table"] += 1
    return dd, n_unlisted


def table_route_admitted(src_ploidies: Sequence[int], n_src_rows: int, environ=None) -> bool:
    """The table route serves a combination whose source populations all have ploidy 1 or 2 (their bytes are then among
    ``DD_VALUES``) and which has at least ``SAI_AMD_DD_TABLE_MIN_ROWS`` source individuals (default 5), unless
    ``SAI_AMD_DD_TABLE=0``."""
    environ = os.environ if environ is None else environ
    if environ.get("SAI_AMD_DD_TABLE", "") == "0":
        return False
    raw = environ.get("SAI_AMD_DD_TABLE_MIN_ROWS", "")
    try:
        min_rows = int(raw) if raw != "" else MIN_ROWS_DEFAULT
    except ValueError:
        raise ValueError(f"SAI_AMD_DD_TABLE_MIN_ROWS must be an integer, not {raw!r}") from None
    ploidies = list(src_ploidies)
    return bool(ploidies) and all(int(p) in (1, 2) for p in ploidies) and n_src_rows >= min_rows


class TablePair:
    """The tables of one (ref, tgt) pair of blocks, kept across the source combinations of a call and dropped when the
    pair changes: 56 bytes per site."""

    def __init__(self):
        self._pair = None
        self._tables = None

    def tables(self, eng, ref_t, tgt_t):
        if self._pair is None or self._pair[0] is not ref_t or self._pair[1] is not tgt_t:
            self._pair = self._tables = None  # the old pair's tables go before the new ones are allocated
            self._tables = (site_absdiff_table(eng, ref_t), site_absdiff_table(eng, tgt_t))
            self._pair = (ref_t, tgt_t)
        return self._tables


def old_route_dd(eng, ref_t, tgt_t, src_t, lo, hi):
    """DD of one source population by two streaming passes per pair of its individuals (f64 [n_windows], device)."""
    CALLS["old_route"] += 1
    return eng.window_dd(eng.site_absdiff(ref_t, src_t), ref_t.n_ind, eng.site_absdiff(tgt_t, src_t), tgt_t.n_ind, lo, hi)


def combination_dd(eng, pair: TablePair, ref_t, tgt_t, srcs, lo, hi) -> np.ndarray:
    """f64 [n_windows][len(srcs)]: DD of every source population of a combination through the tables of ref and tgt --
    one window kernel per population, ONE synchronisation for all their counters of unlisted bytes, and the old route
    for a population whose counter is not zero."""
    import torch

    table_ref, table_tgt = pair.tables(eng, ref_t, tgt_t)
    outs = [window_dd_table(eng, s, table_ref, ref_t.n_ind, table_tgt, tgt_t.n_ind, lo, hi) for s in srcs]
    unlisted = torch.cat([n for _, n in outs]).cpu().tolist()
    cols = [(old_route_dd(eng, ref_t, tgt_t, s, lo, hi) if n else dd).cpu().numpy() for s, (dd, _), n in zip(srcs, outs, unlisted)]
    return np.stack(cols, axis=1)
