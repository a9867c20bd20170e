"""Seeded inputs and numpy statements for the DD table entry points (sai_amd/csrc/dd_table/), shared by
test_dd_table_cpu.py (the host twins, no GPU) and test_dd_table_device.py (the kernels).

The table is ``np.abs(values[:, None, None] - g[None]).sum(axis=1)`` for g = int64 [individuals][sites]; the window half
reuses tests/sum_order_cases.py (``dd_expected``, ``WINDOWS``, ``clamp``) on the per-individual terms the table stands
for: ad[s][i] = table[index of src[s][i] in values][i]."""

from __future__ import annotations

from functools import lru_cache
from pathlib import Path

import numpy as np

import sum_order_cases as S
from capacity_cases import parse_constants

KERNELS = Path(__file__).resolve().parent.parent / "sai_amd" / "csrc" / "dd_table" / "dd_table.hip"

DD_VALUES = (-2, -1, 0, 1, 2, 3, 4)
N_IND = (0, 1, 3, 16, 17, 64, 65, 250)
N_SITES = (1, 63, 64, 65, 130)
VALUE_LISTS = ((3,), DD_VALUES, (-128, -2, -1, 0, 1, 2, 64, 127))  # 1, 7 and 8 entries; both ends of int8
KINDS = ("all", "listed")  # genotypes from all of -128 .. 127, or from DD_VALUES only


@lru_cache(maxsize=None)
def constants() -> dict:
    found = parse_constants(KERNELS.read_text())
    for n in ("kTableChunkGroups", "kTableGroupIters", "kDdStageWords"):
        if n not in found:
            raise KeyError(f"dd_table.hip no longer defines constexpr int {n}")
    return found


def widen_rows() -> int:
    """Individuals of a population after which the streaming kernel closes its first chunk of 16-bit fields: groups per
    chunk x iterations per group x 16 rows per iteration."""
    c = constants()
    return c["kTableChunkGroups"] * c["kTableGroupIters"] * 16


def stage_sites(n_values: int) -> int:
    """dd_stage_sites of dd_table.hip: the longest window sai_window_dd_table stages in LDS."""
    return (constants()["kDdStageWords"] // (2 * n_values)) & ~63


def genotypes(n_sites: int, n_ind: int, kind: str, seed=0) -> np.ndarray:
    """int8 [sites][individuals]."""
    rng = np.random.default_rng([21, n_sites, n_ind, KINDS.index(kind), seed])
    if kind == "all":
        g = rng.integers(-128, 128, size=(n_sites, n_ind)).astype(np.int8)
        if g.size >= 2:
            g.flat[0], g.flat[-1] = -128, 127
        return g
    return rng.choice(np.array(DD_VALUES, dtype=np.int8), size=(n_sites, n_ind))


def tile_numpy(g: np.ndarray) -> np.ndarray:
    """The int8 tiled layout of saihip.h: byte(tile, individual, site-in-tile) = tiles[(tile * n_ind + individual) * 64 +
    site-in-tile], the last tile padded with zero bytes."""
    n_sites, n_ind = g.shape
    n_tiles = -(-n_sites // 64)
    padded = np.zeros((n_tiles * 64, n_ind), dtype=np.int8)
    padded[:n_sites] = g
    return np.ascontiguousarray(padded.reshape(n_tiles, 64, n_ind).transpose(0, 2, 1)).reshape(-1)


def table_numpy(values, g: np.ndarray) -> np.ndarray:
    """int64 [len(values)][sites]: the header's statement."""
    v = np.asarray(values, dtype=np.int64)
    g64 = np.ascontiguousarray(g.T).astype(np.int64)  # [individuals][sites]
    return np.abs(v[:, None, None] - g64[None]).sum(axis=1)


def terms_of(table: np.ndarray, values, src: np.ndarray):
    """(ad int64 [individuals of src][sites], unlisted): the entry each source byte names; a byte outside ``values``
    adds nothing and is counted."""
    values = list(values)
    index = np.full(256, -1, dtype=np.int64)
    index[np.asarray(values, dtype=np.int8).view(np.uint8)] = np.arange(len(values))
    k = index[np.ascontiguousarray(src.T).view(np.uint8)]  # [individuals][sites]
    sites = np.arange(src.shape[0])[None, :]
    ad = np.where(k >= 0, table[np.maximum(k, 0), sites], 0)
    return ad, int((k < 0).sum())


# ---- the window half: sum_order_cases' block of 256 sites, 7 reference and 3 target individuals ----

N_SRC = tuple(sorted({1, 2, 5, 8, 9, 129, *S.SIZES}))
BLOCK_SITES = S.DD_SITES


@lru_cache(maxsize=None)
def window_block(n_sites: int = BLOCK_SITES, kind: str = "listed"):
    """(ref int8 [sites][7], tgt int8 [sites][3], table_ref, table_tgt int64 [7][sites]) over DD_VALUES -- computed once,
    never changed."""
    ref, tgt = genotypes(n_sites, S.N_REF, kind, seed=1), genotypes(n_sites, S.N_TGT, kind, seed=2)
    return ref, tgt, table_numpy(DD_VALUES, ref), table_numpy(DD_VALUES, tgt)


@lru_cache(maxsize=None)
def window_source(n_src: int, n_sites: int = BLOCK_SITES) -> np.ndarray:
    """int8 [sites][n_src] from DD_VALUES."""
    return genotypes(n_sites, n_src, "listed", seed=3)


def window_expected(n_src: int, windows, n_sites: int = BLOCK_SITES):
    """(d f64 [n_windows][n_src], dd f64 [n_windows], unlisted) of ``window_source(n_src)`` against ``window_block``."""
    _, _, table_ref, table_tgt = window_block(n_sites)
    src = window_source(n_src, n_sites)
    ad_ref, u1 = terms_of(table_ref, DD_VALUES, src)
    ad_tgt, _ = terms_of(table_tgt, DD_VALUES, src)
    d, dd = S.dd_expected(ad_ref, ad_tgt, windows)
    return d, dd, u1


def long_block_sites() -> int:
    """A block that holds a window one site past the staging capacity of seven values, and some more."""
    return stage_sites(len(DD_VALUES)) + 70


def capacity_windows():
    """One window at the staging capacity, one a site past it, one over the whole block (in place), and neighbours."""
    cap, n = stage_sites(len(DD_VALUES)), long_block_sites()
    return ((3, 3 + cap), (3, 4 + cap), (0, n), (n - cap, n), (n - cap - 1, n), (1, cap), (-5, n + 9), (40, 40), (90, 10))
