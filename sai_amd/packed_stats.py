"""fd, df, Danc and Dplus over populations that are held in the 2-bit layout (``PackedPop``).

The window half of the ABBA-BABA family -- ``Engine.window_fourpop`` -- takes f64 frequencies ``[P][n_sites]`` and does
not care which layout they came from.  The site half for packed blocks is ``packed_site_freqs``: one kernel
(include/saihip_packed_stats.h, ``sai_packed2_site_freqs``) that counts the three codes of a site and divides, for up
to nine populations (ref, tgt, ``SAI_FUSED_SRC`` sources, outgroup) -- the doubles of ``Engine.site_pass_packed2(counts)``
+ ``Engine.site_freqs`` bit for bit, without the counts tensor in between.  ``packed_fourpop_windows`` is the packed
twin of ``Engine.fourpop_windows``.

(It lives beside ``engine.py`` and not in it: the stored figures under profiles/ name the digest of the sources
they were measured on -- ``bench.source_digest``: ``engine.py`` among them -- and this route changes nothing those
figures depend on.)
"""

from __future__ import annotations

import ctypes as C
from typing import Sequence

from . import _ffi, _ffi_packed_stats
from .engine import PackedPop


def packed_site_freqs(eng, pops: Sequence[PackedPop], ploidies: Sequence[int]):
    """f64 frequency per population and site ([P][n_sites], NaN where nothing is called) of 1 ..
    ``SAI_PACKED_FREQ_POPS`` packed2 blocks over the same sites."""
    import torch

    lib = _ffi_packed_stats.load()
    if len(pops) != len(ploidies):
        raise ValueError("one ploidy per population")
    if not pops:
        raise ValueError("no population")
    n_sites = pops[0].n_sites
    if any(p.n_sites != n_sites for p in pops):
        raise ValueError("all populations of one call must cover the same sites")
    arr = (_ffi.SaiPop * len(pops))()
    for i, p in enumerate(pops):
        arr[i].tiles = p.data.data_ptr() if p.data.numel() else 0
        arr[i].n_ind = p.n_ind
        arr[i].ploidy = int(ploidies[i])
    freqs = torch.empty((len(pops), n_sites), dtype=torch.float64, device=eng.device)
    _ffi.check(lib.sai_packed2_site_freqs(eng.ctx, n_sites, len(pops), arr, C.c_void_p(freqs.data_ptr() if freqs.numel() else 0),
                                          eng._stream()), lib)  # fmt: skip
    return freqs


def packed_fourpop_windows(eng, pops: Sequence[PackedPop], ploidies: Sequence[int], n_src: int, has_outgroup: bool, lo, hi):
    """fd, df, Danc, Dplus per (window, source) for ANY number of sources, f64 [n_windows][n_src][4]: ``pops`` =
    packed2 blocks in the order ref, tgt, sources..., (outgroup).  Every source is a statistic of its own
    (fd_statistic.py:63-88), so the sources go ``SAI_FUSED_SRC`` at a time as [ref, tgt, sources of the group,
    (outgroup)] through ``packed_site_freqs`` and ``Engine.window_fourpop``, as ``Engine.fourpop_windows`` sends
    counts through ``site_freqs``."""
    import torch

    if len(pops) != 2 + n_src + (1 if has_outgroup else 0):
        raise ValueError("pops must be ref, tgt, the sources and, with has_outgroup, the outgroup")
    parts = []
    tail = [2 + n_src] if has_outgroup else []
    for s0 in range(0, n_src, _ffi.SAI_FUSED_SRC):
        s1 = min(s0 + _ffi.SAI_FUSED_SRC, n_src)
        rows = [0, 1, *range(2 + s0, 2 + s1), *tail]
        freqs = packed_site_freqs(eng, [pops[r] for r in rows], [ploidies[r] for r in rows])
        parts.append(eng.window_fourpop(freqs, s1 - s0, has_outgroup, lo, hi))
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
