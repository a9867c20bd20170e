"""ctypes binding of the packed-statistics entry points of libsaihip.so (include/saihip_packed_stats.h): per-site allele
frequencies straight from packed2 blocks, the site half of fd / df / Danc / Dplus in the 2-bit layout.

They live in the same shared library as the entry points of ``_ffi`` (and their host part in the sanitizer
build of the host units), but in a header and a table of their own, with their own version number:
``load()`` / ``load_host()`` take the handle ``_ffi`` returns and declare the prototypes below on it.  A
library without them is an error, as everywhere in this package.
"""

from __future__ import annotations

import ctypes as C

from . import _ffi
from ._binding import extension

SAI_PACKED_STATS_ABI_VERSION = 1
SAI_PACKED_FREQ_POPS = 9  # ref, tgt, SAI_FUSED_SRC sources, outgroup

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names include/saihip_packed_stats.h declares
SIGNATURES = {
    "sai_packed_stats_abi_version": (C.c_int, []),
    "sai_packed2_site_freqs": (C.c_int, [_p, _i64, _i32, C.POINTER(_ffi.SaiPop), _p, _p]),
    "sai_packed2_site_freqs_host": (C.c_int, [_i64, _i32, C.POINTER(_ffi.SaiPop), _p, _i32]),
}

# entry points that never touch the GPU (packed_stats/packed2_freqs_host.cpp)
HOST_SYMBOLS = tuple(n for n in SIGNATURES if n != "sai_packed2_site_freqs")

load, load_host = extension("packed-stats", "saihip_packed_stats.h", "sai_packed_stats_abi_version", SAI_PACKED_STATS_ABI_VERSION, SIGNATURES, HOST_SYMBOLS,
                            built_from="packed_stats/packed2_freqs*")  # fmt: skip
