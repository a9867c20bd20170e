"""ctypes binding of the join entry points of libsaihip.so (include/saihip_join.h): the common rows of two ascending
position lists -- what the host readers run between reading a panel and a source file of its own
(``sai_amd.site_join``).  Host code only in this version.

They live in the same shared library as the entry points of ``_ffi`` (and in the sanitizer build of the host units),
but in a header and a table of their own, with their own version number: ``load()`` / ``load_host()`` take the handle
``_ffi`` returns and declare the prototypes below on it.  A library without them is an error, as everywhere in this
package.
"""

from __future__ import annotations

import ctypes as C

from ._binding import extension

SAI_JOIN_ABI_VERSION = 1
SAI_JOIN_INFO_WORDS = 4  # int64 words: n_common, first bad index of a, of b, rows_a is the identity

_p, _i64 = C.c_void_p, C.c_int64

# name -> (restype, argtypes): the names include/saihip_join.h declares
SIGNATURES = {
    "sai_join_abi_version": (C.c_int, []),
    "sai_site_join_host": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _p]),
}

# entry points that never touch the GPU (join/site_join_host.cpp): all of them
HOST_SYMBOLS = tuple(SIGNATURES)

load, load_host = extension("join", "saihip_join.h", "sai_join_abi_version", SAI_JOIN_ABI_VERSION, SIGNATURES, HOST_SYMBOLS,
                            built_from="join/site_join_host.cpp")  # fmt: skip
