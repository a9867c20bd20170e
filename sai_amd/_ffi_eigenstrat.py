"""ctypes binding of the EIGENSOFT fileset entry points of libsaihip.so (include/saihip_eigenstrat.h).

As ``_ffi_plink``: the entry points live in the same shared library as those of ``_ffi`` (and their host part
in the sanitizer build of the host units), in a header and a table of their own, with their own version
number.  ``load()`` / ``load_host()`` take the handle ``_ffi`` returns and declare the prototypes below on it.
A library without them is an error, as everywhere in this package.
"""

from __future__ import annotations

import ctypes as C

from ._binding import extension

SAI_EIGENSTRAT_ABI_VERSION = 1
SAI_EIGENSTRAT_STATUS_BAD_INDEX = 0x7FFFFFFF
SAI_EIGENSTRAT_STATUS_BAD_CHAR = 0x7FFFFFFE
TEXT, PACKED, TRANSPOSED = 1, 2, 3

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names include/saihip_eigenstrat.h declares
SIGNATURES = {
    "sai_eigenstrat_abi_version": (C.c_int, []),
    "sai_eigenstrat_scan": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(_i64), C.POINTER(_i64)]),
    "sai_eigenstrat_open": (
        C.c_int,
        [C.c_char_p, C.c_char_p, _i64, _i64, _i32, C.POINTER(C.c_char_p), C.POINTER(_i32), C.c_char_p, _i32, C.POINTER(_p)],
    ),
    "sai_eigenstrat_index_info": (C.c_int, [_p] + [C.POINTER(_i64)] * 10),
    "sai_eigenstrat_index_copy": (C.c_int, [_p, _p, _p, _p, _p]),
    "sai_eigenstrat_index_close": (C.c_int, [_p]),
    "sai_eigenstrat_decode_host": (C.c_int, [_i32, _p, _i64, _i64, _i32, _i64, _p, _p, _i32, _i32, _p, _p, _p, _p, _i32]),
    "sai_eigenstrat_decode": (C.c_int, [_p, _i32, _p, _i64, _i64, _i64, _p, _p, _i32, _i32, _p, _i32, _p, _i32, _p, _i64, _p, _p]),
    "sai_eigenstrat_decode_transposed": (C.c_int, [_p, _p, _i32, _i64, _i32, _i64, _i64, _p, _p, _i32, _p, _p, _p, _i64, _p, _p]),
}

# entry points that never touch the GPU (eigenstrat_index.cpp)
HOST_SYMBOLS = tuple(n for n in SIGNATURES if n not in ("sai_eigenstrat_decode", "sai_eigenstrat_decode_transposed"))

load, load_host = extension("EIGENSTRAT", "saihip_eigenstrat.h", "sai_eigenstrat_abi_version", SAI_EIGENSTRAT_ABI_VERSION, SIGNATURES, HOST_SYMBOLS,
                            built_from="eigenstrat")  # fmt: skip
