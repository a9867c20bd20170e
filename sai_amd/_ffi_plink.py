"""ctypes binding of the PLINK 1 fileset entry points of libsaihip.so (include/saihip_plink.h).

They live in the same shared library as the entry points of ``_ffi`` (and their host part in the
sanitizer build of the host units), but in a header and a table of their own, with their own version
number: ``load()`` / ``load_host()`` take the handle ``_ffi`` returns and declare the prototypes below
on it.  A library without them is an error, as everywhere in this package.
"""

from __future__ import annotations

import ctypes as C

from ._binding import extension

SAI_PLINK_ABI_VERSION = 1
SAI_PLINK_STATUS_BAD_INDEX = 0x7FFFFFFF

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names include/saihip_plink.h declares
SIGNATURES = {
    "sai_plink_abi_version": (C.c_int, []),
    "sai_plink_scan": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(_i64), C.POINTER(_i64)]),
    "sai_plink_open": (
        C.c_int,
        [C.c_char_p, C.c_char_p, _i64, _i64, _i32, C.POINTER(C.c_char_p), C.POINTER(_i32), C.c_char_p, _i32, C.POINTER(_p)],
    ),
    "sai_plink_index_info": (C.c_int, [_p] + [C.POINTER(_i64)] * 8),
    "sai_plink_index_copy": (C.c_int, [_p, _p, _p, _p, _p]),
    "sai_plink_index_close": (C.c_int, [_p]),
    "sai_plink_decode_host": (C.c_int, [_p, _i64, _i64, _i64, _p, _p, _i32, _i32, _p, _p, _p, _p, _i32]),
    "sai_plink_decode": (C.c_int, [_p, _p, _i64, _i64, _i64, _p, _p, _i32, _i32, _p, _i32, _p, _i32, _p, _i64, _p, _p]),
}

# entry points that never touch the GPU (plink_index.cpp)
HOST_SYMBOLS = tuple(n for n in SIGNATURES if n != "sai_plink_decode")


load, load_host = extension("PLINK", "saihip_plink.h", "sai_plink_abi_version", SAI_PLINK_ABI_VERSION, SIGNATURES, HOST_SYMBOLS,
                            built_from="plink")  # fmt: skip
