"""ctypes binding of the BCF entry points of libsaihip.so (include/saihip_bcf.h).

As ``_ffi_plink``: the entry points live in the same shared library as those of ``_ffi`` (and their host part
in the sanitizer build of the host units), in a header and a table of their own, with their own version
number.  ``load()`` / ``load_host()`` take the handle ``_ffi`` returns and declare the prototypes below on it.
A library without them is an error, as everywhere in this package.
"""

from __future__ import annotations

import ctypes as C

from ._binding import extension

SAI_BCF_ABI_VERSION = 1
SAI_BCF_STATUS_RANGE = 1
SAI_BCF_STATUS_BAD_VALUE = 2
SAI_BCF_STATUS_BAD_INDEX = 3
SAI_BCF_GT_ALIGN = 16

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names include/saihip_bcf.h declares
SIGNATURES = {
    "sai_bcf_abi_version": (C.c_int, []),
    "sai_bcf_probe": (C.c_int, [C.c_char_p]),
    "sai_bcf_scan": (C.c_int, [C.c_char_p, C.c_char_p] + [C.POINTER(_i64)] * 4),
    "sai_bcf_stream_open": (
        C.c_int,
        [C.c_char_p, C.c_char_p, _i64, _i64, _i32, C.POINTER(C.c_char_p), C.POINTER(_i32), C.c_char_p, _i32, _p, _p, _i64, C.POINTER(_p)],
    ),
    "sai_bcf_stream_next": (C.c_int, [_p, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)] + [C.POINTER(_p)] * 5 + [C.POINTER(_i32)]),
    "sai_bcf_stream_selection": (C.c_int, [_p, _p, _i32, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)]),
    "sai_bcf_stream_stats": (C.c_int, [_p] + [C.POINTER(C.c_double)] * 5 + [C.POINTER(_i64)] * 2),
    "sai_bcf_stream_close": (C.c_int, [_p]),
    "sai_bcf_decode_host": (C.c_int, [_p, _i64, _i64, _p, _p, _p, _p, _i32, _i32, _p, _p, _p, _p, _i32]),
    "sai_bcf_decode": (C.c_int, [_p, _p, _i64, _i64, _p, _p, _p, _p, _i32, _i32, _p, _i32, _p, _i32, _p, _i64, _p, _p]),
}

# entry points that never touch the GPU (bcf/bcf_index.cpp)
HOST_SYMBOLS = tuple(n for n in SIGNATURES if n != "sai_bcf_decode")

load, load_host = extension("BCF", "saihip_bcf.h", "sai_bcf_abi_version", SAI_BCF_ABI_VERSION, SIGNATURES, HOST_SYMBOLS,
                            built_from="bcf")  # fmt: skip
