"""ctypes binding of the entry points of include/saihip_bcf_index.h: the .csi index of a BCF file and the variants
of ``sai_bcf_stream_open`` / ``sai_bcf_feed_open`` that begin where it says.

As ``_ffi_bcf_device``: the entry points live in libsaihip.so (and, none of them touching the GPU, in the sanitizer
build of the host units), in a header and a table of their own, with their own version number.  A library without
them is an error.
"""

from __future__ import annotations

import ctypes as C

from ._binding import extension

SAI_BCF_INDEX_ABI_VERSION = 1
SAI_BCF_INDEX_NONE = 0
SAI_BCF_INDEX_SEEK = 1
SAI_BCF_INDEX_WALK = 2

_p, _i32, _i64, _u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
_pi32, _pi64, _pu64, _pp = C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_u64), C.POINTER(C.c_void_p)

# name -> (restype, argtypes): the names include/saihip_bcf_index.h declares
SIGNATURES = {
    "sai_bcf_index_abi_version": (C.c_int, []),
    "sai_bcf_index_open": (C.c_int, [C.c_char_p, _i64, _pp]),
    "sai_bcf_index_info": (C.c_int, [_p, _pi32, _pi32, _pi32, _pi64]),
    "sai_bcf_index_query": (C.c_int, [_p, _i32, _i64, _i64, _pi32, _pu64]),
    "sai_bcf_index_close": (C.c_int, [_p]),
    "sai_bcf_stream_open_at": (
        C.c_int,
        [C.c_char_p, C.c_char_p, _i64, _i64, _i32, C.POINTER(C.c_char_p), _pi32, C.c_char_p, _i32, _p, _p, _i64, _p, _pp],
    ),
    "sai_bcf_stream_seek_stats": (C.c_int, [_p, _pi32, _pu64, _pi64, _pi64]),
    "sai_bcf_feed_open_at": (C.c_int, [C.c_char_p, C.c_char_p, _i64, _i64, _i32, C.POINTER(C.c_char_p), C.c_char_p, _p, _p, _i64, _i64, _i32, _p, _pp]),
    "sai_bcf_feed_seek_stats": (C.c_int, [_p, _pi32, _pu64, _pi32, _pi64, _pi64]),
}

# every one of them is plain C++ (bcf/csi_index.cpp, bcf/bcf_index.cpp, bcf/bcf_feed.cpp)
HOST_SYMBOLS = tuple(SIGNATURES)


load, load_host = extension("BCF index", "saihip_bcf_index.h", "sai_bcf_index_abi_version", SAI_BCF_INDEX_ABI_VERSION, SIGNATURES,
                            HOST_SYMBOLS, built_from="bcf/csi_index.cpp")  # fmt: skip
