"""ctypes binding of the entry points of include/saihip_bcf_device.h: the BCF route whose members are inflated and
whose records are found on the GPU -- the two kernels, their host twins, the stitch and the feed.

As ``_ffi_bcf``: the entry points live in libsaihip.so (their host part also in the sanitizer build of the host
units), in a header and a table of their own, with their own version number.  A library without them is an error.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import extension

SAI_BCF_DEVICE_ABI_VERSION = 1
SAI_BCF_MAX_HEADS = 8
SAI_BCF_MAX_HEADS_LIMIT = 64
SAI_BCF_SEG_MIN = 256
SAI_BCF_SEG_MAX = 65536
SAI_BCF_ALLELE_BYTES = 12
SAI_BCF_HOST_ROUTE = 1
SAI_BCF_CHAIN_BROKEN = 1
SAI_BCF_CHAIN_INCOMPLETE = 2
SAI_BCF_HEAD_NO_GT = 1
SAI_BCF_HEAD_GT_NOT_INT = 2
SAI_BCF_HEAD_LEAVES = 4
SAI_BCF_HEAD_SHARED_LEAVES = 8
SEG_DENSE = 1 << 30  # bit of seg_info

# sai_bcf_chain and sai_bcf_record_head as numpy sees them
CHAIN = np.dtype([("head", "<u4"), ("chain_exit", "<u4"), ("n_records", "<u4"), ("flags", "<u4")])
HEAD = np.dtype([("off", "<u4"), ("gt_off", "<u4"), ("l_shared", "<u4"), ("l_indiv", "<u4"), ("chrom", "<i4"), ("pos0", "<i4"),
                 ("gt_len", "<i4"), ("n_allele", "<u2"), ("n_fmt", "u1"), ("flags", "u1"), ("ref_len", "u1"), ("alt_len", "u1"),
                 ("gt_width", "u1"), ("reserved0", "u1"), ("ref", "S12"), ("alt", "S12"), ("reserved1", "<u4")])  # fmt: skip
assert CHAIN.itemsize == 16 and HEAD.itemsize == 64

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
_pi32, _pi64, _pp = C.POINTER(_i32), C.POINTER(_i64), C.POINTER(C.c_void_p)

# name -> (restype, argtypes): the names include/saihip_bcf_device.h declares
SIGNATURES = {
    "sai_bcf_device_abi_version": (C.c_int, []),
    "sai_bcf_chain_segments": (C.c_int, [_p, _p, _i64, _i32, _i32, _p, _i32, _i32, _p, _p, _p]),
    "sai_bcf_chain_segments_host": (C.c_int, [_p, _i64, _i32, _i32, _p, _i32, _i32, _p, _p]),
    "sai_bcf_stitch": (C.c_int, [_p, _p, _i64, _i32, _i32, _i64, _p, _p, _pi64, _pi64, _pi32]),
    "sai_bcf_record_heads": (C.c_int, [_p, _p, _i64, _i32, _p, _p, _i64, _i64, _i64, _i32, _p, _p]),
    "sai_bcf_record_heads_host": (C.c_int, [_p, _i64, _i32, _p, _p, _i64, _i64, _i64, _i32, _p]),
    "sai_bcf_feed_open": (C.c_int, [C.c_char_p, C.c_char_p, _i64, _i64, _i32, C.POINTER(C.c_char_p), C.c_char_p, _p, _p, _i64, _i64, _i32, _pp]),
    "sai_bcf_feed_next": (C.c_int, [_p, _pi32, _pi64, _pi32, _pp, _pi64, _pi64, _pi32]),
    "sai_bcf_feed_release": (C.c_int, [_p]),
    "sai_bcf_feed_select": (C.c_int, [_p, _p, _i64, _pi64] + [_pp] * 5 + [_pi32, _pi32]),
    "sai_bcf_feed_selection": (C.c_int, [_p, _p, _i32, _p, _i32, _pi32, _pi32, _pi64, _pi64, _pi64, _pi64, _pi64, _pi64]),
    "sai_bcf_feed_stats": (C.c_int, [_p] + [C.POINTER(C.c_double)] * 4 + [_pi64]),
    "sai_bcf_feed_close": (C.c_int, [_p]),
}

# entry points that never touch the GPU (bcf/bcf_feed.cpp)
HOST_SYMBOLS = tuple(n for n in SIGNATURES if n not in ("sai_bcf_chain_segments", "sai_bcf_record_heads"))


load, load_host = extension("BCF device", "saihip_bcf_device.h", "sai_bcf_device_abi_version", SAI_BCF_DEVICE_ABI_VERSION,
                            SIGNATURES, HOST_SYMBOLS, built_from="bcf/bcf_walk.hip or bcf_feed.cpp")  # fmt: skip
