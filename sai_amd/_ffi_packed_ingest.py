"""ctypes binding of the packed-ingest entry points of libsaihip.so (include/saihip_packed_ingest.h): ``.bed`` rows
decoded straight into the packed2 layout.

They live in the same shared library as the entry points of ``_ffi`` (and their host part in the sanitizer
build of the host units), but in a header and a table of their own, with their own version number:
``load()`` / ``load_host()`` take the handle ``_ffi`` returns and declare the prototypes below on it.  A
library without them is an error, as everywhere in this package.
"""

from __future__ import annotations

import ctypes as C

from ._binding import extension

SAI_PACKED_INGEST_ABI_VERSION = 1

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names include/saihip_packed_ingest.h declares
SIGNATURES = {
    "sai_packed_ingest_abi_version": (C.c_int, []),
    "sai_bed_pack2_host": (C.c_int, [_p, _i64, _i64, _i64, _p, _p, _i32, _i32, _p, _i32, _i32, _p, _i64, _i64, _p, _p, _i32]),
    "sai_bed_pack2": (C.c_int, [_p, _p, _i64, _i64, _i64, _p, _p, _i32, _i32, _p, _i32, _i32, _p, _i64, _i64, _p, _p, _p]),
}

# entry points that never touch the GPU (plink/bed_pack2_host.cpp)
HOST_SYMBOLS = tuple(n for n in SIGNATURES if n != "sai_bed_pack2")

load, load_host = extension("packed-ingest", "saihip_packed_ingest.h", "sai_packed_ingest_abi_version", SAI_PACKED_INGEST_ABI_VERSION, SIGNATURES, HOST_SYMBOLS,
                            built_from="plink/bed_pack2*")  # fmt: skip
