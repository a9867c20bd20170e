"""ctypes binding of the packed-ingest entry points of libsaihip.so (include/saihip_pgen_packed.h): the records of a
``.pgen`` decoded straight into the packed2 layout.

They live in the same shared library as the entry points of ``_ffi`` (and their host part in the sanitizer
build of the host units), but in a header and a table of their own, with their own version number:
``load()`` / ``load_host()`` take the handle ``_ffi`` returns and declare the prototypes below on it.  A
library without them is an error, as everywhere in this package.
"""

from __future__ import annotations

import ctypes as C

from . import _ffi

SAI_PGEN_PACKED_ABI_VERSION = 1

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names include/saihip_pgen_packed.h declares
SIGNATURES = {
    "sai_pgen_packed_abi_version": (C.c_int, []),
    "sai_pgen_pack2_host": (C.c_int, [_p, _i64, _i64, _p, _p, _p, _i32, _i32, _p, _i32, _i32, _p, _i64, _i64, _p, _p, _i32]),
    "sai_pgen_pack2": (C.c_int, [_p, _p, _i64, _i64, _p, _p, _p, _i32, _i32, _p, _i32, _i32, _p, _i64, _i64, _p, _p, _p]),
}

# entry points that never touch the GPU (pgen/pgen_pack2_host.cpp)
HOST_SYMBOLS = tuple(n for n in SIGNATURES if n != "sai_pgen_pack2")


def _attach(lib: C.CDLL, names) -> C.CDLL:
    if getattr(lib, "_sai_pgen_packed_attached", None) == tuple(names):
        return lib
    for name in names:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise RuntimeError(f"{name} is missing from libsaihip: the library was built without sai_amd/csrc/pgen/pgen_pack2* "
                               "(rebuild it: `python -c 'import __graft_entry__ as g; g.build()'`)") from None  # fmt: skip
        fn.restype, fn.argtypes = SIGNATURES[name]
    if lib.sai_pgen_packed_abi_version() != SAI_PGEN_PACKED_ABI_VERSION:
        raise RuntimeError(f"libsaihip: PGEN packed ABI {lib.sai_pgen_packed_abi_version()} != expected {SAI_PGEN_PACKED_ABI_VERSION}")
    lib._sai_pgen_packed_attached = tuple(names)
    return lib


def load() -> C.CDLL:
    """``_ffi.load()`` with every prototype of saihip_pgen_packed.h declared."""
    return _attach(_ffi.load(), tuple(SIGNATURES))


def load_host() -> C.CDLL:
    """``_ffi.load_host()`` with the host-only prototypes declared (the sanitizer build has no kernel)."""
    lib = _ffi.load_host()
    if lib is _ffi._lib:
        return load()
    return _attach(lib, HOST_SYMBOLS)
