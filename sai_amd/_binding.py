"""What every ``_ffi_X`` module does with its table: declare the prototypes of one family of entry points on the
handle ``_ffi`` returns, refuse a library that lacks one of them or answers another version number.  A group of entry
points that is internal to the package (declared in a ``.hpp`` under sai_amd/csrc, bound by the one module that calls
them: ``utils/bed_writer.py``) uses ``extension`` the same way, without being a family: it is not in ``family_modules``.

A family is a header of its own under include/ (``saihip_X.h``) with its own version number, bound by
``sai_amd/_ffi_X.py``: constants, ``SIGNATURES``, ``HOST_SYMBOLS``, and one call of ``extension``.  ``_ffi``
itself (include/saihip.h) is not built on this module: it opens the library, and its text is part of the digest
the stored measurements name.
"""

from __future__ import annotations

import ctypes as C
import importlib
from pathlib import Path

from . import _ffi

REBUILD = "`python -c 'import __graft_entry__ as g; g.build()'`"


def family_modules() -> list:
    """``_ffi`` and every ``_ffi_*.py`` of the package, imported, in sorted order of their names."""
    names = sorted(p.stem for p in Path(__file__).resolve().parent.glob("_ffi_*.py"))
    return [_ffi, *(importlib.import_module(f"{__package__}.{name}") for name in names)]


def extension(tag: str, header: str, version_symbol: str, version: int, signatures: dict, host_symbols, built_from: str):
    """``(load, load_host)`` of one family or internal group.  ``tag`` names it in the version message ("PLINK"), ``header``
    is the file that declares it, as the docstrings name it (a family's file under include/; a path from the repository
    root for an internal group), ``version_symbol`` the entry point that answers ``version``, ``built_from`` the sources
    under sai_amd/csrc a library without these entry points was built without."""
    memo = "_sai_attached_" + version_symbol

    def attach(lib: C.CDLL, names: tuple) -> C.CDLL:
        if getattr(lib, memo, None) == names:
            return lib
        for name in names:
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise RuntimeError(f"{name} is missing from libsaihip: the library was built without sai_amd/csrc/{built_from} "
                                   f"(rebuild it: {REBUILD})") from None  # fmt: skip
            fn.restype, fn.argtypes = signatures[name]
        found = getattr(lib, version_symbol)()
        if found != version:
            raise RuntimeError(f"libsaihip: {tag} ABI {found} != expected {version}")
        setattr(lib, memo, names)
        return lib

    def load() -> C.CDLL:
        return attach(_ffi.load(), tuple(signatures))

    def load_host() -> C.CDLL:
        lib = _ffi.load_host()
        if lib is _ffi._lib:
            return load()
        return attach(lib, tuple(host_symbols))

    load.__doc__ = f"``_ffi.load()`` with every prototype of {header} declared."
    load_host.__doc__ = "``_ffi.load_host()`` with the host-only prototypes declared (the sanitizer build has no kernel)."
    return load, load_host
