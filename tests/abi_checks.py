"""What the tests read out of the public headers under include/, and which binding module goes with which header."""

import re
import runpy

from conftest import ROOT


def header_text(header):
    """include/<header> without its comments."""
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)


def declared_names(header):
    """The sorted entry points (``sai_*(``) that include/<header> declares."""
    return sorted(set(re.findall(r"\b(sai_[a-z0-9_]+)\s*\(", header_text(header))))


def header_macro(header, name):
    """The integer a ``#define <name> <value>`` of include/<header> gives (decimal or hexadecimal)."""
    (value,) = re.findall(rf"^\s*#\s*define\s+{name}\s+\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]*\)?\s*(?://.*)?$", header_text(header), flags=re.M)
    return int(value, 0)


def header_of(module):
    """``sai_amd._ffi`` binds saihip.h, ``sai_amd._ffi_X`` binds saihip_X.h."""
    return "saihip" + module.__name__.rpartition(".")[2][len("_ffi"):] + ".h"


def version_constant(module):
    """The one ``SAI_*ABI_VERSION`` of a binding module: its name and value."""
    ((name, value),) = [(k, v) for k, v in vars(module).items() if re.fullmatch(r"SAI_(\w+_)?ABI_VERSION", k)]
    return name, value


def package_data_patterns():
    """The patterns setup.py adds to the package data of sai_amd, read without running its ``setup()``."""
    return runpy.run_path(str(ROOT / "setup.py"), run_name="setup")["EXTRA_PACKAGE_DATA"]["sai_amd"]
