"""Stand-alone programs of tests/native/ linked against the host units of libsaihip: under ASan + UBSan with the
runtimes linked in statically ("san"), or with the flags of the library itself ("plain").  The host units are
compiled once per kind in a pytest process, whichever modules ask; each program adds its own source and a link."""

import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

from conftest import ROOT

_objects = {}  # kind -> the object files of HOST_UNITS, once they are all there


def flags_of(kind):
    import __graft_entry__ as entry

    return {"san": [*entry.SAN_FLAGS, "-static-libasan", "-static-libubsan"], "plain": list(entry.HOST_FLAGS)}[kind]


def _gxx():
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed to build the stand-alone programs"
    return gxx


def compile_object(src, obj, kind):
    """One source into one object; a refusal of the compiler fails the test with its message."""
    res = subprocess.run([_gxx(), *flags_of(kind), f"-I{ROOT / 'include'}", "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return str(obj)


def host_objects(kind, tmp_path_factory):
    """The objects of every unit of HOST_UNITS, compiled for ``kind`` at most once per pytest process."""
    import __graft_entry__ as entry

    if kind not in _objects:
        out = tmp_path_factory.mktemp(f"host_units_{kind}")
        with ThreadPoolExecutor(8) as pool:
            _objects[kind] = list(pool.map(lambda u: compile_object(entry.CSRC / u, out / (u.replace("/", "_") + ".o"), kind), entry.HOST_UNITS))
    return _objects[kind]


def dump_program(name, tmp_path_factory, kinds=("san",)):
    """tests/native/<name>.cpp linked against the host units, once per kind: {kind: path of the program}."""
    out = tmp_path_factory.mktemp(name)
    exes = {}
    for kind in kinds:
        objs = [*host_objects(kind, tmp_path_factory), compile_object(ROOT / "tests" / "native" / f"{name}.cpp", out / f"{kind}_{name}.o", kind)]
        exes[kind] = str(out / f"{name}_{kind}")
        res = subprocess.run([_gxx(), *flags_of(kind), *objs, "-o", exes[kind], "-lz", "-lpthread", "-ldl"], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
    return exes


def run_native(exe, args):
    """Run a program of ``dump_program``: a finding of ASan ends it with status 97, one of UBSan with 98."""
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:exitcode=97:verify_asan_link_order=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=98")
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=300)
