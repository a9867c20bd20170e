"""CPU-side checks of the C ABI: the library builds/loads, exports every symbol that
include/saihip.h declares, refuses to run without a device, and its host-side synthetic
generator equals the numpy definition.  No GPU compute is attempted here."""

import ctypes as C

import numpy as np
import pytest

import abi_checks
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from sai_amd import _ffi

    return _ffi.load()


def families():
    """(header, binding module) of saihip.h and of every family of entry points: the modules the build loads."""
    from sai_amd._binding import family_modules

    return [(abi_checks.header_of(module), module) for module in family_modules()]


def test_every_header_has_one_binding_module_and_every_module_its_header():
    headers = sorted(p.name for p in (ROOT / "include").iterdir())
    assert sorted(header for header, _ in families()) == headers and len(headers) >= 10
    from sai_amd import _build

    assert sorted(p.name for p in _build.PUBLIC_HEADERS) == headers


@pytest.mark.parametrize("header", sorted(p.name for p in (ROOT / "include").iterdir()))
def test_header_binding_and_library_agree(lib, header):
    (module,) = [m for h, m in families() if h == header]
    names = abi_checks.declared_names(header)
    assert names and names == sorted(module.SIGNATURES)
    loaded = module.load()
    for n in names:
        assert hasattr(loaded, n), f"{n} is declared in {header} but not exported"
    constant, value = abi_checks.version_constant(module)
    (answer,) = [n for n in names if n.endswith("abi_version")]
    assert answer == constant.lower() and abi_checks.header_macro(header, constant) == value == getattr(loaded, answer)()
    assert set(module.HOST_SYMBOLS) <= set(module.SIGNATURES) and answer in module.HOST_SYMBOLS
    assert module.load_host() is not None


def test_a_library_without_a_family_or_of_another_version_is_refused(lib):
    """The two refusals of ``_binding.extension``, on a handle that stands for a library built without the family."""
    from sai_amd import _binding, _ffi_plink

    class Without:
        def __init__(self, missing=(), version=_ffi_plink.SAI_PLINK_ABI_VERSION):
            self.missing, self.version = missing, version

        def __getattr__(self, name):
            if name.startswith("_") or name in self.missing:
                raise AttributeError(name)
            return type("Fn", (), {"__call__": lambda fn: self.version})()

    real = _binding._ffi._lib
    try:
        _binding._ffi._lib = Without(missing=("sai_plink_decode",))
        with pytest.raises(RuntimeError) as exc:
            _ffi_plink.load()
        assert str(exc.value) == ("sai_plink_decode is missing from libsaihip: the library was built without sai_amd/csrc/plink "
                                  "(rebuild it: `python -c 'import __graft_entry__ as g; g.build()'`)")  # fmt: skip
        _binding._ffi._lib = Without(version=7)
        with pytest.raises(RuntimeError) as exc:
            _ffi_plink.load()
        assert str(exc.value) == "libsaihip: PLINK ABI 7 != expected 1"
        _binding._ffi._lib = handle = Without()
        assert _ffi_plink.load() is handle and handle._sai_attached_sai_plink_abi_version == tuple(_ffi_plink.SIGNATURES)
    finally:
        _binding._ffi._lib = real
    assert _ffi_plink.load() is lib


def test_staleness_inputs_are_the_list_the_build_used_to_spell_out():
    """What an object is stale against, found by rule, is what sai_amd/_build.py listed by hand while it had ten
    headers and six directories of .hpp files: those names, once, here."""
    from sai_amd import _build

    include, csrc = ROOT / "include", _build.CSRC
    spelled_out = [include / "saihip.h", include / "saihip_plink.h", include / "saihip_eigenstrat.h", include / "saihip_pgen.h",
                   include / "saihip_packed_ingest.h", include / "saihip_pgen_packed.h", include / "saihip_bcf.h", include / "saihip_bcf_device.h",
                   include / "saihip_bcf_index.h", include / "saihip_packed_stats.h", *csrc.glob("*.hpp"), *csrc.glob("plink/*.hpp"),
                   *csrc.glob("eigenstrat/*.hpp"), *csrc.glob("pgen/*.hpp"), *csrc.glob("bcf/*.hpp"), *csrc.glob("packed_stats/*.hpp")]  # fmt: skip
    inputs = _build.staleness_inputs()
    assert sorted(inputs) == sorted(spelled_out) and len(set(inputs)) == len(inputs) and all(p.is_file() for p in inputs)


def test_units_exist_have_objects_of_their_own_and_their_directories_are_packaged():
    from sai_amd import _build

    assert all((_build.CSRC / u).is_file() for u in _build.UNITS) and set(_build.HOST_UNITS) < set(_build.UNITS)
    assert _build.UNITS[-len(_build.HOST_UNITS):] == _build.HOST_UNITS and all(u.endswith(".cpp") for u in _build.HOST_UNITS)
    assert sorted(str(p.relative_to(_build.CSRC)) for ext in ("hip", "cpp") for p in _build.CSRC.rglob(f"*.{ext}")) == sorted(_build.UNITS)
    _build.check_object_names(_build.UNITS)
    with pytest.raises(RuntimeError, match=r"^units with the same object name: bcf/core\.cpp core\.hip$"):
        _build.check_object_names([*_build.UNITS, "bcf/core.cpp"])
    patterns = abi_checks.package_data_patterns()
    for unit in _build.UNITS:
        directory, _, name = unit.rpartition("/")
        assert not directory or f"csrc/{directory}/*{name[name.rindex('.'):]}" in patterns, unit
    assert all(f"csrc/{p.parent.name}/*.hpp" in patterns for p in _build.CSRC.glob("*/*.hpp"))


def test_compile_jobs_follow_max_jobs(monkeypatch):
    import os

    from sai_amd import _build

    cpus = os.cpu_count() or 1
    for value, want in (("1", 1), (str(cpus + 5), cpus), ("0", cpus), ("-3", cpus), ("many", cpus), ("", cpus)):
        monkeypatch.setenv("MAX_JOBS", value)
        assert _build._max_jobs() == want, value
    monkeypatch.delenv("MAX_JOBS")
    assert _build._max_jobs() == cpus


def test_host_objects_are_compiled_once_per_kind(tmp_path, tmp_path_factory):
    import os

    import native_build

    first = native_build.host_objects("san", tmp_path_factory)
    from sai_amd import _build

    assert len(first) == len(set(first)) == len(_build.HOST_UNITS)
    stamps = [os.stat(o).st_mtime_ns for o in first]
    assert native_build.host_objects("san", tmp_path_factory) == first and [os.stat(o).st_mtime_ns for o in first] == stamps
    exe = native_build.dump_program("packed_freqs_dump", tmp_path_factory)["san"]
    assert os.access(exe, os.X_OK) and [os.stat(o).st_mtime_ns for o in first] == stamps
    # a refusal of the compiler fails the test with the compiler's words
    bad = tmp_path / "bad.cpp"
    bad.write_text("int main() { return no_such_name; }\n")
    with pytest.raises(AssertionError, match="no_such_name"):
        native_build.compile_object(bad, tmp_path / "bad.o", "san")
    assert not (tmp_path / "bad.o").exists()


def test_header_and_binding_agree(lib):
    from sai_amd import _ffi

    names = abi_checks.declared_names("saihip.h")
    assert len(names) >= 15
    assert sorted(_ffi.SIGNATURES) == names
    for n in names:
        assert hasattr(lib, n), f"{n} is declared in saihip.h but not exported"
    assert lib.sai_abi_version() == _ffi.SAI_ABI_VERSION
    assert lib.sai_build_arch() == b"gfx950"
    assert C.sizeof(_ffi.SaiWindowRecord) == 24
    assert C.sizeof(_ffi.SaiParams) == 32 + _ffi.SAI_MAX_SRC * 20 == 312  # op (4) + y (8) + one_minus_y (8) per source
    assert C.sizeof(_ffi.SaiPop) == 16


def test_tiled_bytes(lib):
    assert lib.sai_tiled_bytes(0, 5) == 0
    assert lib.sai_tiled_bytes(1, 5) == 5 * 64
    assert lib.sai_tiled_bytes(64, 1000) == 64000
    assert lib.sai_tiled_bytes(65, 1000) == 128000
    assert lib.sai_tiled_bytes(-1, 3) == -1


def test_fails_loudly_without_gpu(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from sai_amd import _ffi
    from sai_amd.engine import Engine

    ctx = C.c_void_p()
    rc = lib.sai_ctx_create(0, C.byref(ctx))
    assert rc != 0 and not ctx.value
    assert b"no CPU fallback" in lib.sai_last_error() or lib.sai_last_error()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Engine(0)
    from sai_amd.stats import UStatistic

    g = np.zeros((2, 2), dtype=np.int64)
    with pytest.raises(RuntimeError):
        UStatistic(ref_gts=g, tgt_gts=g, src_gts_list=[g], ref_ploidy=2, tgt_ploidy=2, src_ploidy_list=[2]).compute(
            pos=np.array([1, 2]), w=0.5, x=0.5, y_list=[("=", 1.0)], anc_allele_available=True
        )
    assert _ffi.SaiHipError(-3, "x").status == -3


def test_plan_and_plane_entry_points_refuse_bad_arguments(lib):
    """The round-3 entry points without a GPU: sizes, NULL handles and a ctx that cannot exist are
    answered with a status and a message, never a crash."""
    from sai_amd import _ffi

    assert lib.sai_plane_words(64, 1) == 3 and lib.sai_plane_words(65, 2) == 12 and lib.sai_plane_words(0, 5) == 0
    assert lib.sai_plane_words(-1, 1) == -1 and lib.sai_plane_words(10, -1) == -1
    plan = C.c_void_p()
    assert lib.sai_plan_create(None, C.byref(plan)) == _ffi.SAI_ERR_ARG and not plan.value
    assert lib.sai_plan_run(None, None) == _ffi.SAI_ERR_ARG and b"NULL" in lib.sai_last_error()
    assert lib.sai_plan_add_copy_to_host(None, None, None, 0) == _ffi.SAI_ERR_ARG
    assert lib.sai_plan_add_copy_to_host(None, None, None, -5) == _ffi.SAI_ERR_ARG
    assert lib.sai_plan_add_window_bounds(None, None, 0, 0, None, None, None, None, None, None) == _ffi.SAI_ERR_ARG
    assert lib.sai_plan_destroy(None) == 0
    a = C.c_int64()
    assert lib.sai_bgzf_stream_region(None, C.byref(a), C.byref(a), C.byref(a)) == _ffi.SAI_ERR_ARG


def test_params_packing():
    from sai_amd import _ffi

    p = _ffi.make_params(0.01, 0.5, 0.95, [("=", 0.9), (">=", 0.2)], False)
    assert (p.w, p.x, p.quantile, p.n_src, p.anc_allele_available) == (0.01, 0.5, 0.95, 2, 0)
    assert list(p.op)[:2] == [0, 4]
    assert p.one_minus_y[0] == 1 - 0.9 and p.one_minus_y[0] != 0.1  # the f64 mirror, not the decimal one
    seven = _ffi.make_params(0.1, 0.1, 0.5, [("=", 1.0)] * 7, True)  # more than a streaming pass takes: counts in groups + site_flags
    assert seven.n_src == 7 > _ffi.SAI_FUSED_SRC and list(seven.y)[:8] == [1.0] * 7 + [0.0]
    with pytest.raises(ValueError):
        _ffi.make_params(0.1, 0.1, 0.5, [("=", 1.0)] * (_ffi.SAI_MAX_SRC + 1), True)


@pytest.mark.parametrize(
    "pop_stream,n_ind,ploidy,mpm", [(0, 33, 2, 0), (1, 17, 2, 1000), (2, 2, 2, 20000), (3, 3, 4, 0), (1, 8, 1, 500000), (0, 5, 3, 0)]
)
def test_host_synth_equals_numpy_definition(lib, pop_stream, n_ind, ploidy, mpm):
    from oracle import synth_numpy as S
    from sai_amd import _ffi

    seed, chrom, site0, n_sites = 20260630 + pop_stream, 7, 99000, 3000
    got = np.empty((n_sites, n_ind), dtype=np.int8)
    _ffi.check(lib.sai_synth_fill_host(seed, chrom, site0, n_sites, pop_stream, n_ind, ploidy, mpm,
                                       got.ctypes.data_as(C.c_void_p)))  # fmt: skip
    exp = S.genotypes(seed, chrom, site0, n_sites, pop_stream, n_ind, ploidy, mpm)
    assert np.array_equal(got, exp)
    gaps = np.empty(n_sites, dtype=np.int32)
    _ffi.check(lib.sai_synth_gaps_host(seed, chrom, site0, n_sites, gaps.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(gaps, S.gaps(seed, chrom, site0, n_sites))


def test_synth_statistics_are_sane(lib):
    """The synthetic chromosome must exercise the statistics: ~0.1 % introgressed sites with
    ref fixed 0 / src fixed ALT, rare-variant background, and U candidates at default thresholds."""
    from oracle import synth_numpy as S

    seed, n = 20260632, 200000
    ref = S.genotypes(seed, 1, 0, n, 0, 20, 2)
    tgt = S.genotypes(seed, 1, 0, n, 1, 20, 2)
    src = S.genotypes(seed, 1, 0, n, 2, 2, 2)
    intro = (ref.sum(1) == 0) & (src.min(1) == 2) & (tgt.mean(1) / 2 > 0.1)
    assert 100 < intro.sum() < 400
    assert 0.15 < (ref.mean() / 2) < 0.25  # E[u^4] = 0.2
    g = S.gaps(seed, 1, 0, n)
    assert 24 < g.mean() < 26
