"""The DD table entry points on the host: ``sai_site_absdiff_table_host`` and ``sai_window_dd_table_host`` against the
numpy statements of tests/dd_table_cases.py, the counter of unlisted source bytes (and that the fixtures of
test_dd_table_device.py have none), every argument error, the agreement of sources, binding and library, the twins as a
program of their own under the sanitizers, and the admission rule of the route in ``FeaturePreprocessor.score_windows``
with the bookkeeping of ``dd_table.combination_dd`` on a stub engine.  tests/test_dd_table_device.py runs the kernels
against the twins on the same shapes."""

import ctypes as C

import numpy as np
import pytest

import abi_checks
import dd_table_cases as D
import native_build
import sum_order_cases as S
from conftest import ROOT


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def values_array(values):
    return (C.c_int8 * len(values))(*values)


def pop_of(tiles, n_ind):
    from sai_amd import _ffi

    p = _ffi.SaiPop()
    p.tiles, p.n_ind, p.ploidy = (tiles.ctypes.data if tiles is not None and tiles.size else None), n_ind, 1
    return p


def host_table(g, values):
    """One ``sai_site_absdiff_table_host`` call on int8 [sites][individuals]: uint32 [len(values)][sites]."""
    from sai_amd import _ffi, dd_table

    lib = dd_table.load_host()
    n_sites, n_ind = g.shape
    tiles = D.tile_numpy(g)
    table = np.full((len(values), n_sites), 0xDEADBEEF, dtype=np.uint32)
    _ffi.check(lib.sai_site_absdiff_table_host(n_sites, C.byref(pop_of(tiles, n_ind)), len(values), values_array(values), ptr(table)), lib)
    return table


def host_window(src, values, table_ref, n_ref, table_tgt, n_tgt, windows):
    """One ``sai_window_dd_table_host`` call: (d f64 [n_windows][n_src], dd f64 [n_windows], n_unlisted)."""
    from sai_amd import _ffi, dd_table

    lib = dd_table.load_host()
    n_sites, n_src = src.shape
    tiles = D.tile_numpy(src)
    w = np.asarray(windows, dtype=np.int32).reshape(-1, 2)
    lo, hi = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
    scratch, dd = np.full((len(w), n_src), -7.0), np.full(len(w), -7.0)
    n_unlisted = np.full(1, -1, dtype=np.int32)
    tr, tt = np.ascontiguousarray(table_ref, dtype=np.uint32), np.ascontiguousarray(table_tgt, dtype=np.uint32)
    _ffi.check(lib.sai_window_dd_table_host(n_sites, C.byref(pop_of(tiles, n_src)), len(values), values_array(values), ptr(tr), n_ref, ptr(tt), n_tgt,
                                            len(w), ptr(lo), ptr(hi), ptr(scratch), ptr(dd), ptr(n_unlisted)), lib)  # fmt: skip
    return scratch, dd, int(n_unlisted[0])


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("n_ind", D.N_IND)
def test_table_twin_equals_the_numpy_statement(n_ind, kind):
    for n_sites in D.N_SITES:
        g = D.genotypes(n_sites, n_ind, kind)
        for values in D.VALUE_LISTS:
            want = D.table_numpy(values, g)
            assert want.shape == (len(values), n_sites) and want.max(initial=0) <= 255 * max(n_ind, 1)
            assert np.array_equal(host_table(g, values), want), (n_ind, n_sites, values)


def test_table_twin_at_the_extremes_of_int8():
    """|127 - (-128)| = 255 per individual, both ways round."""
    for v, fill in ((127, -128), (-128, 127)):
        g = np.full((65, 17), fill, dtype=np.int8)
        assert (host_table(g, (v, 0)) == np.array([[255 * 17], [abs(fill) * 17]])).all()


@pytest.mark.parametrize("n_src", D.N_SRC)
def test_window_twin_equals_numpy_order(n_src):
    _, _, table_ref, table_tgt = D.window_block()
    want_d, want_dd, unlisted = D.window_expected(n_src, S.WINDOWS)
    assert unlisted == 0
    d, dd, n_unlisted = host_window(D.window_source(n_src), D.DD_VALUES, table_ref, S.N_REF, table_tgt, S.N_TGT, S.WINDOWS)
    assert n_unlisted == 0 and same_bits(d, want_d) and same_bits(dd, want_dd)


def test_window_twin_on_the_capacity_windows_and_other_value_lists():
    n = D.long_block_sites()
    _, _, table_ref, table_tgt = D.window_block(n)
    windows = D.capacity_windows()
    lo, hi = S.clamp(windows, n)
    assert (hi - lo).max() == n and D.stage_sites(7) in (hi - lo) and D.stage_sites(7) + 1 in (hi - lo)
    for n_src in (5, 9):
        want_d, want_dd, unlisted = D.window_expected(n_src, windows, n)
        d, dd, n_unlisted = host_window(D.window_source(n_src, n), D.DD_VALUES, table_ref, S.N_REF, table_tgt, S.N_TGT, windows)
        assert unlisted == n_unlisted == 0 and same_bits(d, want_d) and same_bits(dd, want_dd)
    # genotypes over all of int8, eight values with both ends: the bytes outside the list add nothing and are counted
    values = D.VALUE_LISTS[2]
    ref, tgt, src = (D.genotypes(130, k, "all", seed=5) for k in (S.N_REF, S.N_TGT, 17))
    table_ref, table_tgt = D.table_numpy(values, ref), D.table_numpy(values, tgt)
    ad_ref, unlisted = D.terms_of(table_ref, values, src)
    ad_tgt, _ = D.terms_of(table_tgt, values, src)
    windows = ((0, 130), (0, 64), (60, 70), (129, 130), (7, 7))
    want_d, want_dd = S.dd_expected(ad_ref, ad_tgt, windows)
    d, dd, n_unlisted = host_window(src, values, table_ref, S.N_REF, table_tgt, S.N_TGT, windows)
    in_windows = sum(int((~np.isin(src[a:b], values)).sum()) for a, b in windows)
    assert 0 < unlisted and 0 < n_unlisted == in_windows and same_bits(d, want_d) and same_bits(dd, want_dd)


def test_one_unlisted_byte_is_counted_and_the_device_fixtures_have_none():
    _, _, table_ref, table_tgt = D.window_block()
    src = D.window_source(5).copy()
    src[100, 3] = 5  # not in DD_VALUES
    d, dd, n_unlisted = host_window(src, D.DD_VALUES, table_ref, S.N_REF, table_tgt, S.N_TGT, [(0, 256), (0, 100), (100, 101)])
    assert n_unlisted == 2  # once per window that holds the site
    for n_src in D.N_SRC:
        assert np.isin(D.window_source(n_src), D.DD_VALUES).all()
    for n_src in (5, 9):
        assert np.isin(D.window_source(n_src, D.long_block_sites()), D.DD_VALUES).all()


def test_every_argument_error():
    from sai_amd import _ffi, dd_table

    lib = dd_table.load_host()
    g = D.genotypes(70, 3, "listed")
    tiles = D.tile_numpy(g)
    table = np.full((2, 70), 7, dtype=np.uint32)

    def call_table(n_sites=70, pop="ok", n_ind=3, n_values=2, values=(0, 1), out=table, null_tiles=False):
        p = pop_of(None if null_tiles else tiles, n_ind)
        rc = lib.sai_site_absdiff_table_host(n_sites, C.byref(p) if pop == "ok" else None, n_values, None if values is None else values_array(values), ptr(out))
        return rc, lib.sai_last_error().decode()

    assert call_table()[0] == 0 and np.array_equal(table, D.table_numpy((0, 1), g))
    for kw, message in [
        (dict(n_sites=-1), "n_sites out of range"),
        (dict(n_sites=2**31 - 1), "n_sites out of range"),
        (dict(pop=None), "NULL population"),
        (dict(n_ind=-1), "bad n_ind"),
        (dict(n_ind=2**24 + 1), "bad n_ind"),
        (dict(n_values=0), "n_values must be 1..8"),
        (dict(n_values=9, values=tuple(range(9))), "n_values must be 1..8"),
        (dict(values=None), "values is NULL"),
        (dict(values=(1, 1)), "values must be distinct"),
        (dict(out=None), "NULL buffer"),
        (dict(null_tiles=True), "NULL buffer"),
    ]:
        table[:] = 7
        rc, text = call_table(**kw)
        assert rc == _ffi.SAI_ERR_ARG and message in text, (kw, rc, text)
        assert (table == 7).all()  # a refused call writes nothing
    # n_sites == 0 is fine and touches nothing; so is a population of nobody, whose table is zero
    assert call_table(n_sites=0, out=None, null_tiles=True)[0] == 0 and (table == 7).all()
    assert call_table(n_ind=0, null_tiles=True)[0] == 0 and (table == 0).all()

    table_ref, table_tgt = (np.ascontiguousarray(D.table_numpy(D.DD_VALUES, D.genotypes(70, k, "listed", seed=k)), dtype=np.uint32) for k in (7, 3))
    lo, hi = np.array([0, 10], dtype=np.int32), np.array([70, 20], dtype=np.int32)
    scratch, dd, counter = np.full((2, 3), -7.0), np.full(2, -7.0), np.full(1, -1, dtype=np.int32)

    def call_window(n_sites=70, src="ok", n_src=3, n_values=7, values=D.DD_VALUES, tr=table_ref, n_ref=7, tt=table_tgt, n_tgt=3, n_windows=2, lo=lo,
                    hi=hi, scratch=scratch, dd=dd, counter=counter, null_tiles=False):  # fmt: skip
        p = pop_of(None if null_tiles else tiles, n_src)
        rc = lib.sai_window_dd_table_host(n_sites, C.byref(p) if src == "ok" else None, n_values, None if values is None else values_array(values),
                                          ptr(tr), n_ref, ptr(tt), n_tgt, n_windows, ptr(lo), ptr(hi), ptr(scratch), ptr(dd), ptr(counter))  # fmt: skip
        return rc, lib.sai_last_error().decode()

    assert call_window()[0] == 0 and counter[0] == 0 and (dd != -7.0).all()
    for kw, message in [
        (dict(n_sites=-1), "size out of range"),
        (dict(n_sites=2**31 - 1), "size out of range"),
        (dict(n_windows=-1), "size out of range"),
        (dict(src=None), "NULL population"),
        (dict(n_src=0), "every population needs an individual"),
        (dict(n_ref=0), "every population needs an individual"),
        (dict(n_tgt=-2), "every population needs an individual"),
        (dict(n_src=2**24 + 1), "bad n_ind"),
        (dict(n_values=0), "n_values must be 1..8"),
        (dict(n_values=9, values=tuple(range(9))), "n_values must be 1..8"),
        (dict(values=None), "values is NULL"),
        (dict(values=(0, 1, 2, 3, 4, 5, 0)), "values must be distinct"),
        (dict(counter=None), "NULL buffer"),
        (dict(tr=None), "NULL buffer"),
        (dict(tt=None), "NULL buffer"),
        (dict(null_tiles=True), "NULL buffer"),
        (dict(lo=None), "NULL buffer"),
        (dict(hi=None), "NULL buffer"),
        (dict(scratch=None), "NULL buffer"),
        (dict(dd=None), "NULL buffer"),
    ]:
        scratch[:], dd[:], counter[:] = -7.0, -7.0, -1
        rc, text = call_window(**kw)
        assert rc == _ffi.SAI_ERR_ARG and message in text, (kw, rc, text)
        assert (scratch == -7.0).all() and (dd == -7.0).all() and counter[0] == -1  # a refused call writes nothing
    # no window: the counter is zeroed and nothing else is looked at; no site: every window is empty, DD is 0
    assert call_window(n_windows=0, lo=None, hi=None, scratch=None, dd=None, tr=None, tt=None)[0] == 0 and counter[0] == 0 and (dd == -7.0).all()
    assert call_window(n_sites=0, tr=None, tt=None, null_tiles=True)[0] == 0 and (dd == 0.0).all() and (scratch == 0.0).all()


def test_sources_binding_and_library_agree():
    """The group has no header under include/: its two units state the entry points, ``sai_amd/dd_table.py`` binds them."""
    import re

    from sai_amd import _binding, _build, _ffi, dd_table

    host = (_build.CSRC / "dd_table" / "dd_table_host.cpp").read_text()
    kernels = (_build.CSRC / "dd_table" / "dd_table.hip").read_text()
    defined = sorted(set(re.findall(r"^int (sai_[a-z0-9_]+)\(", host + kernels, flags=re.M)) - {n for n in re.findall(r"^int (sai_dd_\w*check\w*)\(", host, flags=re.M)})
    assert defined == sorted(dd_table.SIGNATURES) == ["sai_dd_table_abi_version", "sai_site_absdiff_table", "sai_site_absdiff_table_host",
                                                      "sai_window_dd_table", "sai_window_dd_table_host"]  # fmt: skip
    lib = dd_table.load()
    (version,) = re.findall(r"^#define SAI_DD_TABLE_ABI_VERSION (\d+)", host, flags=re.M)
    assert lib.sai_dd_table_abi_version() == dd_table.SAI_DD_TABLE_ABI_VERSION == int(version) == 1
    n_values = [int(v) for text in (host, kernels) for v in re.findall(r"^#define SAI_DD_TABLE_VALUES (\d+)", text, flags=re.M)]
    assert n_values == [8, 8] and dd_table.SAI_DD_TABLE_VALUES == 8 >= len(dd_table.DD_VALUES) == 7
    assert dd_table.DD_VALUES == D.DD_VALUES == (-2, -1, 0, 1, 2, 3, 4)
    assert set(dd_table.HOST_SYMBOLS) == {"sai_dd_table_abi_version", "sai_site_absdiff_table_host", "sai_window_dd_table_host"}
    assert dd_table.load_host() is not None
    assert lib.sai_site_absdiff_table(None, 1, None, 1, None, None, None) == _ffi.SAI_ERR_ARG and b"ctx is NULL" in lib.sai_last_error()
    assert lib.sai_window_dd_table(None, 1, None, 1, None, None, 1, None, 1, 0, None, None, None, None, None, None) == _ffi.SAI_ERR_ARG
    assert b"ctx is NULL" in lib.sai_last_error()
    assert lib.sai_abi_version() == _ffi.SAI_ABI_VERSION  # saihip.h is as it was
    assert "dd_table/dd_table.hip" in _build.UNITS and "dd_table/dd_table_host.cpp" in _build.HOST_UNITS
    # no family: no header, no binding module of the families' kind, nothing of its own to be stale against
    assert not (ROOT / "include" / "saihip_dd_table.h").exists() and dd_table not in _binding.family_modules()
    assert _build.own_inputs("dd_table/dd_table.hip") == [] and not list((_build.CSRC / "dd_table").glob("*.hpp"))
    assert "csrc/dd_table/*.hip" in abi_checks.package_data_patterns() and "csrc/dd_table/*.cpp" in abi_checks.package_data_patterns()
    # the sizes the cases are built from are the ones the sources state
    assert D.widen_rows() == 4096 and D.stage_sites(7) == 576 and D.stage_sites(8) == 512 and D.stage_sites(1) == 4096


@pytest.fixture(scope="module")
def dump_program(tmp_path_factory):
    """tests/native/dd_table_dump.cpp + the host units of libsaihip under ASan + UBSan, the runtimes linked in."""
    return native_build.dump_program("dd_table_dump", tmp_path_factory)["san"]


def clean(res):
    return res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr


def test_host_twins_are_clean_under_asan_ubsan(tmp_path, dump_program):
    """Both twins run (not only compiled) under the sanitizers as a program of its own, on buffers of exactly the size the
    header asks for: the numbers of the numpy statements."""
    for n_ind in (0, 1, 17, 250):
        for n_sites in (1, 64, 130):
            for kind, values in (("all", D.VALUE_LISTS[2]), ("listed", D.DD_VALUES)):
                g = D.genotypes(n_sites, n_ind, kind)
                (tmp_path / "tiles.bin").write_bytes(D.tile_numpy(g).tobytes())
                res = native_build.run_native(dump_program, ["table", n_sites, n_ind, tmp_path / "tiles.bin", ",".join(map(str, values))])
                assert clean(res), res.stderr[-3000:]
                got = np.array([[int(line[8 * s : 8 * s + 8], 16) for s in range(n_sites)] for line in res.stdout.splitlines()], dtype=np.int64)
                assert np.array_equal(got, D.table_numpy(values, g)), (n_ind, n_sites, kind)
    _, _, table_ref, table_tgt = D.window_block()
    (tmp_path / "ref.bin").write_bytes(table_ref.astype(np.uint32).tobytes())
    (tmp_path / "tgt.bin").write_bytes(table_tgt.astype(np.uint32).tobytes())
    (tmp_path / "win.bin").write_bytes(np.asarray(S.WINDOWS, dtype=np.int32).tobytes())
    for n_src, poke in ((1, False), (9, False), (129, False), (5, True)):
        src = D.window_source(n_src).copy()
        if poke:
            src[255, 4] = -128
        (tmp_path / "src.bin").write_bytes(D.tile_numpy(src).tobytes())
        res = native_build.run_native(dump_program, ["window", 256, n_src, tmp_path / "src.bin", ",".join(map(str, D.DD_VALUES)), tmp_path / "ref.bin",
                                                     S.N_REF, tmp_path / "tgt.bin", S.N_TGT, tmp_path / "win.bin"])  # fmt: skip
        assert clean(res), res.stderr[-3000:]
        lines = res.stdout.splitlines()
        unhex = lambda line: np.array([int(line[16 * i : 16 * i + 16], 16) for i in range(len(line) // 16)], dtype=np.uint64)  # noqa: E731
        d, dd, n_unlisted = host_window(src, D.DD_VALUES, table_ref, S.N_REF, table_tgt, S.N_TGT, S.WINDOWS)
        assert int(lines[0]) == n_unlisted and (n_unlisted > 0) == poke
        assert np.array_equal(unhex(lines[1]), dd.view(np.uint64))
        assert np.array_equal(np.stack([unhex(line) for line in lines[2:]]), d.view(np.uint64))
        if not poke:
            want_d, want_dd, _ = D.window_expected(n_src, S.WINDOWS)
            assert same_bits(dd, want_dd) and same_bits(d, want_d)
    res = native_build.run_native(dump_program, ["table", 3, 1, tmp_path / "missing.bin", "0"])
    assert res.returncode == 4
    (tmp_path / "one.bin").write_bytes(bytes(64))
    res = native_build.run_native(dump_program, ["table", 3, 1, tmp_path / "one.bin", "1,1"])
    assert res.returncode == 3 and "values must be distinct" in res.stderr and "Sanitizer" not in res.stderr


# ---- the route ----


def test_admission_rule():
    from sai_amd.dd_table import MIN_ROWS_DEFAULT, table_route_admitted

    assert MIN_ROWS_DEFAULT == 5
    env = {}
    assert table_route_admitted([2], 5, env) and table_route_admitted([1, 2, 2], 5, env) and table_route_admitted([1], 500, env)
    assert not table_route_admitted([2], 4, env)  # fewer rows than the default: they ride along or take the old route
    assert not table_route_admitted([3], 9, env) and not table_route_admitted([2, 4], 9, env) and not table_route_admitted([], 9, env)
    assert not table_route_admitted([2], 9, {"SAI_AMD_DD_TABLE": "0"})
    assert table_route_admitted([2], 9, {"SAI_AMD_DD_TABLE": "1"}) and table_route_admitted([2], 9, {"SAI_AMD_DD_TABLE": ""})
    assert table_route_admitted([2], 9, {"SAI_AMD_DD_TABLE_MIN_ROWS": "9"}) and not table_route_admitted([2], 8, {"SAI_AMD_DD_TABLE_MIN_ROWS": "9"})
    assert table_route_admitted([2], 1, {"SAI_AMD_DD_TABLE_MIN_ROWS": "1"})
    assert not table_route_admitted([2], 100, {"SAI_AMD_DD_TABLE_MIN_ROWS": "1", "SAI_AMD_DD_TABLE": "0"})
    with pytest.raises(ValueError, match="SAI_AMD_DD_TABLE_MIN_ROWS must be an integer"):
        table_route_admitted([2], 9, {"SAI_AMD_DD_TABLE_MIN_ROWS": "many"})


def test_the_environment_is_read_at_every_call(monkeypatch):
    from sai_amd.dd_table import table_route_admitted

    monkeypatch.delenv("SAI_AMD_DD_TABLE", raising=False)
    monkeypatch.delenv("SAI_AMD_DD_TABLE_MIN_ROWS", raising=False)
    assert table_route_admitted([2, 2], 6)
    monkeypatch.setenv("SAI_AMD_DD_TABLE", "0")
    assert not table_route_admitted([2, 2], 6)
    monkeypatch.setenv("SAI_AMD_DD_TABLE", "1")
    monkeypatch.setenv("SAI_AMD_DD_TABLE_MIN_ROWS", "7")
    assert not table_route_admitted([2, 2], 6) and table_route_admitted([2, 2], 7)


def test_combination_dd_on_a_stub_engine(monkeypatch):
    """One pair of tables per (ref, tgt) pair of blocks, one window call per source population, the old route for the
    population whose counter is not zero -- with every device step replaced by a recording stand-in."""
    import torch

    from sai_amd import dd_table

    log = []

    class Pop:
        def __init__(self, name, n_ind):
            self.name, self.n_ind, self.n_sites = name, n_ind, 10

    class Eng:
        def site_absdiff(self, pop, src):
            log.append(("absdiff", pop.name, src.name))
            return (pop.name, src.name)

        def window_dd(self, ad_ref, n_ref, ad_tgt, n_tgt, lo, hi):
            log.append(("window_dd", ad_ref, n_ref, ad_tgt, n_tgt))
            return torch.full((2,), -1.0, dtype=torch.float64)

    def fake_table(eng, pop, values=dd_table.DD_VALUES):
        log.append(("table", pop.name))
        return "T" + pop.name

    def fake_window(eng, src, table_ref, n_ref, table_tgt, n_tgt, lo, hi, values=dd_table.DD_VALUES):
        log.append(("window", src.name, table_ref, n_ref, table_tgt, n_tgt))
        return torch.full((2,), float(src.n_ind), dtype=torch.float64), torch.tensor([3 if src.name == "bad" else 0], dtype=torch.int32)

    monkeypatch.setattr(dd_table, "site_absdiff_table", fake_table)
    monkeypatch.setattr(dd_table, "window_dd_table", fake_window)
    dd_table.reset_calls()
    ref, tgt, other = Pop("ref", 7), Pop("tgt", 3), Pop("tgt2", 4)
    a, bad, b = Pop("a", 5), Pop("bad", 8), Pop("b", 9)
    pair = dd_table.TablePair()
    got = dd_table.combination_dd(Eng(), pair, ref, tgt, [a, bad, b], None, None)
    assert got.tolist() == [[5.0, -1.0, 9.0]] * 2
    assert log == [("table", "ref"), ("table", "tgt"), ("window", "a", "Tref", 7, "Ttgt", 3), ("window", "bad", "Tref", 7, "Ttgt", 3),
                   ("window", "b", "Tref", 7, "Ttgt", 3), ("absdiff", "ref", "bad"), ("absdiff", "tgt", "bad"),
                   ("window_dd", ("ref", "bad"), 7, ("tgt", "bad"), 3)]  # fmt: skip
    assert dd_table.CALLS["old_route"] == 1
    del log[:]
    dd_table.combination_dd(Eng(), pair, ref, tgt, [b], None, None)  # the same pair: its tables are kept
    assert log == [("window", "b", "Tref", 7, "Ttgt", 3)]
    del log[:]
    dd_table.combination_dd(Eng(), pair, ref, other, [b], None, None)  # another pair: both are made again
    assert log == [("table", "ref"), ("table", "tgt2"), ("window", "b", "Tref", 7, "Ttgt2", 4)]
    dd_table.reset_calls()
    assert set(dd_table.CALLS.values()) == {0}
