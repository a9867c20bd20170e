"""Sources from a file of their own, without a GPU: ``sai_site_join_host`` of include/saihip_join.h on every shared case,
the family's header against its binding, the argument errors, the join under ASan + UBSan in a stand-alone program, every
refusal of ``read_dosage_data(..., src_file=)``, its blocks for every format the source file may have against the one
VCF of the common sites, and the host ``WindowGenerator`` over two inputs window by window."""

import ctypes as C

import numpy as np
import pytest

import abi_checks
import native_build
import site_join_cases as K

BLOCK, CAP = 256, 2  # lengths around 256 rows, and one of 7 x 256


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return K.write_inputs(tmp_path_factory.mktemp("two_inputs"))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_header_binding_and_constants_agree():
    from sai_amd import _ffi_join as J

    names = abi_checks.declared_names("saihip_join.h")
    assert names == sorted(J.SIGNATURES) == ["sai_join_abi_version", "sai_site_join_host"] == sorted(J.HOST_SYMBOLS)
    for constant in ("SAI_JOIN_ABI_VERSION", "SAI_JOIN_INFO_WORDS"):
        assert abi_checks.header_macro("saihip_join.h", constant) == getattr(J, constant)
    lib = J.load()
    assert lib.sai_join_abi_version() == J.SAI_JOIN_ABI_VERSION == 1 and all(hasattr(lib, n) for n in names)


def test_the_familys_unit_is_stale_against_its_own_header():
    """The family's header is read by its one unit only: that unit is rebuilt when it changes, no other unit is, and
    nothing under include/ or csrc is outside both lists."""
    from sai_amd import _build

    own = [_build.INCLUDE / "saihip_join.h"]
    assert _build.own_inputs("join/site_join_host.cpp") == own
    assert all(_build.own_inputs(u) == [] for u in _build.UNITS if not u.startswith("join/"))
    common = _build.staleness_inputs()
    assert not set(own) & set(common)
    assert sorted([*common, *own]) == sorted([*_build.PUBLIC_HEADERS, *_build.CSRC.rglob("*.hpp")])
    including = {str(p.relative_to(_build.CSRC)) for ext in ("hip", "cpp", "hpp") for p in _build.CSRC.rglob(f"*.{ext}")
                 if "saihip_join.h" in p.read_text()}
    assert including == {"join/site_join_host.cpp"}


@pytest.mark.parametrize("name,a,b", K.join_cases(BLOCK, CAP), ids=lambda v: v if isinstance(v, str) else "")
def test_join_twin_equals_intersect1d(name, a, b):
    from sai_amd import site_join

    rows_a, rows_b, info = site_join.join_host(a, b)
    want_a, want_b, want_info = K.expected_join(a, b)
    assert info.tolist() == want_info.tolist()
    assert np.array_equal(rows_a, want_a) and np.array_equal(rows_b, want_b) and rows_a.dtype == np.int32


@pytest.mark.parametrize("name,a,b,bad_a,bad_b", K.disordered_cases(BLOCK), ids=lambda v: v if isinstance(v, str) else "")
def test_join_twin_names_the_first_position_out_of_order(name, a, b, bad_a, bad_b):
    from sai_amd import site_join

    rows_a, rows_b, info = site_join.join_host(a, b)
    assert info.tolist() == [0, bad_a, bad_b, 0] and rows_a.size == 0 == rows_b.size


def test_argument_errors():
    from sai_amd import _ffi, _ffi_join

    lib = _ffi_join.load_host()
    a = np.array([1, 2, 3], dtype=np.int32)
    rows, info = np.zeros(3, dtype=np.int32), np.zeros(4, dtype=np.int64)
    join = lib.sai_site_join_host
    for args, words in (((ptr(a), -1, ptr(a), 3, ptr(rows), ptr(rows), ptr(info)), b"n_a and n_b must be 0..2^31 - 2"),
                        ((ptr(a), 3, ptr(a), 2**31 - 1, ptr(rows), ptr(rows), ptr(info)), b"n_a and n_b must be 0..2^31 - 2"),
                        ((ptr(a), 3, ptr(a), 3, ptr(rows), ptr(rows), None), b"info is NULL"),
                        ((None, 3, ptr(a), 3, ptr(rows), ptr(rows), ptr(info)), b"NULL buffer"),
                        ((ptr(a), 3, None, 3, ptr(rows), ptr(rows), ptr(info)), b"NULL buffer"),
                        ((ptr(a), 3, ptr(a), 3, None, ptr(rows), ptr(info)), b"NULL buffer"),
                        ((ptr(a), 3, ptr(a), 3, ptr(rows), None, ptr(info)), b"NULL buffer")):  # fmt: skip
        assert join(*args) == _ffi.SAI_ERR_ARG and lib.sai_last_error() == words
    assert join(None, 0, None, 0, None, None, ptr(info)) == 0 and info.tolist() == [0, -1, -1, 1]  # an empty side needs no buffer
    assert join(ptr(a), 3, None, 0, None, None, ptr(info)) == 0 and info.tolist() == [0, -1, -1, 0]


def test_the_join_is_clean_under_asan_ubsan(tmp_path_factory):
    exe = native_build.dump_program("site_join_dump", tmp_path_factory)["san"]
    res = native_build.run_native(exe, [])
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout[-2000:] + res.stderr[-3000:]
    assert int(res.stdout.split()[1]) > 90


# -- the readers ---------------------------------------------------------------------------------------------------------


def groups_of(results):
    return {(g, p): (cd.POS, np.asarray(cd.GT)) for g in ("ref", "tgt", "src", "outgroup") for p, cd in ((results[g][0] or {}).items())}


@pytest.fixture(scope="module")
def expected(inputs):
    from sai_amd.configs import GlobalConfig  # noqa: F401
    from sai_amd.sai import load_config
    from sai_amd.utils.read_data import read_dosage_data

    cfg = load_config(str(K.CONFIG))
    files = {g: cfg.populations.get_population(g) for g in ("ref", "tgt", "src", "outgroup")}
    read = lambda vcf, **kw: read_dosage_data(vcf, "1", cfg.ploidies, files["ref"], files["tgt"], files["src"], files["outgroup"],  # noqa: E731
                                              inputs["anc"], **kw)
    return read, groups_of(read(inputs["common"])), groups_of(read(inputs["common"], start=5000, end=30000))


def test_refusals(inputs, expected, tmp_path, monkeypatch):
    from sai_amd.sai import load_config
    from sai_amd.utils.read_data import read_dosage_data

    monkeypatch.chdir(K.ROOT)
    read, _, _ = expected
    source = K.write_source(inputs, "vcf", tmp_path)
    cfg = load_config(str(K.CONFIG))
    files = [cfg.populations.get_population(g) for g in ("ref", "tgt", "src", "outgroup")]
    with pytest.raises(ValueError, match=r"requires `anc_allele_file`: the two inputs are reconciled through the ancestral allele.*follow-up"):
        read_dosage_data(inputs["panel"], "1", cfg.ploidies, *files, None, src_file=source)
    # a position that repeats in the source file, one that descends in the panel: the file and the position are named
    lines = open(source).read().splitlines()
    repeated = tmp_path / "repeated.vcf"
    at = next(i for i, ln in enumerate(lines) if not ln.startswith("#")) + 5
    fields = lines[at].split("\t")
    fields[1] = lines[at - 1].split("\t")[1]
    repeated.write_text("\n".join(lines[:at] + ["\t".join(fields)] + lines[at + 1 :]) + "\n")
    with pytest.raises(ValueError, match=rf"repeated\.vcf: position {fields[1]} repeats or does not ascend \(after {fields[1]}\)"):
        read(inputs["panel"], src_file=str(repeated))
    lines = open(inputs["panel"]).read().splitlines()
    at = next(i for i, ln in enumerate(lines) if not ln.startswith("#")) + 9
    lines[at], lines[at + 1] = lines[at + 1], lines[at]
    descending = tmp_path / "descending.vcf"
    descending.write_text("\n".join(lines) + "\n")
    lower, upper = lines[at + 1].split("\t")[1], lines[at].split("\t")[1]
    with pytest.raises(ValueError, match=rf"descending\.vcf: position {lower} repeats or does not ascend \(after {upper}\)"):
        read(str(descending), src_file=source)
    # a src sample the source file does not hold: the reader's words, about the source file
    with pytest.raises(ValueError, match=r"Failed to read VCF file .*panel\.vcf from 1.*src_i1"):
        read(inputs["common"], src_file=inputs["panel"])


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_host_route_equals_the_one_vcf_of_the_common_sites(inputs, expected, tmp_path, fmt, monkeypatch):
    monkeypatch.chdir(K.ROOT)
    read, whole, region = expected
    source = K.write_source(inputs, fmt, tmp_path)
    for want, kw in ((whole, {}), (region, dict(start=5000, end=30000))):
        got = read(inputs["panel"], src_file=source, **kw)
        summary = got["site_join"]
        assert set(groups_of(got)) == set(want) == {("ref", "ref"), ("tgt", "tgt"), ("src", "src"), ("outgroup", "out")}
        for key, (pos, gt) in groups_of(got).items():
            assert np.array_equal(pos, want[key][0]) and np.array_equal(gt, want[key][1]) and gt.dtype == want[key][1].dtype, key
        assert summary["n_common"] == want[("ref", "ref")][0].size and not summary["panel_identity"] and not summary["source_identity"]
    assert whole[("ref", "ref")][0].size == inputs["n_common"] < inputs["n_fixture"]
    if fmt in ("bed", "geno-text"):  # the bare prefix names the same fileset
        bare = read(inputs["panel"], src_file=source.rsplit(".", 1)[0])
        assert np.array_equal(groups_of(bare)[("src", "src")][1], whole[("src", "src")][1])


def test_host_route_identity_same_file_and_no_common_site(inputs, expected, tmp_path, monkeypatch):
    monkeypatch.chdir(K.ROOT)
    read, whole, _ = expected
    same = read(inputs["common"], src_file=inputs["common"])  # the main input as its own source file: the one-input result
    assert same["site_join"]["panel_identity"] and same["site_join"]["source_identity"]
    for key, (pos, gt) in groups_of(same).items():
        assert np.array_equal(pos, whole[key][0]) and np.array_equal(gt, whole[key][1])
    full = K.write_inputs(tmp_path, complete=True)  # the source file covers every panel site and has sites of its own
    got = read(full["panel"], src_file=K.write_source(full, "vcf", tmp_path))
    assert got["site_join"]["panel_identity"] and not got["site_join"]["source_identity"] and got["site_join"]["n_common"] == full["n_fixture"]
    # no common site: as a region without a record
    source = K.write_source(inputs, "vcf", tmp_path)
    lines = [ln for ln in open(source).read().splitlines()]
    own = [ln for ln in lines if ln.startswith("#") or ln.split("\t")[1] in ("60", "7001", "30001", "39995")]
    (tmp_path / "apart.vcf").write_text("\n".join(own) + "\n")
    apart = read(inputs["panel"], src_file=str(tmp_path / "apart.vcf"))
    empty = read(inputs["common"], start=39900, end=39910)
    assert apart["site_join"]["n_common"] == 0
    assert {g: apart[g] for g in ("ref", "tgt", "src", "outgroup")} == {g: empty[g] for g in ("ref", "tgt", "src", "outgroup")}
    assert all(apart[g][0] is None and apart[g][1] for g in ("ref", "tgt", "src", "outgroup"))


def test_window_generator_over_two_inputs_yields_the_windows_of_the_one_vcf(inputs, tmp_path, monkeypatch):
    """The host generator (what the plug-in classes iterate): every window's positions and matrices, for a source file
    in another format than the panel's; the resident form refuses a second input."""
    from sai_amd.generators import WindowGenerator
    from sai_amd.sai import load_config

    monkeypatch.chdir(K.ROOT)
    cfg = load_config(str(K.CONFIG))
    files = {g: cfg.populations.get_population(g) for g in ("ref", "tgt", "src", "outgroup")}
    kw = dict(chr_name="1", ref_ind_file=files["ref"], tgt_ind_file=files["tgt"], src_ind_file=files["src"], out_ind_file=files["outgroup"],
              win_len=8000, win_step=4000, ploidy_config=cfg.ploidies, anc_allele_file=inputs["anc"], start=1, end=40000)  # fmt: skip
    source = K.write_source(inputs, "geno-packed", tmp_path)
    want = list(WindowGenerator(vcf_file=inputs["common"], **kw).get())
    got = list(WindowGenerator(vcf_file=inputs["panel"], src_file=source, **kw).get())
    assert len(got) == len(want) > 5 and sum(len(w["pos"]) for w in want) > inputs["n_common"]  # the windows overlap
    for a, b in zip(got, want):
        assert (a["start"], a["end"], a["ref_pop"], a["tgt_pop"], a["src_pop_list"], a["out_pop"]) == (b["start"], b["end"], b["ref_pop"], b["tgt_pop"], b["src_pop_list"], b["out_pop"])
        assert np.array_equal(a["pos"], b["pos"])
        for key in ("ref_gts", "tgt_gts", "out_gts"):
            assert (a[key] is None and b[key] is None) or np.array_equal(a[key], b[key]), key
        assert (a["src_gts_list"] is None and b["src_gts_list"] is None) or all(np.array_equal(x, y) for x, y in zip(a["src_gts_list"], b["src_gts_list"]))
    with pytest.raises(ValueError, match="joined over host matrices only"):
        WindowGenerator(vcf_file=inputs["panel"], src_file=source, resident=True, **kw)
