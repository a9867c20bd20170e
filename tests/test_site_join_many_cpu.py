"""Sources from several files of their own, without a GPU: ``sai_site_join_many_host``
(sai_amd/csrc/join/site_join_many_host.cpp) against ``functools.reduce(np.intersect1d, ...)`` for 2 to 5 lists, against
``sai_site_join_host`` for two, with a list out of order at every place, its argument errors, and under ASan + UBSan in a
stand-alone program; the bindings, versions and the units' places in the build; ``input_samples`` for every format; every
refusal of ``score(..., src_file=[...])`` before the output directory is made; ``--src-input`` given more than once, from
the parser down to the ranks' command line; and ``read_dosage_data(..., src_file=[...])`` and the host ``WindowGenerator``
against the one VCF of the common sites."""

import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import native_build
import site_join_cases as K
import site_join_many_cases as M

BLOCK, CAP = 256, 2  # lengths around 256 rows, and one of 7 x 256


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("many_inputs")
    out = M.write_inputs(tmp)
    out["paths"] = {cut: M.write_sources(out, cut, tmp) for cut in M.CUTS}
    out["tmp"] = tmp
    return out


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# -- sai_site_join_many_host -----------------------------------------------------------------------------------------------


def many_cases():
    """(name, lists) for k = 2 .. 5, built from the pairs of ``join_cases``: the pair itself, the pair with further lists
    drawn around it, and an empty list at each place."""
    rng = np.random.default_rng(20261021)
    cases = []
    for name, a, b in K.join_cases(BLOCK, CAP):
        cases.append((f"2: {name}", [a, b]))
        pool = np.union1d(a, b).astype(np.int32)
        for k in (3, 4, 5):
            more = [pool[rng.random(pool.size) < 0.8] for _ in range(k - 2)]
            at = k % 3  # where the pair stands among the lists differs with k
            lists = more[:at] + [a, b] + more[at:]
            cases.append((f"{k}: {name}", lists))
    some = K.ascending(rng, 300, 5000)
    for k in (2, 3, 4, 5):
        for at in range(k):
            cases.append((f"{k}: empty at {at}", [some[:0] if j == at else some[j::2] for j in range(k)]))
        cases.append((f"{k}: identical", [some.copy() for _ in range(k)]))
        cases.append((f"{k}: disjoint", [some[j::k] for j in range(k)]))
        cases.append((f"{k}: subsets of the first", [some] + [some[j :: j + 2] for j in range(k - 1)]))
        cases.append((f"{k}: single entries", [some[7:8]] * (k - 1) + [some]))
        cases.append((f"{k}: up to the top", [np.array([1, 5, K.TOP - 2, K.TOP - 1, K.TOP], dtype=np.int32)] * (k - 1) + [np.array([5, K.TOP - 3, K.TOP - 1, K.TOP], dtype=np.int32)]))  # fmt: skip
    return cases


@pytest.mark.parametrize("name,lists", many_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_join_equals_reduce_intersect1d(name, lists):
    from sai_amd import site_join, site_join_many

    rows, info = site_join_many.join_many_host(lists)
    k = len(lists)
    common = functools.reduce(np.intersect1d, lists)
    empty = any(pos.size == 0 for pos in lists)
    identity = [pos.size == 0 if empty else common.size == pos.size for pos in lists]
    assert info.tolist() == [common.size, -1, *([-1] * k), *map(int, identity)]
    for pos, r in zip(lists, rows):
        assert r.dtype == np.int32 and r.size == common.size and np.array_equal(pos[r], common)
    if k == 2:  # word for word the two-list join's rows
        rows_a, rows_b, info2 = site_join.join_host(*lists)
        assert np.array_equal(rows[0], rows_a) and np.array_equal(rows[1], rows_b) and info[0] == info2[0]


@pytest.mark.parametrize("k", (2, 3, 5))
def test_join_names_the_first_list_and_position_out_of_order(k):
    from sai_amd import site_join_many

    for name, a, b, bad_a, bad_b in K.disordered_cases(BLOCK):
        bad, at = (a, bad_a) if bad_a != -1 else (b, bad_b)
        good = b if bad_a != -1 and bad_b == -1 else a
        if bad_a != -1 and bad_b != -1:
            continue
        for place in range(k):
            lists = [bad if j == place else good for j in range(k)]
            rows, info = site_join_many.join_many_host(lists)
            assert info.tolist() == [0, place, *(at if j == place else -1 for j in range(k)), *([0] * k)], (name, place)
            assert all(r.size == 0 for r in rows)
    # two lists out of order: the first one is named, every list has its own index; nothing is written
    _, twice, _, at, _ = K.disordered_cases(BLOCK)[-1]
    lib = site_join_many.load_host()
    lists = [twice if j else K.disordered_cases(BLOCK)[0][2] for j in range(k)]
    rows = [np.full(lists[0].size, 77, dtype=np.int32) for _ in range(k)]
    info = np.zeros(2 + 2 * k, dtype=np.int64)
    sizes = np.array([pos.size for pos in lists], dtype=np.int64)
    table = lambda arrays: (C.c_void_p * k)(*[x.ctypes.data for x in arrays])  # noqa: E731
    assert lib.sai_site_join_many_host(k, table(lists), ptr(sizes), table(rows), ptr(info)) == 0
    assert info.tolist() == [0, 1, -1, *([at] * (k - 1)), *([0] * k)] and all((r == 77).all() for r in rows)


def test_join_argument_errors():
    from sai_amd import _ffi, site_join_many

    lib = site_join_many.load_host()
    a = np.array([1, 2, 3], dtype=np.int32)
    rows, info = np.zeros(3, dtype=np.int32), np.zeros(2 + 2 * 17, dtype=np.int64)
    table = lambda *arrays: (C.c_void_p * 18)(*[None if x is None else x.ctypes.data for x in arrays])  # noqa: E731
    sizes = lambda *n: ptr(np.array(n + (3,) * (18 - len(n)), dtype=np.int64))  # noqa: E731
    join = lib.sai_site_join_many_host
    for args, words in (((1, table(a, a), sizes(3, 3), table(rows, rows), ptr(info)), b"n_lists must be 2..17"),
                        ((18, table(*[a] * 18), sizes(), table(*[rows] * 18), ptr(info)), b"n_lists must be 2..17"),
                        ((2, table(a, a), sizes(3, 3), table(rows, rows), None), b"info is NULL"),
                        ((2, table(a, a), None, table(rows, rows), ptr(info)), b"NULL buffer"),
                        ((2, table(a, a), sizes(-1, 3), table(rows, rows), ptr(info)), b"the length of a list must be 0..2^31 - 2"),
                        ((2, table(a, a), sizes(3, 2**31 - 1), table(rows, rows), ptr(info)), b"the length of a list must be 0..2^31 - 2"),
                        ((2, None, sizes(3, 3), table(rows, rows), ptr(info)), b"NULL buffer"),
                        ((2, table(a, a), sizes(3, 3), None, ptr(info)), b"NULL buffer"),
                        ((3, table(a, None, a), sizes(3, 3, 3), table(rows, rows, rows), ptr(info)), b"NULL buffer"),
                        ((3, table(a, a, a), sizes(3, 3, 3), table(rows, rows, None), ptr(info)), b"NULL buffer")):  # fmt: skip
        assert join(*args) == _ffi.SAI_ERR_ARG and lib.sai_last_error() == words, words
    # an empty list needs no buffer, and nothing is read
    assert join(3, None, sizes(3, 0, 3), None, ptr(info)) == 0 and info[:8].tolist() == [0, -1, -1, -1, -1, 0, 1, 0]
    assert join(17, table(*[a] * 17), sizes(), table(*[rows] * 17), ptr(info)) == 0 and info.tolist() == [3, -1, *([-1] * 17), *([1] * 17)]


def test_the_join_is_clean_under_asan_ubsan(tmp_path_factory):
    exe = native_build.dump_program("site_join_many_dump", tmp_path_factory)["san"]
    res = native_build.run_native(exe, [])
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout[-2000:] + res.stderr[-3000:]
    assert int(res.stdout.split()[1]) > 400


def test_bindings_versions_and_units():
    from sai_amd import _build, _ffi, site_join_many, site_join_parts

    assert sorted(site_join_many.SIGNATURES) == ["sai_join_many_abi_version", "sai_site_join_many_host"] == sorted(site_join_many.HOST_SYMBOLS)
    assert sorted(site_join_parts.SIGNATURES) == ["sai_tile_parts_abi_version", "sai_tile_rows_from_parts"]
    assert site_join_parts.HOST_SYMBOLS == ("sai_tile_parts_abi_version",)
    lib = site_join_many.load()
    assert lib.sai_join_many_abi_version() == site_join_many.SAI_JOIN_MANY_ABI_VERSION == 1
    lib = site_join_parts.load()
    assert lib.sai_tile_parts_abi_version() == site_join_parts.SAI_TILE_PARTS_ABI_VERSION == 1 and site_join_parts.SAI_TILE_MAX_PARTS == 16
    assert C.sizeof(site_join_parts.TilePart) == 40
    device = _build.UNITS[: -len(_build.HOST_UNITS)]
    assert device[-2:] == ["join/tile_parts.hip", "join/tile_rows.hip"] and "join/tile_parts.hip" not in _build.HOST_UNITS
    assert _build.HOST_UNITS[-2:] == ["join/site_join_host.cpp", "join/site_join_many_host.cpp"]
    assert _build.own_inputs("join/site_join_many_host.cpp") == _build.own_inputs("join/site_join_host.cpp")
    # the existing headers and version numbers are what they were
    from sai_amd import _ffi_join, site_join_device

    assert (_ffi_join.SAI_JOIN_ABI_VERSION, _ffi_join.SAI_JOIN_INFO_WORDS, site_join_device.SAI_JOIN_DEVICE_ABI_VERSION) == (1, 4, 1)
    # the context is looked at before any other argument: the other argument errors are checked where there is a GPU
    assert lib.sai_tile_rows_from_parts(None, 0, None, -1, -1, None, None, None) == _ffi.SAI_ERR_ARG and lib.sai_last_error() == b"ctx is NULL"


# -- which sample comes from which file ------------------------------------------------------------------------------------


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_input_samples_of_every_format(tmp_path, fmt):
    from sai_amd.utils.filesets import input_samples

    one = K.write_inputs(tmp_path)
    assert input_samples(K.write_source(one, fmt, tmp_path)) == ["src_i1"]
    if fmt == "vcf":
        names = input_samples(one["panel"])
        assert len(names) == 1512 and "src_i1" not in names and names[:2] == ["src_i2", "tgt_i1"] and input_samples(str(K.FIXTURE))[0] == "src_i1"


def test_input_samples_of_several_samples_and_a_psam_with_a_header(inputs, tmp_path):
    from sai_amd.utils.filesets import input_samples

    for cut, files in M.CUTS.items():
        assert [input_samples(p) for p in inputs["paths"][cut]] == [names for _, names in files]
    import pgen_builder

    prefix = str(tmp_path / "two")
    pgen_builder.write_fileset(prefix, ["1"], [5], ["v0"], ["A"], ["T"], np.array([[0, 1]], dtype=np.uint8), ["x1", "x2"])
    assert input_samples(prefix + ".pgen") == ["x1", "x2"]
    open(prefix + ".psam", "w").write("#FID\tIID\tSEX\nf\tx1\t0\nf\tx2\t0\n")
    assert input_samples(prefix + ".pgen") == ["x1", "x2"]
    open(prefix + ".psam", "w").write("#IID\tSEX\nx1\t0\nx2\t0\n")
    assert input_samples(prefix + ".pgen") == ["x1", "x2"]


def _no_rank_environment(monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SAI_AMD_INGEST", "SAI_AMD_LAYOUT"):
        monkeypatch.delenv(name, raising=False)


def test_score_refusals_come_before_the_output_directory(inputs, tmp_path, monkeypatch):
    import re

    from sai_amd import sai as sai_mod

    _no_rank_environment(monkeypatch)
    monkeypatch.chdir(K.ROOT)
    a, b, c = inputs["paths"][3]
    out = tmp_path / "made_by_score" / "s.tsv"
    ask = dict(vcf_file=inputs["panel"], chr_name="1", win_len=8000, win_step=4000, output_file=str(out), config=inputs["config"])
    score = lambda files, anc=inputs["anc"], workers=1, **kw: sai_mod.score(anc_allele_file=anc, num_workers=workers, src_file=files, **ask, **kw)  # noqa: E731
    unrelated = K.write_source(K.write_inputs(tmp_path), "vcf", tmp_path)  # holds src_i1 only
    for files, words in (
        ([a, b], rf"^source sample tgt_i502 is held by none of the source files: {re.escape(a)}, {re.escape(b)}$"),
        ([a, b, c, unrelated], rf"^source sample src_i1 is held by two source files, {re.escape(a)} and {re.escape(unrelated)}: it must come from exactly one\.$"),
        ([a, b, c, inputs["panel"]], rf"^source file {re.escape(inputs['panel'])} holds no sample of the src list: it would only remove sites\. Leave it out\.$"),
        ([a, b, c, b], rf"^`src_file` names {re.escape(b)} twice: every source file is read and joined once\.$"),
        ([a, b, c] + [str(tmp_path / f"further_{k}.vcf") for k in range(14)], r"^`src_file` names 17 source files; at most 16 are joined in one run\.$"),
        ([], r"^`src_file` is an empty sequence"),
    ):  # fmt: skip
        for workers in (1, 2):
            with pytest.raises(ValueError, match=words):
                score(files, workers=workers)
            assert not out.parent.exists()
    # every existing refusal applies to every file, in its existing words
    with pytest.raises(ValueError, match=r"requires `anc_allele_file`: the two inputs are reconciled through the ancestral allele.*follow-up"):
        score([a, b, c], anc=None)
    for workers in (1, 2):
        with pytest.raises(ValueError, match=r"^a source file of its own is read in the int8 layout"):
            score([a, b, c], workers=workers, layout="packed2")
        for files in ([str(tmp_path / "no_such.vcf"), b, c], [a, b, str(tmp_path / "no_such.vcf")]):
            with pytest.raises(ValueError, match=r"^cannot open VCF .*no_such\.vcf$"):
                score(files, workers=workers)
        assert not out.parent.exists()
    # the readers refuse the same, before they read
    from sai_amd.generators import WindowGenerator
    from sai_amd.utils.read_data import read_data_device, read_dosage_data

    cfg, lists = M.reader_arguments(inputs)
    for read in (lambda **kw: read_dosage_data(inputs["panel"], "1", cfg.ploidies, *lists, **kw),
                 lambda **kw: read_data_device(None, inputs["panel"], "1", cfg.ploidies, *lists, **kw)):  # fmt: skip
        with pytest.raises(ValueError, match=r"requires `anc_allele_file`"):
            read(anc_allele_file=None, src_file=[a, b, c])
        with pytest.raises(ValueError, match=r"held by none of the source files"):
            read(anc_allele_file=inputs["anc"], src_file=[a, b])
        with pytest.raises(ValueError, match=r"names .* twice"):
            read(anc_allele_file=inputs["anc"], src_file=[a, b, a])
    with pytest.raises(ValueError, match=r"^a source file of its own is read in the int8 layout"):
        read_data_device(None, inputs["panel"], "1", cfg.ploidies, *lists, inputs["anc"], layout="packed2", src_file=[a, b, c])
    with pytest.raises(ValueError, match="joined over host matrices only"):
        WindowGenerator(vcf_file=inputs["panel"], src_file=[a, b, c], resident=True, chr_name="1", ref_ind_file=lists[0], tgt_ind_file=lists[1],
                        src_ind_file=lists[2], out_ind_file=lists[3], win_len=8000, win_step=4000, ploidy_config=cfg.ploidies,
                        anc_allele_file=inputs["anc"], start=1, end=40000)  # fmt: skip


# -- the flag, from the parser down to the ranks ---------------------------------------------------------------------------


def _parse(argv):
    import argparse

    from sai_amd.parsers.score_parser import add_score_parser

    top = argparse.ArgumentParser()
    add_score_parser(top.add_subparsers())
    return top.parse_args(argv)


def test_src_input_may_be_given_more_than_once(inputs, tmp_path, monkeypatch):
    from sai_amd import distributed, launcher
    from sai_amd import sai as sai_mod
    from sai_amd.parsers import score_parser
    from sai_amd.preprocessors import ChunkPreprocessor

    _no_rank_environment(monkeypatch)
    monkeypatch.chdir(K.ROOT)
    a, b, c = inputs["paths"][3]
    base = ["score", "--vcf", inputs["panel"], "--chr-name", "1", "--anc-alleles", inputs["anc"], "--output", str(tmp_path / "o.tsv"),
            "--config", inputs["config"], "--num-workers", "1"]  # fmt: skip
    assert _parse(base).src_input is None
    assert _parse(base + ["--src-input", a]).src_input == a  # one occurrence: the str, as before
    assert _parse(base + ["--src-input", a, "--src-input", b]).src_input == [a, b]
    assert _parse(["score", "--src-input", c] + base[1:] + ["--src-input", a, "--src-input", b]).src_input == [c, a, b]  # command-line order
    with pytest.raises(SystemExit):
        _parse(base + ["--src-input", a, "--src-input", str(tmp_path / "missing.vcf")])
    seen = []
    monkeypatch.setattr(score_parser, "score", lambda **kw: seen.append(kw))
    for flags in ([], ["--src-input", a], ["--src-input", a, "--src-input", b, "--src-input", c]):
        args = _parse(base + flags)
        args.runner(args)
    assert "src_file" not in seen[0] and seen[1]["src_file"] == a and seen[2]["src_file"] == [a, b, c]
    assert {k: v for k, v in seen[2].items() if k != "src_file"} == seen[0]
    res = subprocess.run([sys.executable, "-m", "sai_amd", "score", "--help"], cwd=str(K.ROOT), capture_output=True, text=True, timeout=600)
    helptext = " ".join(res.stdout.split())
    assert "--src-input PATH" in helptext and "Requires --anc-alleles" in helptext and "int8 layout" in helptext
    assert "May be given up to 16 times, once per source file" in helptext

    # the command line of the ranks repeats the flag, and the parser takes it back
    plain = sai_mod._score_cli_arguments(inputs["panel"], "1", 10, 5, inputs["anc"], "o.tsv", inputs["config"], 2)
    many = sai_mod._score_cli_arguments(inputs["panel"], "1", 10, 5, inputs["anc"], "o.tsv", inputs["config"], 2, src_file=[a, b, c])
    assert many == plain + ["--src-input", a, "--src-input", b, "--src-input", c]
    assert _parse(many).src_input == [a, b, c]

    # score(num_workers=2) hands the list to the launcher, a rank hands it to the sharded route; a sequence of one path is that path
    launched, sharded = [], []
    monkeypatch.setattr(launcher, "launch_ranks", lambda n, argv, **kw: launched.append(argv) or 0)
    ask = dict(vcf_file=inputs["panel"], chr_name="1", win_len=10, win_step=5, anc_allele_file=inputs["anc"], output_file="o.tsv",
               config=inputs["config"], num_workers=2)  # fmt: skip
    sai_mod.score(**ask, src_file=(a, b, c))
    sai_mod.score(**ask, src_file=[a])
    sai_mod.score(**ask, src_file=a)
    assert launched[0] == many and launched[1] == launched[2] == plain + ["--src-input", a]
    monkeypatch.setattr(distributed, "score_sharded", lambda *x, **kw: sharded.append((x, kw)))
    monkeypatch.setattr(distributed, "shutdown_process_group", lambda: None)
    monkeypatch.setattr(launcher, "in_rank_job", lambda: True)
    sai_mod.score(**ask, src_file=[a, b, c])
    assert sharded[0][1]["src_file"] == [a, b, c]

    # the driver keeps the list for the readers
    monkeypatch.undo()
    monkeypatch.chdir(K.ROOT)
    cfg = sai_mod.load_config(inputs["config"])
    driver = sai_mod.chunk_preprocessor_for(cfg, inputs["panel"], 8000, 4000, str(tmp_path / "o.tsv"), inputs["anc"], src_file=[a, b, c])
    assert isinstance(driver, ChunkPreprocessor) and driver.src_file == [a, b, c] and driver._second_input() == {"src_file": [a, b, c]}


def test_score_sharded_hands_the_list_to_the_chunk_driver(inputs, tmp_path, monkeypatch):
    from sai_amd import distributed
    from sai_amd import sai as sai_mod

    _no_rank_environment(monkeypatch)
    monkeypatch.chdir(K.ROOT)
    made, ran = [], []
    monkeypatch.setattr(distributed, "init_process_group", lambda *x, **kw: (0, 1))
    monkeypatch.setattr(sai_mod, "chunk_preprocessor_for", lambda *x, **kw: made.append((x, kw)) or "driver")
    monkeypatch.setattr(sai_mod, "write_headers", lambda *x, **kw: None)
    monkeypatch.setattr(distributed, "run_sharded", lambda driver, generator, **kw: ran.append(driver) or "batches")
    ask = (inputs["panel"], "1", 8000, 4000, inputs["anc"], str(tmp_path / "o.tsv"), inputs["config"])
    assert distributed.score_sharded(*ask, src_file=list(inputs["paths"][3])) == "batches"
    assert distributed.score_sharded(*ask) == "batches"
    assert made[0][0] == made[1][0] and made[0][1] == {**made[1][1], "src_file": inputs["paths"][3]} and "src_file" not in made[1][1]
    assert ran == ["driver", "driver"]


def test_the_memory_estimate_adds_every_source_file(inputs, monkeypatch):
    from sai_amd import sai as sai_mod
    from sai_amd.utils.filesets import resident_bytes

    _no_rank_environment(monkeypatch)
    monkeypatch.chdir(K.ROOT)
    a, b, c = inputs["paths"][3]
    panel_bytes = os.path.getsize(inputs["panel"]) // 4
    estimates = [os.path.getsize(a) * 3, resident_bytes(b), resident_bytes(c)]  # bgzip text, .bed, packed .geno
    assert all(e > 0 for e in estimates)
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", str(panel_bytes))
    assert sai_mod.chunks_for_memory(inputs["panel"]) == 1
    assert sai_mod.chunks_for_memory(inputs["panel"], src_file=[a, b]) == -(-(panel_bytes + sum(estimates[:2])) // panel_bytes) >= 2
    assert sai_mod.chunks_for_memory(inputs["panel"], src_file=(a, b, c)) == -(-(panel_bytes + sum(estimates)) // panel_bytes)
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "1000")
    assert sai_mod.chunks_for_memory(inputs["panel"], src_file=[a, b, c]) - sai_mod.chunks_for_memory(inputs["panel"], src_file=[a, b]) in (
        estimates[2] // 1000, estimates[2] // 1000 + 1)  # fmt: skip


# -- the host readers ------------------------------------------------------------------------------------------------------

GROUPS = ("ref", "tgt", "src", "outgroup")


def groups_of(results):
    return {(g, p): (cd.POS, np.asarray(cd.GT)) for g in GROUPS for p, cd in ((results[g][0] or {}).items())}


@pytest.fixture(scope="module")
def read(inputs):
    from sai_amd.utils.read_data import read_dosage_data

    os.chdir(K.ROOT)
    cfg, lists = M.reader_arguments(inputs)
    return lambda vcf, **kw: read_dosage_data(vcf, "1", cfg.ploidies, *lists, inputs["anc"], **kw)


@pytest.mark.parametrize("cut", sorted(M.CUTS))
def test_host_route_equals_the_one_vcf_of_the_common_sites(inputs, read, cut):
    paths = inputs["paths"][cut]
    for kw in ({}, M.REGION):
        want = groups_of(read(inputs["common"][cut], **kw))
        got = read(inputs["panel"], src_file=paths, **kw)
        assert set(groups_of(got)) == set(want) == {("ref", "ref"), ("tgt", "tgt"), ("src", "NEA"), ("src", "DEN"), ("outgroup", "out")}
        assert got["src"][1] == {"NEA": M.NEA, "DEN": M.DEN}
        for key, (pos, gt) in groups_of(got).items():
            assert np.array_equal(pos, want[key][0]) and np.array_equal(gt, want[key][1]) and gt.dtype == want[key][1].dtype, key
        # NEA spans the files and stands in the order of the src list; DEN lies in one file
        assert groups_of(got)[("src", "NEA")][1].shape[1] == 3 and groups_of(got)[("src", "DEN")][1].shape[1] == 1
        summary = got["site_join"]
        assert set(summary) == {"n_common", "n_panel", "n_sources", "panel_identity", "source_identities"}
        assert summary["n_common"] == want[("ref", "ref")][0].size and len(summary["n_sources"]) == cut == len(summary["source_identities"])
        assert not summary["panel_identity"] and not any(summary["source_identities"]) and all(n > summary["n_common"] for n in summary["n_sources"])
        # the files in another order: the same blocks, the summary's lists in the files' order
        other = read(inputs["panel"], src_file=tuple(paths[::-1]), **kw)
        for key, (pos, gt) in groups_of(other).items():
            assert np.array_equal(pos, want[key][0]) and np.array_equal(gt, want[key][1]), key
        assert other["site_join"]["n_sources"] == summary["n_sources"][::-1]
    assert read(inputs["common"][cut])["ref"][0]["ref"].POS.size == inputs["n_common"][cut] < inputs["n_fixture"]


def test_a_sequence_of_one_path_is_that_path(tmp_path, monkeypatch):
    from sai_amd.sai import load_config
    from sai_amd.utils.read_data import read_dosage_data

    monkeypatch.chdir(K.ROOT)
    one = K.write_inputs(tmp_path)
    source = K.write_source(one, "vcf", tmp_path)
    cfg = load_config(str(K.CONFIG))
    lists = [cfg.populations.get_population(g) for g in GROUPS]
    read = lambda **kw: read_dosage_data(one["panel"], "1", cfg.ploidies, *lists, one["anc"], **kw)  # noqa: E731
    want = read(src_file=source)
    for form in ([source], (source,)):
        got = read(src_file=form)
        assert got["site_join"] == want["site_join"] and set(got["site_join"]) == {"n_common", "n_panel", "n_source", "panel_identity", "source_identity"}
        for key, (pos, gt) in groups_of(got).items():
            assert np.array_equal(pos, groups_of(want)[key][0]) and np.array_equal(gt, groups_of(want)[key][1])


def test_host_route_identity_no_common_site_and_no_record(inputs, read, tmp_path):
    import gzip

    # no common site: one file holds its own sites only -- as a region without a record, with the summary
    a, rest = inputs["paths"][3][0], inputs["paths"][3][1:]
    own = [ln for ln in gzip.open(a, "rt").read().splitlines() if ln.startswith("#") or int(ln.split("\t")[1]) in M.OWN_SITES[0]]
    (tmp_path / "apart.vcf").write_text("\n".join(own) + "\n")
    apart = read(inputs["panel"], src_file=[str(tmp_path / "apart.vcf"), *rest])
    empty = read(inputs["common"][3], start=39900, end=39910)
    assert apart["site_join"]["n_common"] == 0 and apart["site_join"]["n_sources"][0] == len(M.OWN_SITES[0])
    assert {g: apart[g] for g in GROUPS} == {g: empty[g] for g in GROUPS}
    assert all(apart[g][0] is None and apart[g][1] for g in GROUPS)
    # a region without a record in one input: every group without data, no summary
    none = read(inputs["panel"], src_file=inputs["paths"][3], start=39900, end=39910)
    assert {g: none[g] for g in GROUPS} == {g: empty[g] for g in GROUPS} and "site_join" not in none
    # a position that repeats in the third file: the file and the position are named
    lines = open(str(tmp_path / "apart.vcf")).read().splitlines()
    lines.append(lines[-1])
    (tmp_path / "repeated.vcf").write_text("\n".join(lines) + "\n")
    with pytest.raises(ValueError, match=rf"repeated\.vcf: position {M.OWN_SITES[0][-1]} repeats or does not ascend \(after {M.OWN_SITES[0][-1]}\)"):
        read(inputs["panel"], src_file=[*rest, str(tmp_path / "repeated.vcf")])


def test_window_generator_over_several_inputs_yields_the_windows_of_the_one_vcf(inputs, monkeypatch):
    from sai_amd.generators import WindowGenerator

    monkeypatch.chdir(K.ROOT)
    cfg, lists = M.reader_arguments(inputs)
    kw = dict(chr_name="1", ref_ind_file=lists[0], tgt_ind_file=lists[1], src_ind_file=lists[2], out_ind_file=lists[3], win_len=8000,
              win_step=4000, ploidy_config=cfg.ploidies, anc_allele_file=inputs["anc"], start=1, end=40000)  # fmt: skip
    want = list(WindowGenerator(vcf_file=inputs["common"][3], **kw).get())
    got = list(WindowGenerator(vcf_file=inputs["panel"], src_file=inputs["paths"][3], **kw).get())
    assert len(got) == len(want) > 5 and sum(len(w["pos"]) for w in want) > inputs["n_common"][3]  # the windows overlap
    assert {p for w in got for p in w["src_pop_list"]} == {"NEA", "DEN"}
    for a, b in zip(got, want):
        assert (a["start"], a["end"], a["ref_pop"], a["tgt_pop"], a["src_pop_list"], a["out_pop"]) == (b["start"], b["end"], b["ref_pop"], b["tgt_pop"], b["src_pop_list"], b["out_pop"])
        assert np.array_equal(a["pos"], b["pos"])
        for key in ("ref_gts", "tgt_gts", "out_gts"):
            assert (a[key] is None and b[key] is None) or np.array_equal(a[key], b[key]), key
        assert (a["src_gts_list"] is None and b["src_gts_list"] is None) or all(np.array_equal(x, y) for x, y in zip(a["src_gts_list"], b["src_gts_list"]))
