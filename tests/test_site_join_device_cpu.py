"""Sources from a file of their own on the product path, without a GPU: the binding of the gathering re-tile
(sai_amd/site_join_device.py, sai_amd/csrc/join/tile_rows.hip), its unit in the build, what ``score(..., src_file=)``
refuses before it makes the output directory, and ``--src-input`` from the parser down to the ranks' command line.  The
kernel itself, the resident reader and the output files are tests/test_site_join_device.py."""

import os
import subprocess
import sys

import pytest

import site_join_cases as K

NAMES = ["sai_join_device_abi_version", "sai_tile_rows_from_site_major"]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return K.write_inputs(tmp_path_factory.mktemp("two_inputs"))


def test_binding_unit_and_the_null_context():
    from sai_amd import _build, _ffi
    from sai_amd import site_join_device as D

    assert sorted(D.SIGNATURES) == NAMES and D.HOST_SYMBOLS == ("sai_join_device_abi_version",)
    lib = D.load()
    assert all(hasattr(lib, n) for n in NAMES)
    assert lib.sai_join_device_abi_version() == D.SAI_JOIN_DEVICE_ABI_VERSION == 1
    assert "join/tile_rows.hip" in _build.UNITS and "join/tile_rows.hip" not in _build.HOST_UNITS
    assert _build.UNITS[-len(_build.HOST_UNITS) :] == _build.HOST_UNITS
    assert _build.UNITS.index("join/tile_rows.hip") == len(_build.UNITS) - len(_build.HOST_UNITS) - 1
    # the context is looked at before any other argument: without a GPU there is no other context than NULL, and the
    # other argument errors are checked where there is one (tests/test_site_join_device.py)
    assert lib.sai_tile_rows_from_site_major(None, None, -1, -1, 0, None, -1, None, None, None) == _ffi.SAI_ERR_ARG
    assert lib.sai_last_error() == b"ctx is NULL"


def _no_rank_environment(monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SAI_AMD_INGEST", "SAI_AMD_LAYOUT"):
        monkeypatch.delenv(name, raising=False)


def test_score_refusals_come_before_the_output_directory(inputs, tmp_path, monkeypatch):
    from sai_amd import sai as sai_mod

    _no_rank_environment(monkeypatch)
    monkeypatch.chdir(K.ROOT)
    source = K.write_source(inputs, "vcf", tmp_path)
    out = tmp_path / "made_by_score" / "s.tsv"
    ask = dict(vcf_file=inputs["panel"], chr_name="1", win_len=8000, win_step=4000, output_file=str(out), config=str(K.CONFIG))
    with pytest.raises(ValueError, match=r"requires `anc_allele_file`: the two inputs are reconciled through the ancestral allele.*follow-up"):
        sai_mod.score(anc_allele_file=None, num_workers=1, src_file=source, **ask)
    assert not out.parent.exists()
    for workers in (1, 2):
        with pytest.raises(ValueError, match=r"^a source file of its own is read in the int8 layout"):
            sai_mod.score(anc_allele_file=inputs["anc"], num_workers=workers, layout="packed2", src_file=source, **ask)
        assert not out.parent.exists()
        with pytest.raises(ValueError, match=r"^cannot open VCF .*no_such\.vcf$"):
            sai_mod.score(anc_allele_file=inputs["anc"], num_workers=workers, src_file=str(tmp_path / "no_such.vcf"), **ask)
        assert not out.parent.exists()
    # the layout from the environment is refused as the argument is
    monkeypatch.setenv("SAI_AMD_LAYOUT", "packed2")
    with pytest.raises(ValueError, match=r"^a source file of its own is read in the int8 layout"):
        sai_mod.score(anc_allele_file=inputs["anc"], num_workers=1, src_file=source, **ask)
    assert not out.parent.exists()


def test_reader_refusals_need_no_gpu(inputs, tmp_path, monkeypatch):
    """``read_data_device`` refuses before it reads (and before it touches the engine, which is None here)."""
    from sai_amd.sai import load_config
    from sai_amd.utils.read_data import read_data_device

    monkeypatch.chdir(K.ROOT)
    cfg = load_config(str(K.CONFIG))
    files = [cfg.populations.get_population(g) for g in ("ref", "tgt", "src", "outgroup")]
    with pytest.raises(ValueError, match=r"requires `anc_allele_file`"):
        read_data_device(None, inputs["panel"], "1", cfg.ploidies, *files, None, src_file=inputs["common"])
    with pytest.raises(ValueError, match=r"^a source file of its own is read in the int8 layout"):
        read_data_device(None, inputs["panel"], "1", cfg.ploidies, *files, inputs["anc"], layout="packed2", src_file=inputs["common"])
    with pytest.raises(TypeError):  # keyword-only
        read_data_device(None, inputs["panel"], "1", cfg.ploidies, *files, inputs["anc"], None, None, "int8", inputs["common"])


def _parse(argv):
    import argparse

    from sai_amd.parsers.score_parser import add_score_parser

    top = argparse.ArgumentParser()
    add_score_parser(top.add_subparsers())
    return top.parse_args(argv)


def test_src_input_reaches_score_and_the_ranks(inputs, tmp_path, monkeypatch):
    from sai_amd import distributed, launcher
    from sai_amd import sai as sai_mod
    from sai_amd.parsers import score_parser

    _no_rank_environment(monkeypatch)
    monkeypatch.chdir(K.ROOT)
    source = K.write_source(inputs, "bed", tmp_path)
    base = ["score", "--vcf", inputs["panel"], "--chr-name", "1", "--anc-alleles", inputs["anc"], "--output", str(tmp_path / "o.tsv"),
            "--config", str(K.CONFIG), "--num-workers", "1"]  # fmt: skip
    seen = []
    monkeypatch.setattr(score_parser, "score", lambda **kw: seen.append(kw))
    args = _parse(base + ["--src-input", source])
    args.runner(args)
    args = _parse(base)
    args.runner(args)
    assert seen[0]["src_file"] == source and seen[0]["vcf_file"] == inputs["panel"]
    assert "src_file" not in seen[1] and {k: v for k, v in seen[0].items() if k != "src_file"} == seen[1]  # without the flag: the call of before
    with pytest.raises(SystemExit):  # a fileset with a file missing, a file that does not exist: usage errors
        _parse(base + ["--src-input", str(tmp_path / "missing.bed")])
    with pytest.raises(SystemExit):
        _parse(base + ["--src-input", str(tmp_path / "missing.vcf")])
    res = subprocess.run([sys.executable, "-m", "sai_amd", "score", "--help"], cwd=str(K.ROOT), capture_output=True, text=True, timeout=600)
    helptext = " ".join(res.stdout.split())
    assert "--src-input PATH" in helptext and "Requires --anc-alleles" in helptext and "int8 layout" in helptext
    assert "the windows come from the main input" in helptext

    # the command line of the ranks
    plain = sai_mod._score_cli_arguments(inputs["panel"], "1", 10, 5, inputs["anc"], "o.tsv", str(K.CONFIG), 2)
    with_src = sai_mod._score_cli_arguments(inputs["panel"], "1", 10, 5, inputs["anc"], "o.tsv", str(K.CONFIG), 2, src_file=source)
    assert with_src == plain + ["--src-input", source] and "--src-input" not in plain
    assert _parse(with_src).src_input == source  # ... is one the parser takes

    # score(num_workers=2) hands it to the launcher, and a rank hands it to the sharded route; without it both calls are what they were
    launched, sharded = [], []
    monkeypatch.setattr(launcher, "launch_ranks", lambda n, argv, **kw: launched.append(argv) or 0)
    ask = dict(vcf_file=inputs["panel"], chr_name="1", win_len=10, win_step=5, anc_allele_file=inputs["anc"], output_file="o.tsv",
               config=str(K.CONFIG), num_workers=2)  # fmt: skip
    sai_mod.score(**ask, src_file=source)
    sai_mod.score(**ask)
    assert launched[0] == launched[1] + ["--src-input", source] and "--src-input" not in launched[1]
    monkeypatch.setattr(distributed, "score_sharded", lambda *a, **kw: sharded.append((a, kw)))
    monkeypatch.setattr(distributed, "shutdown_process_group", lambda: None)
    monkeypatch.setattr(launcher, "in_rank_job", lambda: True)
    sai_mod.score(**ask, src_file=source)
    sai_mod.score(**ask)
    assert sharded[0][0] == sharded[1][0] and sharded[0][1] == {**sharded[1][1], "src_file": source} and "src_file" not in sharded[1][1]

    # ... which builds its chunk driver with it, and the driver keeps it for the readers
    made = []
    monkeypatch.setattr(sai_mod, "ChunkPreprocessor", lambda *a, **kw: made.append((a, kw)))
    cfg = sai_mod.load_config(str(K.CONFIG))
    sai_mod.chunk_preprocessor_for(cfg, inputs["panel"], 10, 5, "o.tsv", inputs["anc"], src_file=source)
    sai_mod.chunk_preprocessor_for(cfg, inputs["panel"], 10, 5, "o.tsv", inputs["anc"])
    assert made[0][0] == made[1][0] and made[0][1] == {**made[1][1], "src_file": source} and "src_file" not in made[1][1]


def test_the_chunk_driver_and_the_memory_estimate_take_the_second_input(inputs, tmp_path, monkeypatch):
    from sai_amd import sai as sai_mod
    from sai_amd.preprocessors import ChunkPreprocessor

    _no_rank_environment(monkeypatch)
    monkeypatch.chdir(K.ROOT)
    cfg = sai_mod.load_config(str(K.CONFIG))
    source = K.write_source(inputs, "vcf", tmp_path)
    driver = sai_mod.chunk_preprocessor_for(cfg, inputs["panel"], 8000, 4000, str(tmp_path / "o.tsv"), inputs["anc"], src_file=source)
    assert isinstance(driver, ChunkPreprocessor) and driver.src_file == source and driver._second_input() == {"src_file": source}
    assert sai_mod.chunk_preprocessor_for(cfg, inputs["panel"], 8000, 4000, str(tmp_path / "o.tsv"), inputs["anc"])._second_input() == {}
    # the estimate: the source file's own is added to the panel's
    panel_bytes, source_bytes = os.path.getsize(inputs["panel"]) // 4, os.path.getsize(source) // 4
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", str(panel_bytes))
    assert sai_mod.chunks_for_memory(inputs["panel"]) == 1
    assert sai_mod.chunks_for_memory(inputs["panel"], src_file=source) == -(-(panel_bytes + source_bytes) // panel_bytes) == 2
