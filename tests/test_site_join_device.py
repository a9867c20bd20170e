"""Sources from a file of their own on the GPU: ``sai_tile_rows_from_site_major`` (sai_amd/csrc/join/tile_rows.hip)
against the layout formula of saihip.h, its guard against row indices outside the block, ``read_data_device(...,
src_file=)`` against the host route for every format the source file may have, and ``score(..., src_file=)`` against
``score`` on the one VCF of the common sites -- TSV, .U.log and .Q.log byte for byte: the device route, the host route,
several chunks, the command line and two workers."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import site_join_cases as K
from conftest import ROOT

pytestmark = pytest.mark.gpu

TILE = 64
WIDEST = 256  # individuals of the widest workgroup (tile_rows.hip: W = 16 .. 256)
N_ROWS = (0, 1, 63, 64, 65, 129)
N_IND = (1, 3, 15, 16, 17, 63, 64, 65, 130, WIDEST + 44)
SENTINEL = 85


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


@pytest.fixture(autouse=True)
def at_the_root(monkeypatch):
    """The fixture's configuration names its sample lists from the repository root."""
    monkeypatch.chdir(ROOT)


def expected_tiles(block, col0, n_ind, rows):
    """byte(t, i, s) = block[rows[t * 64 + s]][col0 + i], zero in the padding sites of the last tile: saihip.h's formula.
    A row index outside the block selects nothing: zeros."""
    rows = np.asarray(rows, dtype=np.int64)
    n_tiles = -(-rows.size // TILE)
    padded = np.zeros((n_tiles * TILE, n_ind), dtype=np.int8)
    inside = (rows >= 0) & (rows < block.shape[0])
    padded[np.flatnonzero(inside)] = block[rows[inside], col0 : col0 + n_ind]
    return np.ascontiguousarray(padded.reshape(n_tiles, TILE, n_ind).transpose(0, 2, 1)).reshape(-1)


def row_lists(n):
    """(name, list or None) over a block of n rows: None is the NULL list."""
    every = np.arange(n, dtype=np.int32)
    lists = [("NULL", None), ("identity", every), ("every other", every[::2].copy()), ("reversed", every[::-1].copy())]
    if n:
        lists += [("first", every[:1]), ("last", every[-1:]), ("one row 70 times", np.full(70, n // 2, dtype=np.int32))]
    return lists


def device_block(eng, host, margin=0, fill=0):
    """``host`` as an interior view of a device tensor with ``margin`` rows of ``fill`` before and behind it."""
    import torch

    whole = torch.full((host.shape[0] + 2 * margin, host.shape[1]), fill, dtype=torch.int8, device=eng.device)
    view = whole[margin : margin + host.shape[0]]
    view.copy_(torch.from_numpy(host))
    return view


@pytest.mark.parametrize("n_ind", N_IND)
def test_kernel_equals_the_layout_formula(eng, n_ind):
    import torch

    from sai_amd.site_join_device import RowTiler

    rng = np.random.default_rng(1000 + n_ind)
    tiler = RowTiler(eng)
    odd = n_ind + 6 + (n_ind + 1) % 2  # an odd width: with columns 5 .. every row starts at another alignment
    assert odd % 2 == 1
    for n in N_ROWS:
        for width, col0 in ((n_ind, 0), (odd, 5)):
            host = rng.integers(-128, 128, size=(n, width), dtype=np.int8)
            block = device_block(eng, host)
            for name, rows in row_lists(n):
                rows_dev = None if rows is None else torch.from_numpy(rows).to(eng.device)
                got = tiler.tile(block, col0, n_ind, rows_dev)
                want = expected_tiles(host, col0, n_ind, np.arange(n) if rows is None else rows)
                assert (got.n_sites, got.n_ind) == (n if rows is None else rows.size, n_ind)
                assert got.tiles.numel() == want.size and np.array_equal(got.tiles.cpu().numpy(), want), (n, width, name)
                if rows is None:  # ... and what the kernel of the one-input read gives
                    old = eng.tile_columns(block, list(range(col0, col0 + n_ind)))
                    assert torch.equal(old.tiles, got.tiles), (n, width)
    tiler.check()


@pytest.mark.parametrize("n_ind", (2, 4, 16, 20, 40, 100, 200, 2 * WIDEST + 3))
def test_kernel_over_several_workgroups_of_every_width(eng, n_ind):
    """2 053 selected rows are more than two workgroups of sites at every width a workgroup takes (16 tiles of 64 sites
    at the narrowest); the list is unsorted and repeats rows."""
    import torch

    from sai_amd.site_join_device import RowTiler

    rng = np.random.default_rng(n_ind)
    n_src, n_rows = 1500, 2 * 16 * TILE + 5
    host = rng.integers(-128, 128, size=(n_src, n_ind + 3), dtype=np.int8)
    rows = rng.integers(0, n_src, size=n_rows).astype(np.int32)
    tiler = RowTiler(eng)
    got = tiler.tile(device_block(eng, host), 3, n_ind, torch.from_numpy(rows).to(eng.device))
    assert np.array_equal(got.tiles.cpu().numpy(), expected_tiles(host, 3, n_ind, rows))
    tiler.check()


@pytest.mark.parametrize("n_ind", (2, 7, 64, WIDEST + 44))
def test_rows_out_of_range_are_counted_and_not_read(eng, n_ind):
    """The block is an interior view of a tensor filled with a sentinel, one row of margin on each side, so that a row
    list holding -1 and n_src_rows can make a kernel without the guard read the margin, never memory outside the tensor:
    it would show up as sentinel bytes."""
    import torch

    from sai_amd.site_join_device import RowTiler

    rng = np.random.default_rng(77 + n_ind)
    n_src, width, col0 = 97, n_ind + 4, 3
    values = np.array([v for v in range(-128, 128) if v not in (0, SENTINEL)], dtype=np.int8)
    host = values[rng.integers(0, values.size, size=(n_src, width))]
    block = device_block(eng, host, margin=1, fill=SENTINEL)
    rows = rng.integers(0, n_src, size=150).astype(np.int32)
    bad_at = np.array([0, 5, 63, 64, 65, 127, 128, 149])
    rows[bad_at] = np.where(np.arange(bad_at.size) % 2 == 0, -1, n_src)
    tiler = RowTiler(eng)
    got = tiler.tile(block, col0, n_ind, torch.from_numpy(rows).to(eng.device))
    assert int(tiler._bad[0].cpu()) == bad_at.size
    tiles = got.tiles.cpu().numpy()
    assert SENTINEL not in tiles
    assert np.array_equal(tiles, expected_tiles(host, col0, n_ind, rows))
    per_site = tiles.reshape(-1, n_ind, TILE).transpose(0, 2, 1).reshape(-1, n_ind)[: rows.size]
    assert not per_site[bad_at].any() and per_site[np.setdiff1d(np.arange(rows.size), bad_at)].all()
    with pytest.raises(RuntimeError, match=rf"met {bad_at.size} row indices outside their block"):
        tiler.check()
    # a call after it starts from zero again
    tiler.tile(block, col0, n_ind, torch.from_numpy(rows[1:5].copy()).to(eng.device))
    tiler.check()


def test_argument_errors(eng):
    import torch

    from sai_amd import _ffi
    from sai_amd import site_join_device as D

    lib = D.load()
    src = torch.zeros((4, 8), dtype=torch.int8, device=eng.device)
    rows = torch.zeros(4, dtype=torch.int32, device=eng.device)
    dst = torch.full((64 * 8 + 16,), 9, dtype=torch.int8, device=eng.device)
    n_bad = torch.full((1,), 7, dtype=torch.int32, device=eng.device)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    call = lambda *a: lib.sai_tile_rows_from_site_major(*a, eng._stream())  # noqa: E731
    assert call(None, p(src), 4, 8, 8, p(rows), 4, p(dst), p(n_bad)) == _ffi.SAI_ERR_ARG and lib.sai_last_error() == b"ctx is NULL"
    for args, code, words in (
        ((p(src), -1, 8, 8, p(rows), 4, p(dst), p(n_bad)), _ffi.SAI_ERR_ARG, b"negative size"),
        ((p(src), 4, -8, 8, p(rows), 4, p(dst), p(n_bad)), _ffi.SAI_ERR_ARG, b"negative size"),
        ((p(src), 4, 8, 8, p(rows), -4, p(dst), p(n_bad)), _ffi.SAI_ERR_ARG, b"negative size"),
        ((p(src), 4, 8, 8, p(rows), 4, p(dst), None), _ffi.SAI_ERR_ARG, b"NULL buffer"),
        ((None, 4, 8, 8, p(rows), 4, p(dst), p(n_bad)), _ffi.SAI_ERR_ARG, b"NULL buffer"),
        ((p(src), 4, 8, 8, p(rows), 4, None, p(n_bad)), _ffi.SAI_ERR_ARG, b"NULL buffer"),
        ((p(src), 4, 8, 8, p(rows), 4, p(dst, 8), p(n_bad)), _ffi.SAI_ERR_ARG, b"dst is not 16-byte aligned"),
        ((p(src), 4, 8, 7, p(rows), 4, p(dst), p(n_bad)), _ffi.SAI_ERR_ARG, b"row_stride 7 < n_ind 8"),
        ((p(src), 4, 8, 8, None, 3, p(dst), p(n_bad)), _ffi.SAI_ERR_ARG, b"rows is NULL (the identity) but n_rows 3 != n_src_rows 4"),
        ((p(src), 4, 65536 * 256 + 1, 65536 * 256 + 1, p(rows), 4, p(dst), p(n_bad)), _ffi.SAI_ERR_UNSUPPORTED, b"block too large for one launch"),
    ):  # fmt: skip
        assert call(eng.ctx, *args) == code and lib.sai_last_error() == words, words
    torch.cuda.synchronize()
    assert (dst == 9).all()  # a refused call writes nothing
    # nothing to tile: SAI_OK, and nothing but the count is touched
    for n_ind, n_rows in ((0, 4), (8, 0)):
        n_bad.fill_(7)
        assert call(eng.ctx, None, 4, n_ind, 8, p(rows), n_rows, None, p(n_bad)) == 0
        torch.cuda.synchronize()
        assert int(n_bad.cpu()) == 0 and (dst == 9).all()


# -- the resident reader ---------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return K.write_inputs(tmp_path_factory.mktemp("two_inputs"))


@pytest.fixture(scope="module")
def readers(eng, inputs):
    """(host read, device read) of the fixture's populations, and the host route's results shared by the cases."""
    from sai_amd.sai import load_config
    from sai_amd.utils.read_data import read_data_device, read_dosage_data

    os.chdir(ROOT)
    cfg = load_config(str(K.CONFIG))
    files = [cfg.populations.get_population(g) for g in ("ref", "tgt", "src", "outgroup")]
    host = lambda vcf, **kw: read_dosage_data(vcf, "1", cfg.ploidies, *files, inputs["anc"], **kw)  # noqa: E731
    device = lambda vcf, **kw: read_data_device(eng, vcf, "1", cfg.ploidies, *files, inputs["anc"], **kw)  # noqa: E731
    return host, device


GROUPS = ("ref", "tgt", "src", "outgroup")
REGION = dict(start=5000, end=30000)


def assert_device_equals_host(eng, got, pos_dev, want):
    """Every population's tiles are ``Engine.tile_many`` of the host route's matrix; ONE position array for all."""
    import torch

    keys = [(g, p) for g in GROUPS for p in (want[g][0] or {})]
    assert keys == [(g, p) for g in GROUPS for p in (got[g][0] or {})] and len(keys) == 4
    assert all(got[g][1] == want[g][1] for g in GROUPS)
    tiled = eng.tile_many([want[g][0][p].GT for g, p in keys])
    pos = got["ref"][0]["ref"].POS
    for (g, p), t in zip(keys, tiled):
        block = got[g][0][p]
        assert block.POS is pos, (g, p)
        assert (block.GT.n_sites, block.GT.n_ind) == (t.n_sites, t.n_ind) and torch.equal(block.GT.tiles, t.tiles), (g, p)
    assert pos.dtype == np.int32 and np.array_equal(pos, want["ref"][0]["ref"].POS)
    assert pos_dev.dtype == torch.int32 and np.array_equal(pos_dev.cpu().numpy(), pos)
    assert got["site_join"] == want["site_join"]


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_reader_equals_the_host_route(eng, inputs, readers, tmp_path, fmt):
    host, device = readers
    source = K.write_source(inputs, fmt, tmp_path)
    for kw in ({}, REGION):
        want = host(inputs["panel"], src_file=source, **kw)
        got, pos_dev = device(inputs["panel"], src_file=source, **kw)
        assert_device_equals_host(eng, got, pos_dev, want)
        assert 0 < got["site_join"]["n_common"] < got["site_join"]["n_source"] and not got["site_join"]["panel_identity"]


def test_reader_identity_same_file_and_no_common_site(eng, inputs, readers, tmp_path):
    import torch

    host, device = readers
    # the main input as its own source file: both sides the identity, the one-input blocks
    got, pos_dev = device(inputs["common"], src_file=inputs["common"])
    assert_device_equals_host(eng, got, pos_dev, host(inputs["common"], src_file=inputs["common"]))
    assert got["site_join"]["panel_identity"] and got["site_join"]["source_identity"]
    one, one_pos = device(inputs["common"])
    for g in GROUPS:
        for p, block in one[g][0].items():
            assert torch.equal(block.GT.tiles, got[g][0][p].GT.tiles) and np.array_equal(block.POS, got[g][0][p].POS)
    assert torch.equal(one_pos, pos_dev) and "site_join" not in one
    # the source file covers the panel (the panel's rows are the identity: the NULL list) and has sites of its own
    full = K.write_inputs(tmp_path, complete=True)
    source = K.write_source(full, "pgen", tmp_path)
    # the ancestral alleles of this pair of inputs are its own file
    from sai_amd.sai import load_config
    from sai_amd.utils.read_data import read_data_device, read_dosage_data

    cfg = load_config(str(K.CONFIG))
    files = [cfg.populations.get_population(g) for g in GROUPS]
    want = read_dosage_data(full["panel"], "1", cfg.ploidies, *files, full["anc"], src_file=source)
    got, pos_dev = read_data_device(eng, full["panel"], "1", cfg.ploidies, *files, full["anc"], src_file=source)
    assert_device_equals_host(eng, got, pos_dev, want)
    assert got["site_join"]["panel_identity"] and not got["site_join"]["source_identity"] and got["site_join"]["n_common"] == full["n_fixture"]
    # no common site: every group without data, no positions, the summary
    text = K.write_source(inputs, "vcf", tmp_path)
    own = [ln for ln in open(text).read().splitlines() if ln.startswith("#") or ln.split("\t")[1] in ("60", "7001", "30001", "39995")]
    (tmp_path / "apart.vcf").write_text("\n".join(own) + "\n")
    want = host(inputs["panel"], src_file=str(tmp_path / "apart.vcf"))
    got, pos_dev = device(inputs["panel"], src_file=str(tmp_path / "apart.vcf"))
    assert pos_dev is None and got["site_join"] == want["site_join"] and got["site_join"]["n_common"] == 0
    assert {g: got[g] for g in GROUPS} == {g: want[g] for g in GROUPS} and all(got[g][0] is None and got[g][1] for g in GROUPS)
    # a region without a record in one of the inputs: as the host route, without a summary
    want = host(inputs["panel"], src_file=text, start=39900, end=39910)
    got, pos_dev = device(inputs["panel"], src_file=text, start=39900, end=39910)
    assert pos_dev is None and {g: got[g] for g in GROUPS} == {g: want[g] for g in GROUPS} and ("site_join" in got) == ("site_join" in want)


# -- score -------------------------------------------------------------------------------------------------------------------

WIN = (8000, 4000)


@pytest.fixture(scope="module")
def run(inputs, tmp_path_factory):
    """The panel clipped to the span of the common sites (it keeps the sites of its own inside the span, so the window
    grid of the panel is the grid of the common VCF), a configuration that adds U, Q and DD to the fixture's statistics,
    and the files ``score`` writes for the common VCF."""
    tmp = tmp_path_factory.mktemp("score_two_inputs")
    common = [int(ln.split("\t")[1]) for ln in open(inputs["common"]) if not ln.startswith("#")]
    lines = open(inputs["panel"]).read().splitlines()
    kept = [ln for ln in lines if ln.startswith("#") or common[0] <= int(ln.split("\t")[1]) <= common[-1]]
    panel_pos = [int(ln.split("\t")[1]) for ln in kept if not ln.startswith("#")]
    assert (panel_pos[0], panel_pos[-1]) == (common[0], common[-1]) and len(set(panel_pos) - set(common)) > 10 and {5001, 20001} <= set(panel_pos)
    (tmp / "panel.vcf").write_text("\n".join(kept) + "\n")
    uq = "    ref:\n      ref: 0.3\n    tgt:\n      tgt: {x}\n    src:\n      src: \"=1\"\n"
    text = open(K.CONFIG).read()
    assert text.startswith("statistics:\n")
    (tmp / "config.yaml").write_text("statistics:\n  U:\n" + uq.format(x=0.2) + "  Q:\n" + uq.format(x=0.9) + "  DD: true\n" + text[len("statistics:\n") :])
    out = dict(tmp=tmp, panel=str(tmp / "panel.vcf"), config=str(tmp / "config.yaml"), anc=inputs["anc"], common=inputs["common"])
    os.chdir(ROOT)
    out["want"] = score_files(out, out["common"], None, tmp / "common" / "s.tsv")
    assert set(out["want"]) == {".tsv", ".U.log", ".Q.log"} and len(out["want"][".tsv"].splitlines()) > 5
    header = out["want"][".tsv"].splitlines()[0].split(b"\t")
    assert header[-7:] == [b"U", b"Q", b"DD", b"fd", b"df", b"Danc", b"Dplus"]
    return out


def files_of(out):
    return {p.name[len(out.stem) :]: p.read_bytes() for p in out.parent.glob(out.stem + "*")}


def score_files(run, vcf, src_file, out):
    from sai_amd.sai import score

    second = {} if src_file is None else {"src_file": src_file}
    score(vcf_file=vcf, chr_name="1", win_len=WIN[0], win_step=WIN[1], anc_allele_file=run["anc"], output_file=str(out), config=run["config"],
          num_workers=1, **second)  # fmt: skip
    return files_of(out)


def child_environment(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                            "SAI_AMD_INGEST", "SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT")}  # fmt: skip
    env.update(extra)
    return env


def sai_score(run, source, out, workers, **env):
    argv = [sys.executable, "-m", "sai_amd", "score", "--vcf", run["panel"], "--src-input", source, "--chr-name", "1", "--win-len", str(WIN[0]),
            "--win-step", str(WIN[1]), "--anc-alleles", run["anc"], "--config", run["config"], "--output", str(out), "--num-workers", str(workers)]  # fmt: skip
    res = subprocess.run(argv, cwd=str(ROOT), env=child_environment(**env), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    return files_of(out)


@pytest.mark.parametrize("fmt", ("vcf", "geno-packed"))
def test_score_writes_the_files_of_the_common_vcf(eng, inputs, run, tmp_path, monkeypatch, fmt):
    from sai_amd import sai as sai_mod

    monkeypatch.chdir(ROOT)
    for name in ("SAI_AMD_INGEST", "SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    source = K.write_source(inputs, fmt, tmp_path)
    assert score_files(run, run["panel"], source, tmp_path / "device" / "s.tsv") == run["want"]
    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    assert score_files(run, run["panel"], source, tmp_path / "host" / "s.tsv") == run["want"]
    monkeypatch.delenv("SAI_AMD_INGEST")
    # several chunks through the one GPU: every chunk reads and joins its own region of both files
    one_chunk = sai_mod.chunks_for_memory(run["panel"], src_file=source)
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", str(os.path.getsize(run["panel"]) // 4 // 3))
    assert one_chunk == 1 and sai_mod.chunks_for_memory(run["panel"], src_file=source) >= 3
    assert score_files(run, run["panel"], source, tmp_path / "chunks" / "s.tsv") == run["want"]
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES")
    if fmt == "vcf":  # the command, as a child process
        assert sai_score(run, source, tmp_path / "cli" / "s.tsv", 1) == run["want"]


def test_sai_score_with_two_workers_and_a_source_file(inputs, run, tmp_path):
    """`sai score --num-workers 2 --src-input ...`: the process starts its two ranks as a child job, both on this box's one
    GPU with gloo for the gather; each rank reads and joins its own regions of both files."""
    source = K.write_source(inputs, "bed", tmp_path)
    assert sai_score(run, source, tmp_path / "two" / "s.tsv", 2, SAI_AMD_DIST_BACKEND="gloo") == run["want"]
