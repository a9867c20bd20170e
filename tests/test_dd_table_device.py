"""The DD table kernels on the GPU (sai_amd/csrc/dd_table/): ``sai_site_absdiff_table`` entry by entry against its
host twin and against ``Engine.site_absdiff`` of a constant source row, ``sai_window_dd_table`` bit for bit against
``Engine.window_dd(Engine.site_absdiff(...))``, and ``score`` through the table route against the old one byte for
byte.  The inputs and their numpy statements are tests/dd_table_cases.py's, proved on the host by
tests/test_dd_table_cpu.py (among them: no fixture here holds a source byte outside ``DD_VALUES``)."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dd_table_cases as D
import sum_order_cases as S
import test_grid_stride_cpu as G
from conftest import ROOT
from test_dd_table_cpu import host_table, host_window, same_bits
from test_plink_cpu import HET, HOM_A1, HOM_A2, write_vcf

pytestmark = pytest.mark.gpu

SITE_TILES_PER_CU = 16  # `constexpr int kStreamWavesPerCu = 16;` (common.hpp): the one-wave blocks per CU `stream_grid` launches at most
SENTINEL = 0x5A5A5A5A


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


def values_array(values):
    return (C.c_int8 * len(values))(*values)


def sai_pop(t):
    from sai_amd import _ffi

    p = _ffi.SaiPop()
    p.tiles, p.n_ind, p.ploidy = (t.tiles.data_ptr() if t.tiles.numel() else 0), t.n_ind, 1
    return p


def device_table(eng, pop, values):
    """``sai_site_absdiff_table`` into the interior of a sentinel-filled tensor: int64 [len(values)][n_sites]; the words
    around the table are checked here."""
    import torch

    from sai_amd import _ffi, dd_table

    lib = dd_table.load()
    n = len(values) * pop.n_sites
    whole = torch.full((n + 24,), SENTINEL, dtype=torch.int32, device=eng.device)
    table = whole[8 : 8 + n]
    _ffi.check(lib.sai_site_absdiff_table(eng.ctx, pop.n_sites, C.byref(sai_pop(pop)), len(values), values_array(values), C.c_void_p(table.data_ptr()),
                                          eng._stream()), lib)  # fmt: skip
    got = whole.cpu().numpy().view(np.uint32)
    assert (got[:8] == SENTINEL).all() and (got[8 + n :] == SENTINEL).all()
    return got[8 : 8 + n].astype(np.int64).reshape(len(values), pop.n_sites)


def constant_rows(eng, n_sites, values):
    """A source 'population' whose individual k holds values[k] at every site."""
    return eng.tile(np.broadcast_to(np.asarray(values, dtype=np.int8)[None, :], (n_sites, len(values))).copy())


def tiled(eng, g):
    """``Engine.tile``; a population of nobody is an empty block."""
    import torch

    from sai_amd.engine import TiledPop

    if g.shape[1] == 0:
        return TiledPop(tiles=torch.empty((0,), dtype=torch.int8, device=eng.device), n_sites=g.shape[0], n_ind=0)
    return eng.tile(g)


def check_table(eng, g, values, where):
    pop = tiled(eng, g)
    got = device_table(eng, pop, values)
    assert np.array_equal(got, host_table(g, values).astype(np.int64)), where  # the twin
    if g.shape[1] > 0:  # the existing kernel, a constant source row per value
        old = eng.site_absdiff(pop, constant_rows(eng, g.shape[0], values)).cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(got, old), where
    return got


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("n_ind", D.N_IND)
def test_table_equals_the_twin_and_site_absdiff(eng, n_ind, kind):
    for n_sites in D.N_SITES:
        g = D.genotypes(n_sites, n_ind, kind)
        for values in D.VALUE_LISTS:
            got = check_table(eng, g, values, (n_ind, n_sites, values))
            assert np.array_equal(got, D.table_numpy(values, g))


@pytest.mark.parametrize("n_ind", [D.widen_rows() - 1, D.widen_rows(), D.widen_rows() + 1, 2 * D.widen_rows() + 17])
def test_table_where_the_packed_fields_are_widened(eng, n_ind):
    """4 096 individuals fill one chunk of 16-bit fields to the last group; one more opens a second chunk.  Every byte
    at the far end from the value: each group adds the 1020 a field is sized for."""
    rng = np.random.default_rng(n_ind)
    g = rng.integers(-128, 128, size=(130, n_ind)).astype(np.int8)
    g[:70] = np.where(np.arange(70)[:, None] % 2 == 0, -128, 127)  # |127 - (-128)| = 255 in every row
    for values in ((127, -128, 0), D.VALUE_LISTS[2], D.DD_VALUES):
        got = check_table(eng, g, values, (n_ind, values))
        assert np.array_equal(got, D.table_numpy(values, g))
    assert got.max() < 2**31 and D.table_numpy((127,), g)[0, 0] == 255 * n_ind


def test_table_past_the_grid_cap(eng):
    """2 x the cap of stream_grid tiles plus a few, 3 individuals: every block takes its second grid-stride step."""
    import torch

    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    n_sites = G.site_count(SITE_TILES_PER_CU * n_cu)
    assert -(-n_sites // 64) > 2 * SITE_TILES_PER_CU * n_cu
    (g,) = G.site_mats(n_sites, (3,), True, seed=33)
    got = check_table(eng, g, D.DD_VALUES, "grid stride")
    assert np.array_equal(got, D.table_numpy(D.DD_VALUES, g))


# ---- the window kernel ----


def device_window(eng, src, table_ref, n_ref, table_tgt, n_tgt, windows, values=D.DD_VALUES):
    """``sai_window_dd_table`` with tables, scratch and dd as interior views of sentinel-filled tensors:
    (d f64 [n_windows][n_src], dd f64 [n_windows], n_unlisted); the sentinels are checked here."""
    import torch

    from sai_amd import _ffi, dd_table

    lib = dd_table.load()
    w = np.asarray(windows, dtype=np.int32).reshape(-1, 2)
    lo, hi = (torch.from_numpy(np.ascontiguousarray(w[:, k])).to(eng.device) for k in (0, 1))
    n_w, n_src, n_sites, n_v = len(w), src.n_ind, src.n_sites, len(values)

    def interior(data, dtype, fill):
        whole = torch.full((data.size + 16,), fill, dtype=dtype, device=eng.device)
        whole[8 : 8 + data.size] = torch.from_numpy(data.reshape(-1)).to(eng.device)
        return whole, whole[8 : 8 + data.size]

    ref_whole, ref_view = interior(np.ascontiguousarray(table_ref, dtype=np.uint32).view(np.int32), torch.int32, SENTINEL)
    tgt_whole, tgt_view = interior(np.ascontiguousarray(table_tgt, dtype=np.uint32).view(np.int32), torch.int32, SENTINEL)
    assert ref_view.numel() == n_v * n_sites
    scratch_whole = torch.full((n_w * n_src + 16,), -7.0, dtype=torch.float64, device=eng.device)
    dd_whole = torch.full((n_w + 16,), -7.0, dtype=torch.float64, device=eng.device)
    scratch, dd = scratch_whole[8 : 8 + n_w * n_src], dd_whole[8 : 8 + n_w]
    counter = torch.full((3,), -1, dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_window_dd_table(eng.ctx, n_sites, C.byref(sai_pop(src)), n_v, values_array(values), C.c_void_p(ref_view.data_ptr()), n_ref,
                                       C.c_void_p(tgt_view.data_ptr()), n_tgt, n_w, eng._ptr(lo), eng._ptr(hi), C.c_void_p(scratch.data_ptr()),
                                       C.c_void_p(dd.data_ptr()), C.c_void_p(counter[1:2].data_ptr()), eng._stream()), lib)  # fmt: skip
    for whole, view in ((ref_whole, ref_view), (tgt_whole, tgt_view)):
        host = whole.cpu().numpy()
        assert (host[:8] == SENTINEL).all() and (host[-8:] == SENTINEL).all()
    s_host, d_host, c_host = scratch_whole.cpu().numpy(), dd_whole.cpu().numpy(), counter.cpu().numpy()
    assert (s_host[:8] == -7.0).all() and (s_host[-8:] == -7.0).all() and (d_host[:8] == -7.0).all() and (d_host[-8:] == -7.0).all()
    assert c_host[0] == -1 and c_host[2] == -1
    return s_host[8:-8].reshape(n_w, n_src), d_host[8:-8], int(c_host[1])


def old_route(eng, ref_t, tgt_t, src_t, windows):
    import torch

    w = np.asarray(windows, dtype=np.int32).reshape(-1, 2)
    lo, hi = (torch.from_numpy(np.ascontiguousarray(w[:, k])).to(eng.device) for k in (0, 1))
    return eng.window_dd(eng.site_absdiff(ref_t, src_t), ref_t.n_ind, eng.site_absdiff(tgt_t, src_t), tgt_t.n_ind, lo, hi).cpu().numpy()


@pytest.fixture(scope="module")
def blocks(eng):
    """{n_sites: (ref, tgt tiled, table_ref, table_tgt as the table kernel made them)} of ``D.window_block``."""
    out = {}
    for n in (D.BLOCK_SITES, D.long_block_sites()):
        ref, tgt, want_ref, want_tgt = D.window_block(n)
        ref_t, tgt_t = eng.tile(ref), eng.tile(tgt)
        table_ref, table_tgt = device_table(eng, ref_t, D.DD_VALUES), device_table(eng, tgt_t, D.DD_VALUES)
        assert np.array_equal(table_ref, want_ref) and np.array_equal(table_tgt, want_tgt)
        out[n] = (ref_t, tgt_t, table_ref, table_tgt)
    return out


@pytest.mark.parametrize("n_src", D.N_SRC)
def test_window_kernel_equals_the_old_route_bit_for_bit(eng, blocks, n_src):
    ref_t, tgt_t, table_ref, table_tgt = blocks[D.BLOCK_SITES]
    src = D.window_source(n_src)
    src_t = eng.tile(src)
    d, dd, n_unlisted = device_window(eng, src_t, table_ref, S.N_REF, table_tgt, S.N_TGT, S.WINDOWS)
    assert n_unlisted == 0
    assert np.array_equal(dd.view(np.int64), old_route(eng, ref_t, tgt_t, src_t, S.WINDOWS).view(np.int64))
    want_d, want_dd, _ = D.window_expected(n_src, S.WINDOWS)  # numpy's own order, and the twin
    assert same_bits(d, want_d) and same_bits(dd, want_dd)
    if n_src <= 129:
        h_d, h_dd, h_n = host_window(src, D.DD_VALUES, table_ref, S.N_REF, table_tgt, S.N_TGT, S.WINDOWS)
        assert h_n == 0 and same_bits(d, h_d) and same_bits(dd, h_dd)


@pytest.mark.parametrize("n_src", [5, 9])
def test_window_kernel_at_the_staging_capacity_and_past_it(eng, blocks, n_src):
    """A window of exactly dd_stage_sites(7) sites is staged in LDS, one a site longer and one over the whole block read
    the tables in place: the same doubles."""
    n = D.long_block_sites()
    ref_t, tgt_t, table_ref, table_tgt = blocks[n]
    windows = D.capacity_windows()
    lo, hi = S.clamp(windows, n)
    cap = D.stage_sites(len(D.DD_VALUES))
    assert cap in (hi - lo) and cap + 1 in (hi - lo) and n in (hi - lo)
    src_t = eng.tile(D.window_source(n_src, n))
    d, dd, n_unlisted = device_window(eng, src_t, table_ref, S.N_REF, table_tgt, S.N_TGT, windows)
    assert n_unlisted == 0
    assert np.array_equal(dd.view(np.int64), old_route(eng, ref_t, tgt_t, src_t, windows).view(np.int64))
    want_d, want_dd, _ = D.window_expected(n_src, windows, n)
    assert same_bits(d, want_d) and same_bits(dd, want_dd)


def test_window_kernel_with_other_value_lists_counts_unlisted_bytes(eng):
    values = D.VALUE_LISTS[2]
    ref, tgt, src = (D.genotypes(130, k, "all", seed=5) for k in (S.N_REF, S.N_TGT, 17))
    table_ref, table_tgt = D.table_numpy(values, ref), D.table_numpy(values, tgt)
    windows = ((0, 130), (0, 64), (60, 70), (129, 130), (7, 7))
    h_d, h_dd, h_n = host_window(src, values, table_ref, S.N_REF, table_tgt, S.N_TGT, windows)
    d, dd, n_unlisted = device_window(eng, eng.tile(src), table_ref, S.N_REF, table_tgt, S.N_TGT, windows, values)
    assert 0 < n_unlisted == h_n and same_bits(d, h_d) and same_bits(dd, h_dd)
    # one value, listed everywhere: nothing is counted
    one = np.full((130, 4), 3, dtype=np.int8)
    t_ref, t_tgt = D.table_numpy((3,), ref), D.table_numpy((3,), tgt)
    h_d, h_dd, h_n = host_window(one, (3,), t_ref, S.N_REF, t_tgt, S.N_TGT, windows)
    d, dd, n_unlisted = device_window(eng, eng.tile(one), t_ref, S.N_REF, t_tgt, S.N_TGT, windows, (3,))
    assert n_unlisted == h_n == 0 and same_bits(d, h_d) and same_bits(dd, h_dd)


def test_the_python_entry_points(eng, blocks):
    import torch

    from sai_amd import dd_table

    ref_t, tgt_t, want_ref, want_tgt = blocks[D.BLOCK_SITES]
    dd_table.reset_calls()
    table_ref, table_tgt = dd_table.site_absdiff_table(eng, ref_t), dd_table.site_absdiff_table(eng, tgt_t)
    assert table_ref.dtype == torch.int32 and tuple(table_ref.shape) == (7, D.BLOCK_SITES)
    assert np.array_equal(table_ref.cpu().numpy(), want_ref) and np.array_equal(table_tgt.cpu().numpy(), want_tgt)
    w = np.asarray(S.WINDOWS, dtype=np.int32)
    lo, hi = (torch.from_numpy(np.ascontiguousarray(w[:, k])).to(eng.device) for k in (0, 1))
    src_t = eng.tile(D.window_source(9))
    dd, n_unlisted = dd_table.window_dd_table(eng, src_t, table_ref, S.N_REF, table_tgt, S.N_TGT, lo, hi)
    assert dd.is_cuda and n_unlisted.is_cuda and n_unlisted.dtype == torch.int32 and int(n_unlisted.cpu()[0]) == 0
    assert same_bits(dd.cpu().numpy(), D.window_expected(9, S.WINDOWS)[1])
    assert dd_table.CALLS == {"site_absdiff_table": 2, "window_dd_table": 1, "old_route": 0}
    with pytest.raises(ValueError, match="the tables must be"):
        dd_table.window_dd_table(eng, src_t, table_ref[:3], S.N_REF, table_tgt, S.N_TGT, lo, hi)


# ---- the route in score_windows ----


def run_arrays(tmp_path, tag, gts, pl, stats, anc=True):
    """``FeaturePreprocessor.score_and_write`` over arrays: the bytes of the TSV and the two logs."""
    import json

    from sai_amd.configs import PloidyConfig, StatConfig
    from sai_amd.generators import WindowGenerator
    from sai_amd.preprocessors import FeaturePreprocessor
    from sai_amd.sai import write_headers
    from sai_amd.utils import ChromosomeData

    pos = np.arange(1, 1 + 40 * len(gts["ref"]["R"]), 40)
    data = {grp: {k: ChromosomeData(pos, None, None, v.astype(np.int8)) for k, v in gts[grp].items()} for grp in gts}
    pc = PloidyConfig(pl)
    wg = WindowGenerator.from_arrays("7", data["ref"], data["tgt"], data["src"], 2000, 1000, pc)
    stat_config = StatConfig(json.loads(json.dumps(stats)))
    out = tmp_path / tag / "o.tsv"
    out.parent.mkdir()
    fp = FeaturePreprocessor(str(out), stat_config, anc_allele_available=anc)
    write_headers(str(out), stat_config, pc)
    fp.score_and_write(wg)
    return {p.name: p.read_bytes() for p in out.parent.iterdir()}


def test_one_unlisted_source_byte_takes_the_old_route(eng, tmp_path, monkeypatch):
    from sai_amd import dd_table

    monkeypatch.delenv("SAI_AMD_DD_TABLE", raising=False)
    monkeypatch.delenv("SAI_AMD_DD_TABLE_MIN_ROWS", raising=False)
    rng = np.random.default_rng(8)
    n = 300
    gts = {"ref": {"R": rng.integers(0, 3, (n, 7))}, "tgt": {"T": rng.integers(0, 3, (n, 3))},
           "src": {"A": rng.integers(0, 3, (n, 6)), "B": rng.integers(0, 3, (n, 5))}}  # fmt: skip
    gts["src"]["B"][150, 2] = 5  # no dosage of ploidy 2, and not in DD_VALUES
    pl = {"ref": {"R": 2}, "tgt": {"T": 2}, "src": {"A": 2, "B": 2}}
    dd_table.reset_calls()
    got = run_arrays(tmp_path, "table", gts, pl, {"DD": True})
    calls = dict(dd_table.CALLS)
    assert calls["site_absdiff_table"] == 2 and calls["window_dd_table"] == 2 and calls["old_route"] == 1  # B alone is done again
    monkeypatch.setenv("SAI_AMD_DD_TABLE", "0")
    dd_table.reset_calls()
    want = run_arrays(tmp_path, "old", gts, pl, {"DD": True})
    assert dd_table.CALLS == {"site_absdiff_table": 0, "window_dd_table": 0, "old_route": 2}
    assert got == want and len(got["o.tsv"].splitlines()) > 5
    # the same without the byte: no population is done again; and with a source of ploidy 3 the old route serves all
    monkeypatch.delenv("SAI_AMD_DD_TABLE")
    gts["src"]["B"][150, 2] = 1
    dd_table.reset_calls()
    clean = run_arrays(tmp_path, "clean", gts, pl, {"DD": True})
    assert dd_table.CALLS == {"site_absdiff_table": 2, "window_dd_table": 2, "old_route": 0} and clean != got
    dd_table.reset_calls()
    pl["src"]["B"] = 3
    assert run_arrays(tmp_path, "ploidy3", gts, pl, {"DD": True}) == clean
    assert dd_table.CALLS == {"site_absdiff_table": 0, "window_dd_table": 0, "old_route": 2}


# ---- the product: a VCF of a few hundred sites through `score` ----

SRC_POPS = (("A", 5, 2), ("B", 8, 2), ("C", 9, 2), ("H", 6, 1))  # name, individuals, ploidy
WIN = (6000, 3000)
UQ = "    ref:\n      R: 0.4\n    tgt:\n      T: {x}\n    src:\n      A: \"=1\"\n      B: \">=0.5\"\n      C: \">0.2\"\n      H: \"<=1\"\n"
CONFIGS = {"dd": "  DD: true\n", "dd_uq": "  U:\n" + UQ.format(x=0.3) + "  Q:\n" + UQ.format(x=0.8) + "  DD: true\n",
           "dd_fd": "  fd: true\n  DD: true\n  df: true\n  Danc: true\n  Dplus: true\n"}  # fmt: skip


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    """A panel of 12 reference, 10 target, 4 outgroup and 5 + 8 + 9 diploid and 6 haploid source samples over 360 sites,
    as one VCF, as a panel VCF without the sources plus a VCF of the sources, with ancestral alleles (a third of them
    the ALT allele: those rows are flipped) and the three configurations."""
    tmp = tmp_path_factory.mktemp("dd_table_product")
    rng = np.random.default_rng(2026)
    n = 360
    groups = [("R", 12, 2, "ref"), ("T", 10, 2, "tgt"), ("O", 4, 2, "outgroup")] + [(p, k, pl, "src") for p, k, pl in SRC_POPS]
    samples, haploid = [], []
    for pop, k, pl, _ in groups:
        names = [f"{pop}_{i}" for i in range(k)]
        samples += names
        haploid += names if pl == 1 else []
    freq = rng.random(n) ** 2
    codes = np.empty((n, len(samples)), dtype=np.uint8)
    for c, s in enumerate(samples):
        f = np.clip(freq + (0.3 if s[0] in "ABCH" else 0.0), 0, 1)
        alleles = (rng.random((n, 2)) < f[:, None]).sum(axis=1)
        if s in haploid:
            alleles = np.where(alleles >= 1, 2, 0)
        codes[:, c] = np.choose(alleles, [HOM_A2, HET, HOM_A1])
    pos = np.cumsum(rng.integers(20, 140, n))
    args = (["1"] * n, pos, ["."] * n, ["T"] * n, ["A"] * n)
    write_vcf(tmp / "all.vcf", *args, codes, samples, haploid=haploid)
    is_src = np.array([s[0] in "ABCH" for s in samples])
    write_vcf(tmp / "panel.vcf", *args, codes[:, ~is_src], [s for s, m in zip(samples, is_src) if not m])
    write_vcf(tmp / "sources.vcf", *args, codes[:, is_src], [s for s, m in zip(samples, is_src) if m], haploid=haploid)
    with open(tmp / "anc.alleles", "w") as f:
        for k, p in enumerate(pos):
            f.write(f"1\t{p - 1}\t{p}\t{'T' if k % 3 == 0 else 'A'}\n")  # REF is A, ALT is T
    for kind in ("ref", "tgt", "src", "outgroup"):
        with open(tmp / f"{kind}.list", "w") as f:
            for pop, k, _, g in groups:
                if g == kind:
                    f.writelines(f"{pop}\t{pop}_{i}\n" for i in range(k))
    tail = ("\nploidies:\n  ref:\n    R: 2\n  tgt:\n    T: 2\n  src:\n" + "".join(f"    {p}: {pl}\n" for p, _, pl in SRC_POPS) + "  outgroup:\n    O: 2\n"
            "\npopulations:\n" + "".join(f"  {k}: \"{tmp / (k + '.list')}\"\n" for k in ("ref", "tgt", "src", "outgroup")))  # fmt: skip
    for name, stats in CONFIGS.items():
        (tmp / f"{name}.yaml").write_text("statistics:\n" + stats + tail)
    return dict(tmp=tmp, all=str(tmp / "all.vcf"), panel=str(tmp / "panel.vcf"), sources=str(tmp / "sources.vcf"), anc=str(tmp / "anc.alleles"))


def files_of(out):
    return {p.name[len(out.stem) :]: p.read_bytes() for p in out.parent.glob(out.stem + "*")}


def score_files(product, config, out, vcf=None, src_file=None):
    from sai_amd.sai import score

    second = {} if src_file is None else {"src_file": src_file}
    score(vcf_file=vcf or product["all"], chr_name="1", win_len=WIN[0], win_step=WIN[1], anc_allele_file=product["anc"], output_file=str(out),
          config=str(product["tmp"] / f"{config}.yaml"), num_workers=1, **second)  # fmt: skip
    return files_of(out)


def clear_environment(monkeypatch):
    monkeypatch.chdir(ROOT)
    for name in ("SAI_AMD_DD_TABLE", "SAI_AMD_DD_TABLE_MIN_ROWS", "SAI_AMD_INGEST", "SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "WORLD_SIZE", "RANK",
                 "LOCAL_RANK"):  # fmt: skip
        monkeypatch.delenv(name, raising=False)


def dd_of_the_oracle(product, config):
    """{(start, end): [DD per source population]} from ``oracle.sai_oracle.dd_stat`` on the host route's matrices."""
    from oracle import sai_oracle as O
    from sai_amd.sai import load_config
    from sai_amd.utils.read_data import read_dosage_data

    cfg = load_config(str(product["tmp"] / f"{config}.yaml"))
    lists = [cfg.populations.get_population(g) for g in ("ref", "tgt", "src", "outgroup")]
    data = read_dosage_data(product["all"], "1", cfg.ploidies, *lists, product["anc"])
    ref, tgt = data["ref"][0]["R"], data["tgt"][0]["T"]
    srcs = [data["src"][0][p] for p, _, _ in SRC_POPS]

    def dd(start, end):
        m = (ref.POS >= start) & (ref.POS <= end)
        return O.dd_stat(ref.GT[m], tgt.GT[m], [s.GT[m] for s in srcs])

    return dd


@pytest.mark.parametrize("config", list(CONFIGS))
def test_score_writes_the_same_bytes_on_both_routes(eng, product, tmp_path, monkeypatch, config):
    from sai_amd import dd_table

    clear_environment(monkeypatch)
    dd_table.reset_calls()
    got = score_files(product, config, tmp_path / "table" / "s.tsv")
    calls = dict(dd_table.CALLS)
    assert calls["site_absdiff_table"] == 2 and calls["window_dd_table"] == len(SRC_POPS) and calls["old_route"] == 0  # the table route ran
    monkeypatch.setenv("SAI_AMD_DD_TABLE", "0")
    dd_table.reset_calls()
    want = score_files(product, config, tmp_path / "old" / "s.tsv")
    assert dd_table.CALLS == {"site_absdiff_table": 0, "window_dd_table": 0, "old_route": len(SRC_POPS)}
    assert {".tsv", ".U.log", ".Q.log"} >= set(got) >= {".tsv"} and got == want
    # the values are the oracle's on the host route's matrices
    rows = [ln.split("\t") for ln in got[".tsv"].decode().splitlines()]
    header, rows = rows[0], rows[1:]
    cols = [header.index(f"DD.{p}") for p, _, _ in SRC_POPS]
    dd = dd_of_the_oracle(product, config)
    assert len(rows) > 5
    for row in rows:
        want_dd = dd(int(row[1]), int(row[2]))
        assert all(a == b or (a != a and b != b) for a, b in zip([float(row[c]) for c in cols], [float(v) for v in want_dd])), row[:3]
    assert any(float(row[c]) != 0.0 for row in rows for c in cols)


def test_score_with_a_source_file_of_its_own(eng, product, tmp_path, monkeypatch):
    from sai_amd import dd_table

    clear_environment(monkeypatch)
    want = score_files(product, "dd_uq", tmp_path / "one" / "s.tsv")
    dd_table.reset_calls()
    got = score_files(product, "dd_uq", tmp_path / "two" / "s.tsv", vcf=product["panel"], src_file=product["sources"])
    assert dd_table.CALLS["window_dd_table"] == len(SRC_POPS) and dd_table.CALLS["old_route"] == 0
    assert got == want
    monkeypatch.setenv("SAI_AMD_DD_TABLE", "0")
    assert score_files(product, "dd_uq", tmp_path / "two_old" / "s.tsv", vcf=product["panel"], src_file=product["sources"]) == want


def test_sai_score_with_two_workers_on_one_gpu(product, tmp_path, monkeypatch):
    """`sai score --num-workers 2`: the two ranks share this box's one GPU, gloo for the gather; the files of one process."""
    clear_environment(monkeypatch)
    want = score_files(product, "dd_uq", tmp_path / "one" / "s.tsv")
    out = tmp_path / "two" / "s.tsv"
    argv = [sys.executable, "-m", "sai_amd", "score", "--vcf", product["all"], "--chr-name", "1", "--win-len", str(WIN[0]), "--win-step", str(WIN[1]),
            "--anc-alleles", product["anc"], "--config", str(product["tmp"] / "dd_uq.yaml"), "--output", str(out), "--num-workers", "2"]  # fmt: skip
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SAI_AMD_DIST_BACKEND"] = "gloo"
    res = subprocess.run(argv, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert files_of(out) == want
