"""Per-site frequencies straight from packed2 blocks, on the GPU: ``sai_packed2_site_freqs`` against its host twin and
against the two launches it replaces (``sai_site_pass_packed2(counts)`` + ``sai_site_freqs``), past its grid cap, and
fd / df / Danc / Dplus of ``score(..., layout="packed2")`` against the reference's table and against the int8 layout."""

import ctypes as C

import numpy as np
import pytest

import pgen_builder as B
from conftest import DATA
from test_bed_pack2_device import eng, score_files  # noqa: F401 -- `eng` is a fixture
from test_packed_stats_cpu import N_IND, N_SITES, case, host_freqs, same_bits
from test_plink_cpu import HET, HOM_A1, HOM_A2, MISSING, fileset_from_vcf, write_fileset

pytestmark = pytest.mark.gpu

STREAM_WAVES_PER_CU = 16  # `constexpr int kStreamWavesPerCu = 16;` -- the grid cap of stream_grid() (csrc/common.hpp)
FORCED_TYPES = (0, 4, 2, 1, 3, 6, 2, 7)  # every .pgen record type in turn: one encoding per row keeps the writer quick


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def packed_pops(eng, blocks, n_inds, n_sites):
    import torch

    from sai_amd.engine import PackedPop

    return [PackedPop(torch.from_numpy(np.ascontiguousarray(b)).to(eng.device), n_sites, n) for b, n in zip(blocks, n_inds)]


def device_freqs(eng, blocks, n_inds, ploidies, n_sites):
    import torch

    from sai_amd.packed_stats import packed_site_freqs

    freqs = packed_site_freqs(eng, packed_pops(eng, blocks, n_inds, n_sites), ploidies)
    torch.cuda.synchronize()
    return freqs.cpu().numpy()


@pytest.mark.parametrize("n_ind", N_IND)
def test_kernel_equals_the_host_twin(eng, n_ind):
    """One population of every width, every site count, both ploidies: the numpy statement's doubles (which the CPU test
    holds the twin to), NaN positions included."""
    rng = np.random.default_rng(900 + n_ind)
    for n_sites in N_SITES:
        blocks, want, ploidies = case(rng, n_sites, [n_ind])
        for ploidy in (1, 2):
            twin = host_freqs(blocks, [n_ind], [ploidy], n_sites, 3)
            assert ploidy != ploidies[0] or same_bits(twin, want)
            assert np.isnan(twin[0, -1]) and np.isnan(twin).sum() == 1
            assert same_bits(device_freqs(eng, blocks, [n_ind], [ploidy], n_sites), twin), (n_ind, n_sites, ploidy)


@pytest.mark.parametrize("n_pops", [1, 4, 9])
def test_kernel_on_several_populations_of_different_widths(eng, n_pops):
    rng = np.random.default_rng(40 + n_pops)
    for n_sites in N_SITES:
        n_inds = [N_IND[(5 * p + n_sites) % len(N_IND)] for p in range(n_pops)]
        blocks, want, ploidies = case(rng, n_sites, n_inds)
        twin = host_freqs(blocks, n_inds, ploidies, n_sites, 3)
        assert same_bits(twin, want) and np.isnan(want).sum() == 1
        assert same_bits(device_freqs(eng, blocks, n_inds, ploidies, n_sites), twin), (n_pops, n_sites)


@pytest.mark.parametrize("n_inds", [[70, 64, 3], [129, 17, 1, 2, 513, 64, 65, 20], [70, 70, 1, 2, 3, 16, 17, 63, 20]], ids=["3", "8", "9"])
def test_kernel_equals_the_two_launches_it_replaces(eng, n_inds):
    """Blocks from ``eng.pack2`` of seeded int8 matrices: ``site_pass_packed2(counts)`` + ``site_freqs`` -- one call of
    each for up to eight populations, two for nine."""
    import torch

    from sai_amd.packed_stats import packed_site_freqs

    rng = np.random.default_rng(len(n_inds))
    for n_sites in (65, 200):
        mats = [rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(n_sites, n), p=[0.1, 0.5, 0.25, 0.15]) for n in n_inds]
        mats[0][n_sites // 2] = -1  # nobody called: NaN
        ploidies = [1 + p % 2 for p in range(len(n_inds))]
        pops = [eng.pack2(eng.tile(m)) for m in mats]
        want = []
        for p0 in range(0, len(pops), 8):
            part, pl = pops[p0 : p0 + 8], ploidies[p0 : p0 + 8]
            counts = torch.empty((len(part), n_sites, 2), dtype=torch.int32, device=eng.device)
            eng.site_pass_packed2(part, pl, [], counts=counts)
            want.append(eng.site_freqs(counts, pl))
        assert len(want) == (2 if len(n_inds) == 9 else 1)
        want = torch.cat(want).cpu().numpy()
        got = packed_site_freqs(eng, pops, ploidies).cpu().numpy()
        assert got.shape == (len(n_inds), n_sites) and np.isnan(want[0, n_sites // 2]) and same_bits(got, want), (n_inds, n_sites)
        # and both are the plain quotient
        called = [(m >= 0).sum(axis=1) * pl for m, pl in zip(mats, ploidies)]
        plain = np.stack([np.where(c > 0, np.maximum(m, 0).sum(axis=1) / np.maximum(c, 1), np.nan) for m, c in zip(mats, called)])
        assert same_bits(got, plain)


def random_block(rng, n_sites, n_ind):
    """Any words are a packed2 block as long as the fields of the padding individuals are 0."""
    n_full, rem = n_ind // 64, n_ind % 64
    w_tail = (rem + 15) // 16
    words = rng.integers(0, 1 << 32, size=(-(-n_sites // 64), n_full * 256 + w_tail * 64), dtype=np.uint32)
    tail = words[:, n_full * 256 :].reshape(len(words), 64, w_tail)
    for j in range(w_tail):
        if rem - 16 * j < 16:
            tail[:, :, j] &= np.uint32((1 << (2 * (rem - 16 * j))) - 1)
    return words.reshape(-1).view(np.uint8)


def test_past_the_grid_cap(eng):
    """2 * cap + 3 tiles, the last one partial: every wave takes its third tile, some a fourth.  Every double of the
    13 MB against the host twin."""
    import torch

    cap = STREAM_WAVES_PER_CU * int(torch.cuda.get_device_properties(0).multi_processor_count)
    n_sites = (2 * cap + 3) * 64 - 5
    assert -(-n_sites // 64) == 2 * cap + 3
    rng = np.random.default_rng(11)
    n_inds, ploidies = [3, 65, 17], [2, 1, 2]
    blocks = [random_block(rng, n_sites, n) for n in n_inds]
    twin = host_freqs(blocks, n_inds, ploidies, n_sites, 16)
    assert np.isnan(twin[0]).any() and not np.isnan(twin[1]).all() and len(np.unique(twin[1][~np.isnan(twin[1])])) > 50
    got = device_freqs(eng, blocks, n_inds, ploidies, n_sites)
    assert same_bits(got, twin)


def test_argument_errors_of_the_device_entry_point(eng):
    import torch

    from sai_amd import _ffi, _ffi_packed_stats
    from sai_amd.engine import PackedPop
    from sai_amd.packed_stats import packed_site_freqs

    lib = _ffi_packed_stats.load()
    block = torch.zeros(64 * 4 + 16, dtype=torch.uint8, device=eng.device)
    freqs = torch.full((1, 3), -7.0, dtype=torch.float64, device=eng.device)
    arr = (_ffi.SaiPop * 1)()
    arr[0].tiles, arr[0].n_ind, arr[0].ploidy = block.data_ptr() + 4, 3, 2
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sai_packed2_site_freqs(eng.ctx, 3, 1, arr, C.c_void_p(freqs.data_ptr()), stream) == _ffi.SAI_ERR_ARG
    assert b"population 0: packed block must be a 16-byte aligned device pointer" in lib.sai_last_error()
    arr[0].tiles = None
    assert lib.sai_packed2_site_freqs(eng.ctx, 3, 1, arr, C.c_void_p(freqs.data_ptr()), stream) == _ffi.SAI_ERR_ARG
    assert b"population 0: packed block must be a 16-byte aligned device pointer" in lib.sai_last_error()
    arr[0].tiles, arr[0].ploidy = block.data_ptr(), 0
    assert lib.sai_packed2_site_freqs(eng.ctx, 3, 1, arr, C.c_void_p(freqs.data_ptr()), stream) == _ffi.SAI_ERR_ARG
    assert b"ploidy[0] must be positive" in lib.sai_last_error()
    assert lib.sai_packed2_site_freqs(eng.ctx, 3, 10, arr, C.c_void_p(freqs.data_ptr()), stream) == _ffi.SAI_ERR_ARG
    assert b"n_pops must be 1..9" in lib.sai_last_error()
    torch.cuda.synchronize()
    assert (freqs.cpu().numpy() == -7.0).all()
    empty = PackedPop(torch.empty(0, dtype=torch.uint8, device=eng.device), 0, 5)
    assert tuple(packed_site_freqs(eng, [empty, empty], [2, 1]).shape) == (2, 0)  # n_sites == 0: nothing to do
    with pytest.raises(ValueError, match="cover the same sites"):
        packed_site_freqs(eng, [empty, PackedPop(block[:256], 3, 3)], [2, 2])


# ---- score(..., layout="packed2") --------------------------------------------------------------------------------

OUTGROUP = dict(chr_name="1", win_len=40000, win_step=40000, anc_allele_file="tests/data/test.with.outgroup.anc.alleles",
                config="tests/data/test.with.outgroup.config.yaml", num_workers=1)  # fmt: skip


@pytest.fixture(scope="module")
def outgroup_filesets(tmp_path_factory):
    """tests/data/test.with.outgroup.vcf.gz (1 513 diploid samples, 373 biallelic records, no missing call) as a PLINK 1
    and as a PLINK 2 fileset."""
    tmp = tmp_path_factory.mktemp("outgroup_filesets")
    bed, pgen = str(tmp / "og"), str(tmp / "og_p")
    positions, _ = fileset_from_vcf(DATA / "test.with.outgroup.vcf.gz", bed)
    assert len(positions) == 373
    B.from_bed_fileset(bed, pgen, [FORCED_TYPES[k % len(FORCED_TYPES)] for k in range(len(positions))], len_bytes=2)
    return tmp, bed, pgen


@pytest.mark.parametrize("kind", ["bed", "pgen"])
def test_score_with_outgroup_in_the_packed_layout_matches_the_reference_tsv(eng, in_repo_root, outgroup_filesets, monkeypatch, kind):
    """The reference's own expected table (tests/test_sai.py:92-110), byte for byte, from the 2-bit layout."""
    from sai_amd.engine import PackedPop
    from sai_amd.sai import load_config, score
    from sai_amd.utils.read_data import read_data_device

    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    tmp, bed, pgen = outgroup_filesets
    source = bed + ".bed" if kind == "bed" else pgen + ".pgen"
    out = tmp / kind / "og.tsv"
    score(vcf_file=source, output_file=str(out), layout="packed2", **OUTGROUP)
    assert out.read_bytes() == open("tests/data/test.with.outgroup.res.tsv", "rb").read()
    assert sorted(p.name for p in out.parent.iterdir()) == ["og.tsv"]  # no U / Q: no logs
    # the reader hands the outgroup over in the layout, like every other group
    cfg = load_config(OUTGROUP["config"])
    lists = [cfg.populations.get_population(g) for g in ("ref", "tgt", "src", "outgroup")]
    results, pos_dev = read_data_device(eng, source, "1", cfg.ploidies, *lists, anc_allele_file=OUTGROUP["anc_allele_file"], layout="packed2")
    for group, pop in (("ref", "ref"), ("tgt", "tgt"), ("src", "src"), ("outgroup", "out")):
        gt = results[group][0][pop].GT
        assert isinstance(gt, PackedPop) and gt.n_sites == int(pos_dev.numel()) == 373 and gt.n_ind == len(results[group][1][pop])


def seeded_panel(tmp, sizes, uq, seed, n=400):
    """``n`` sites x the diploid populations of ``sizes`` ({"ref": {name: n_ind}, ...}) as a PLINK 1 and a PLINK 2 fileset,
    an ancestral-allele file that flips about half of the rows, 2 % missing calls in the rows it keeps, and a
    configuration with fd, df, Danc and Dplus (and U + Q with ``uq``).  Returns (bed prefix, pgen prefix, config, anc)."""
    rng = np.random.default_rng(seed)
    p = rng.random(n) ** 2
    cols, samples, lists = [], [], {}
    for group, pops in sizes.items():
        lines = []
        for pop, n_ind in pops.items():
            scale = {"ref": 0.3, "tgt": 1.2, "src": 1.0, "outgroup": 0.1}[group]
            if group == "src":
                cols.append(np.where(rng.random((n, n_ind)) < np.clip(p[:, None] * scale, 0, 1), 2, rng.integers(0, 2, size=(n, n_ind))))
            else:
                cols.append(rng.binomial(2, np.clip(p[:, None] * scale, 0, 1), size=(n, n_ind)))
            names = [f"{pop}_{i}" for i in range(n_ind)]
            samples += names
            lines += [f"{pop}\t{s}\n" for s in names]
        lists[group] = tmp / f"{group}.list"
        lists[group].write_text("".join(lines))
    codes = np.array([HOM_A2, HET, HOM_A1], dtype=np.uint8)[np.concatenate(cols, axis=1)]
    flipped = rng.random(n) < 0.5
    missing = (rng.random(codes.shape) < 0.02) & ~flipped[:, None]  # a missing call in a flipped row does not fit two bits
    codes[missing] = MISSING
    assert missing.any() and flipped.any() and not flipped.all()
    positions = np.cumsum(rng.integers(1, 50, n)).tolist()
    bed, pgen = str(tmp / "panel"), str(tmp / "panel_p")
    write_fileset(bed, chroms=["4"] * n, positions=positions, ids=[f"v{k}" for k in range(n)], a1=["T"] * n, a2=["G"] * n, codes=codes, samples=samples)
    B.from_bed_fileset(bed, pgen, [FORCED_TYPES[k % len(FORCED_TYPES)] for k in range(n)], len_bytes=2)
    anc = tmp / "anc.bed"
    anc.write_text("".join(f"4\t{q - 1}\t{q}\t{'T' if f else 'G'}\n" for q, f in zip(positions, flipped)))  # A1 = T: flipped
    src = "".join(f'      {s}: "=1"\n' if k == 0 else f'      {s}: ">0.2"\n' for k, s in enumerate(sizes["src"]))
    sets = "    ref:\n      R: 0.3\n    tgt:\n      T: {x}\n    src:\n" + src
    cfg = tmp / "panel.yaml"
    cfg.write_text("statistics:\n" + ("  U:\n" + sets.format(x=0.2) + "  Q:\n" + sets.format(x=0.9) if uq else "")
                   + "  fd: true\n  df: true\n  Danc: true\n  Dplus: true\nploidies:\n"
                   + "".join(f"  {g}:\n" + "".join(f"    {pop}: 2\n" for pop in pops) for g, pops in sizes.items())
                   + "populations:\n" + "".join(f'  {g}: "{lists[g]}"\n' for g in sizes))  # fmt: skip
    return bed, pgen, str(cfg), str(anc)


def test_mixed_configuration_writes_the_files_of_the_int8_run(eng, in_repo_root, tmp_path, monkeypatch):
    """U + Q + fd + df + Danc + Dplus, two source populations and an outgroup: TSV and both logs."""
    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    sizes = {"ref": {"R": 70}, "tgt": {"T": 70}, "src": {"S1": 3, "S2": 2}, "outgroup": {"O": 20}}
    bed, pgen, cfg, anc = seeded_panel(tmp_path, sizes, uq=True, seed=31)
    win = (2000, 1000)
    want = score_files(bed + ".bed", cfg, anc, tmp_path / "int8" / "s.tsv", "int8", win)
    assert set(want) == {".tsv", ".U.log", ".Q.log"} and len(want[".tsv"].splitlines()) >= 8
    header = want[".tsv"].decode().splitlines()[0].split("\t")
    assert header[8:] == ["U", "Q", "fd.S1", "fd.S2", "df.S1", "df.S2", "Danc.S1", "Danc.S2", "Dplus.S1", "Dplus.S2"]
    assert len(want[".Q.log"].splitlines()) > 1
    assert score_files(bed + ".bed", cfg, anc, tmp_path / "bed" / "s.tsv", "packed2", win) == want
    assert score_files(pgen + ".pgen", cfg, anc, tmp_path / "pgen_int8" / "s.tsv", "int8", win) == want
    assert score_files(pgen + ".pgen", cfg, anc, tmp_path / "pgen" / "s.tsv", "packed2", win) == want


def test_seven_sources_take_two_groups(eng, in_repo_root, tmp_path, monkeypatch):
    """Seven source populations and an outgroup, ABBA-BABA statistics only: no scorer, and the sources go through the
    frequency kernel six and one at a time (the U / Q limit of six sources does not apply)."""
    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    sizes = {"ref": {"R": 70}, "tgt": {"T": 65}, "src": {f"S{k}": 1 + k % 3 for k in range(7)}, "outgroup": {"O": 17}}
    bed, pgen, cfg, anc = seeded_panel(tmp_path, sizes, uq=False, seed=32)
    win = (2000, 1000)
    want = score_files(bed + ".bed", cfg, anc, tmp_path / "int8" / "s.tsv", "int8", win)
    assert set(want) == {".tsv"} and len(want[".tsv"].splitlines()) >= 8
    assert len(want[".tsv"].decode().splitlines()[0].split("\t")) == 8 + 4 * 7
    assert score_files(bed + ".bed", cfg, anc, tmp_path / "bed" / "s.tsv", "packed2", win) == want
    assert score_files(pgen, cfg, anc, tmp_path / "pgen" / "s.tsv", "packed2", win) == want
