"""PLINK 1 ``.bed`` rows decoded straight into the packed2 layout on the GPU: ``sai_bed_pack2`` against the host decoder
byte for byte and against ``pack2(tile(.))`` of the int8 decoder, the streaming reader ``load_packed_device`` against
the int8 reader, its memory, and ``score(..., layout="packed2")`` against the int8 run (byte-identical files)."""

import ctypes as C
import shutil

import numpy as np
import pytest

from test_bed_pack2_cpu import N_IND, N_SITES, column_lists, cuts_of, pack_host, pack_numpy, site_words, tile_words
from test_plink_cpu import random_case
from test_plink_device import seeded_block

pytestmark = pytest.mark.gpu


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


class DeviceCall:
    """The device copies of one decode problem; ``run`` is one ``sai_bed_pack2`` call into the block."""

    def __init__(self, eng, rows, row_bytes, rib, flip, n_cols, cols, first_col, ploidy, n_sites, fill=0xA5):
        import torch

        self.eng, self.n = eng, (len(rows) // row_bytes if row_bytes else 0, row_bytes, n_cols, len(cols), first_col, ploidy, n_sites)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
        self.rows, self.rib, self.flip, self.cols = dev(rows), dev(rib), dev(flip), dev(cols)
        self.packed = torch.full((-(-n_sites // 64) * tile_words(len(cols)) * 4,), fill, dtype=torch.uint8, device=eng.device)
        self.status = torch.full((len(rib),), -5, dtype=torch.int32, device=eng.device)
        self.unfit = torch.full((len(rib),), -5, dtype=torch.int32, device=eng.device)

    def run(self, lo, hi):
        import torch

        from sai_amd import _ffi, _ffi_packed_ingest

        lib, eng = _ffi_packed_ingest.load(), self.eng
        n_batch, row_bytes, n_cols, n_ind, first_col, ploidy, n_sites = self.n
        at = lambda t, k: C.c_void_p(t.data_ptr() + k * t.element_size())  # noqa: E731
        _ffi.check(lib.sai_bed_pack2(eng.ctx, eng._ptr(self.rows), n_batch, row_bytes, hi - lo, at(self.rib, lo), at(self.flip, lo), n_cols,
                                     n_ind, None if first_col >= 0 else eng._ptr(self.cols), first_col, ploidy,
                                     C.c_void_p(self.packed.data_ptr()), n_sites, lo, at(self.status, lo), at(self.unfit, lo),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
        torch.cuda.synchronize()
        return self.packed.cpu().numpy()


def check_against_host(eng, rows, row_bytes, rib, flip, n_cols, cols, first_col, ploidy, where, cuts=None):
    """The kernel's block, status and unfit equal the host decoder's; a call leaves every word of other sites alone."""
    n_sites, n_ind = len(rib), len(cols)
    want = np.zeros(-(-n_sites // 64) * tile_words(n_ind) * 4, dtype=np.uint8)
    want_st, want_uf = pack_host(rows, row_bytes, rib, flip, n_cols, cols, first_col, ploidy, want, n_sites, 0)
    call = DeviceCall(eng, rows, row_bytes, rib, flip, n_cols, cols, first_col, ploidy, n_sites)
    got = call.packed.cpu().numpy()
    for lo, hi in cuts or cuts_of(n_sites):
        before, got = got, call.run(lo, hi)
        mine = np.zeros(want.size // 4, dtype=bool)
        mine[site_words(n_sites, n_ind, lo, hi)] = True
        assert np.array_equal(got.view(np.uint32)[~mine], before.view(np.uint32)[~mine]), (where, lo, hi)  # the sentinel, or earlier calls
    assert np.array_equal(got, want), where
    assert np.array_equal(call.status.cpu().numpy(), want_st) and np.array_equal(call.unfit.cpu().numpy(), want_uf), where
    return want, want_st, want_uf


@pytest.mark.parametrize("n_ind", N_IND)
def test_kernel_equals_host_decoder(eng, n_ind):
    rng = np.random.default_rng(900 + n_ind)
    n_cols = n_ind + 9
    row_bytes = (n_cols + 3) // 4
    seen = set()
    for n_sites in N_SITES:
        n_batch = n_sites + 3
        rows = rng.integers(0, 256, size=n_batch * row_bytes, dtype=np.uint8)  # any byte string is a valid row
        rib = rng.permutation(n_batch)[:n_sites].astype(np.int32)
        flip = rng.integers(0, 2, size=n_sites).astype(np.uint8)
        for first_col, cols in column_lists(n_ind, n_cols, rng):
            for ploidy in (1, 2):
                _, st, uf = check_against_host(eng, rows, row_bytes, rib, flip, n_cols, cols, first_col, ploidy, (n_ind, n_sites, first_col, ploidy))
                seen |= {"het"} if st.any() else set()
                seen |= {"unfit"} if uf.any() else set()
    assert seen == {"het", "unfit"}


@pytest.mark.parametrize("n_cols,n_ind,run", [(2002, 2002, True), (10007, 300, False), (2002, 1800, True)])
def test_kernel_equals_host_decoder_on_wide_rows(eng, n_cols, n_ind, run):
    """2 002 of 2 002 columns (32 groups: several runs of groups per tile), 300 permuted columns of 10 007, and a run
    that starts inside a byte; the rows of the batch are used out of order and some of them twice."""
    rng = np.random.default_rng(n_cols + n_ind)
    row_bytes = (n_cols + 3) // 4
    n_batch, n_sites = 41, 150
    rows = rng.integers(0, 256, size=n_batch * row_bytes, dtype=np.uint8)
    rib = rng.integers(0, n_batch, size=n_sites).astype(np.int32)
    flip = rng.integers(0, 2, size=n_sites).astype(np.uint8)
    first_col = (n_cols - n_ind) // 2 if run else -1
    cols = np.arange(first_col, first_col + n_ind, dtype=np.int32) if run else rng.permutation(n_cols)[:n_ind].astype(np.int32)
    for ploidy in (1, 2):
        check_against_host(eng, rows, row_bytes, rib, flip, n_cols, cols, first_col, ploidy, (n_cols, n_ind, ploidy), cuts=[(0, 70), (70, 150)])
    # indices out of range: flagged, written as 0, never dereferenced -- as the host decoder says
    rib[3], rib[77] = -1, n_batch
    if not run:
        cols[5], cols[-1] = n_cols, -3
    _, st, _ = check_against_host(eng, rows, row_bytes, rib, flip, n_cols, cols, first_col, 2, (n_cols, n_ind, "bad"))
    assert st[3] == st[77] == 0x7FFFFFFF and (run or (st == 0x7FFFFFFF).all())


def int8_dosages(rows, row_bytes, rib, flip, n_cols, cols, ploidy):
    from sai_amd import _ffi, _ffi_plink

    lib = _ffi_plink.load()
    out = np.empty((len(rib), len(cols)), dtype=np.int8)
    st = np.empty(len(rib), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pl = np.full(len(cols), ploidy, dtype=np.int32)
    _ffi.check(lib.sai_plink_decode_host(p(rows), len(rows) // row_bytes, row_bytes, len(rib), p(rib), p(flip), n_cols, len(cols), p(cols),
                                         p(pl), p(out), p(st), 3))  # fmt: skip
    return out, st


@pytest.mark.parametrize("n_ind,n_sites", [(17, 65), (130, 130), (2002, 200)])
def test_kernel_equals_pack2_of_the_int8_decoder(eng, n_ind, n_sites):
    """The second, independent expectation: ``eng.pack2(eng.tile(d))`` with d the int8 block of ``sai_plink_decode_host``
    (and the numpy statement of the layout) -- where every dosage fits, i.e. kept rows at ploidy 2 and any row at ploidy 1."""
    rng = np.random.default_rng(n_ind)
    n_cols = n_ind + 6
    row_bytes = (n_cols + 3) // 4
    rows = rng.integers(0, 256, size=(n_sites + 2) * row_bytes, dtype=np.uint8)
    rib = rng.permutation(n_sites + 2)[:n_sites].astype(np.int32)
    cols = np.arange(3, 3 + n_ind, dtype=np.int32)
    for ploidy, flip in ((2, np.zeros(n_sites, np.uint8)), (1, rng.integers(0, 2, size=n_sites).astype(np.uint8))):
        d, _ = int8_dosages(rows, row_bytes, rib, flip, n_cols, cols, ploidy)
        assert d.max() <= 2
        want = eng.pack2(eng.tile(d)).data.cpu().numpy()
        assert np.array_equal(want, pack_numpy(np.where(d < 0, 3, d).astype(np.uint8)))
        call = DeviceCall(eng, rows, row_bytes, rib, flip, n_cols, cols, 3, ploidy, n_sites)
        assert np.array_equal(call.run(0, n_sites), want), (n_ind, n_sites, ploidy)


def populations_of(request):
    """The request of a random case as populations: the diploid samples in two of them, the haploid ones in a third."""
    two = [s for s, p in request if p == 2]
    one = [s for s, p in request if p == 1]
    return [(names, ploidy) for names, ploidy in ((two[: len(two) // 2 + 1], 2), (two[len(two) // 2 + 1 :], 2), (one, 1)) if names]


def test_streaming_reader_equals_pack2_of_the_int8_reader(eng, tmp_path):
    from sai_amd.utils import plink

    compared = refused = 0
    for seed in (3, 4, 11):
        case = random_case(seed, tmp_path)
        pops = populations_of(case["request"])
        here = case["positions"]
        row_bytes = (len(case["samples"]) + 3) // 4
        for anc in (None, case["anc"]):
            for start, end in [(None, None), (here[2], here[-2])]:
                dosages = [plink.load_dosage(case["prefix"], "7", names, [ploidy] * len(names), start, end, anc) for names, ploidy in pops]
                fits = all(int(d[1].max(initial=0)) <= 2 for d in dosages)
                for cap in (3 * row_bytes + 1, 4096, None):  # three rows per batch, a few KiB, one batch
                    if not fits:  # a missing call in a flipped diploid row: dosage 4
                        with pytest.raises(ValueError, match=r"missing call of sample s\d+ at variant rs\d+_\d+ \(position \d+\) in a row flipped"):
                            plink.load_packed_device(eng, case["prefix"], "7", pops, start, end, anc, buffer_bytes=cap)
                        refused += 1
                        continue
                    pos, packed, n_matched, n_anc = plink.load_packed_device(eng, case["prefix"] + ".bed", "7", pops, start, end, anc, buffer_bytes=cap)
                    assert pos.dtype == np.int32 and pos.tolist() == dosages[0][0].tolist() and (n_matched, n_anc) == dosages[0][2:]
                    for (names, _), got, (_, d, _, _) in zip(pops, packed, dosages):
                        assert (got.n_sites, got.n_ind) == d.shape
                        want = eng.pack2(eng.tile(d)).data.cpu().numpy() if d.size else np.zeros(0, np.uint8)
                        assert np.array_equal(got.data.cpu().numpy(), want), (seed, anc, start, cap)
                        compared += 1
    assert compared >= 18 and refused


@pytest.fixture(scope="module")
def block(tmp_path_factory):
    """The seeded 20 000-site block of test_plink_device with its configuration reduced to U + Q, a copy of the fileset
    without missing calls, and an ancestral-allele file that flips about half of the sites."""
    tmp = tmp_path_factory.mktemp("packed_block")
    _, prefix, cfg = seeded_block(tmp)
    uq = tmp / "uq.yaml"
    uq.write_text(open(cfg).read().replace("  DD: true\n", ""))
    clean = str(tmp / "clean")
    for ext in (".bim", ".fam"):
        shutil.copy(prefix + ext, clean + ext)
    bed = np.fromfile(prefix + ".bed", dtype=np.uint8)
    body = bed[3:]
    body |= (body & 0x55 & ~(body >> 1)) << 1  # every missing call (01) becomes A2 A2 (11)
    bed.tofile(clean + ".bed")
    positions = [int(line.split()[3]) for line in open(prefix + ".bim")]
    rng = np.random.default_rng(4)
    anc = tmp / "anc.bed"
    anc.write_text("".join(f"4\t{p - 1}\t{p}\t{rng.choice(['T', 'G'])}\n" for p in positions))  # A1 = T: flipped; A2 = G: kept
    return dict(tmp=tmp, prefix=prefix, clean=clean, cfg=str(uq), anc=str(anc), n_rows=len(positions))


POPS = [([f"r{i}" for i in range(60)], 2), ([f"t{i}" for i in range(60)], 2), ([f"n{i}" for i in range(2)], 2)]


def test_the_int8_block_never_exists(eng, block):
    import torch

    from sai_amd.utils import plink

    plink.release_buffers(eng)  # the staging counts too
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pos, packed, _, _ = plink.load_packed_device(eng, block["prefix"], "4", POPS, buffer_bytes=64 << 10)
    rise = torch.cuda.max_memory_allocated() - base
    n_rows, n_slots = len(pos), sum(len(names) for names, _ in POPS)
    print(f"rise of max_memory_allocated: {rise} bytes; int8 block: {n_rows * n_slots} bytes")
    assert (n_rows, n_slots) == (20000, 122) and rise < n_rows * n_slots
    d = plink.load_dosage(block["prefix"], "4", POPS[1][0], [2] * 60)[1]
    assert np.array_equal(packed[1].data.cpu().numpy(), pack_numpy(np.where(d < 0, 3, d).astype(np.uint8)))
    plink.release_buffers(eng)


def score_files(source, cfg, anc, out, layout, win=(5000, 2500)):
    from sai_amd.sai import score

    score(vcf_file=source, chr_name="4", win_len=win[0], win_step=win[1], anc_allele_file=anc, output_file=str(out), config=cfg,
          num_workers=1, layout=layout)  # fmt: skip
    return {p.name[len(out.stem) :]: p.read_bytes() for p in out.parent.glob(out.stem + "*")}


def test_score_packed2_writes_the_files_of_the_int8_run(eng, in_repo_root, block, monkeypatch):
    from sai_amd import sai as sai_mod

    tmp, prefix, cfg = block["tmp"], block["prefix"], block["cfg"]
    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    want = score_files(prefix + ".bed", cfg, None, tmp / "int8" / "s.tsv", "int8")
    assert set(want) == {".tsv", ".U.log", ".Q.log"} and len(want[".tsv"].splitlines()) > 150
    assert len(want[".U.log"].splitlines()) > 1 and len(want[".Q.log"].splitlines()) > 1
    assert score_files(prefix + ".bed", cfg, None, tmp / "one" / "s.tsv", "packed2") == want
    monkeypatch.setenv("SAI_AMD_LAYOUT", "packed2")  # the environment's default, through the bare prefix
    assert score_files(prefix, cfg, None, tmp / "env" / "s.tsv", None) == want
    monkeypatch.delenv("SAI_AMD_LAYOUT")
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "250000")  # the .bed is 620 003 bytes and stays 620 003: three chunks
    assert sai_mod.chunks_for_memory(prefix + ".bed", "packed2") == 3
    assert score_files(prefix + ".bed", cfg, None, tmp / "three" / "s.tsv", "packed2") == want


def test_score_packed2_with_ancestral_alleles(eng, in_repo_root, block, monkeypatch):
    """Flipped rows: the files of the int8 run on the copy without missing calls; with the 1 % missing calls a flipped row
    holds a dosage of 4, which is the reader's error.  The host decoder says beforehand which case is which."""
    from sai_amd.utils import plink

    tmp, cfg, anc = block["tmp"], block["cfg"], block["anc"]
    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    pos, blocks, n_matched, n_anc = plink.load_packed(block["clean"], "4", POPS, anc_allele_file=anc)  # no unfit row: no error
    assert len(pos) == n_matched == n_anc == block["n_rows"]
    with pytest.raises(ValueError, match="its dosage is 4"):  # at least one unfit row
        plink.load_packed(block["prefix"], "4", POPS, anc_allele_file=anc)
    want = score_files(block["clean"] + ".bed", cfg, anc, tmp / "anc_int8" / "s.tsv", "int8")
    assert len(want[".tsv"].splitlines()) > 150
    assert score_files(block["clean"] + ".bed", cfg, anc, tmp / "anc_one" / "s.tsv", "packed2") == want
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "250000")
    assert score_files(block["clean"], cfg, anc, tmp / "anc_three" / "s.tsv", "packed2") == want
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES")
    with pytest.raises(ValueError, match=r"block.bed: missing call of sample [rtn]\d+ at variant v\d+ \(position \d+\) in a row flipped by the "
                       r"ancestral allele: its dosage is 4, which the 2-bit layout cannot hold; read this fileset with --layout int8"):
        score_files(block["prefix"] + ".bed", cfg, anc, tmp / "anc_unfit" / "s.tsv", "packed2")
