"""PLINK 2 ``.pgen`` records decoded straight into the packed2 layout on the GPU: ``sai_pgen_pack2`` against the host
decoder byte for byte and against ``pack2(tile_columns(.))`` of the int8 kernel, rows wider than one LDS window, the
streaming reader ``load_packed_device`` against the int8 reader, its memory, and ``score(..., layout="packed2")``
against the int8 run of the same ``.pgen`` and of the ``.bed`` it was made from (byte-identical files)."""

import ctypes as C

import numpy as np
import pytest

import pgen_builder as B
from test_bed_pack2_cpu import pack_numpy, site_words, tile_words
from test_bed_pack2_device import POPS, block, eng, score_files  # noqa: F401 -- `block` and `eng` are fixtures
from test_pgen_cpu import ALL_TYPES, BAD_RECORD, random_matrix, random_types, tables_of
from test_pgen_pack2_cpu import N_IND, N_SITES, READER_SEEDS, column_lists, pack_host, packed_of, reader_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def cuts_of(n_sites):
    """Calls cut at out_row0 = 0, 37 and 64: two calls complete the first tile."""
    edges = sorted({0, min(37, n_sites), min(64, n_sites), n_sites})
    return list(zip(edges, edges[1:]))


class DeviceCall:
    """The device copies of one decode problem; ``run`` is one ``sai_pgen_pack2`` call into the block."""

    def __init__(self, eng, data, rec, base, flip, sample_ct, cols, first_col, ploidy, fill=0xA5):
        import torch

        dev = lambda a, t: torch.from_numpy(np.array(a, dtype=t)).to(eng.device)  # noqa: E731 -- a writable copy
        self.eng, self.n = eng, (len(data), sample_ct, len(cols), first_col, ploidy, len(rec))
        self.data = dev(np.frombuffer(bytes(data), dtype=np.uint8), np.uint8)
        self.rec, self.base, self.flip, self.cols = dev(rec, np.int64), dev(base, np.int64), dev(flip, np.uint8), dev(cols, np.int32)
        self.packed = torch.full((-(-len(rec) // 64) * tile_words(len(cols)) * 4,), fill, dtype=torch.uint8, device=eng.device)
        self.status = torch.full((len(rec),), -5, dtype=torch.int32, device=eng.device)
        self.unfit = torch.full((len(rec),), -5, dtype=torch.int32, device=eng.device)

    def run(self, lo, hi):
        import torch

        from sai_amd import _ffi, _ffi_pgen_packed

        lib, eng = _ffi_pgen_packed.load(), self.eng
        n_bytes, sample_ct, n_ind, first_col, ploidy, n_sites = self.n
        at = lambda t, k: C.c_void_p(t.data_ptr() + k * t.element_size())  # noqa: E731
        _ffi.check(lib.sai_pgen_pack2(eng.ctx, eng._ptr(self.data), n_bytes, hi - lo, at(self.rec, 3 * lo), at(self.base, 3 * lo), at(self.flip, lo),
                                      sample_ct, n_ind, None if first_col >= 0 else eng._ptr(self.cols), first_col, ploidy,
                                      C.c_void_p(self.packed.data_ptr()), n_sites, lo, at(self.status, lo), at(self.unfit, lo),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
        torch.cuda.synchronize()
        return self.packed.cpu().numpy()


def check_against_host(eng, data, rec, base, flip, sample_ct, cols, first_col, ploidy, where, cuts=None):
    """The kernel's block, status and unfit equal the host decoder's, written whole and in cut calls; a call leaves every
    word of other sites alone."""
    n_sites, n_ind = len(rec), len(cols)
    want = np.zeros(-(-n_sites // 64) * tile_words(n_ind) * 4, dtype=np.uint8)
    want_st, want_uf = pack_host(data, rec, base, flip, sample_ct, cols, first_col, ploidy, want, n_sites, 0)
    call = DeviceCall(eng, data, rec, base, flip, sample_ct, cols, first_col, ploidy)
    assert np.array_equal(call.run(0, n_sites), want), (where, "whole")
    assert np.array_equal(call.status.cpu().numpy(), want_st) and np.array_equal(call.unfit.cpu().numpy(), want_uf), (where, "whole")
    cuts = cuts or cuts_of(n_sites)
    if len(cuts) > 1:
        call = DeviceCall(eng, data, rec, base, flip, sample_ct, cols, first_col, ploidy)
        got = call.packed.cpu().numpy()
        for lo, hi in cuts:
            before, got = got, call.run(lo, hi)
            mine = np.zeros(want.size // 4, dtype=bool)
            mine[site_words(n_sites, n_ind, lo, hi)] = True
            assert np.array_equal(got.view(np.uint32)[~mine], before.view(np.uint32)[~mine]), (where, lo, hi)  # the sentinel, or earlier calls
        assert np.array_equal(got, want), (where, "cut")
        assert np.array_equal(call.status.cpu().numpy(), want_st) and np.array_equal(call.unfit.cpu().numpy(), want_uf), (where, "cut")
    return want, want_st, want_uf


def typed_case(rng, n_sites, sample_ct):
    """A matrix and forced record types of every kind; the rows at which the calls are cut (37, 64) differ from a base
    that lies before them, so the base of a call's first row is no row of the call."""
    matrix = random_matrix(rng, n_sites, sample_ct)
    types = random_types(rng, n_sites)
    for cut, kind, base_kind in ((37, 2, 1), (64, 3, 4)):
        if cut < n_sites:
            types[cut - 2 : cut + 1] = [base_kind, 2, kind]
    data, table = B.build_pgen(matrix, types, wide_types=bool(n_sites & 1), len_bytes=2)
    return data, table


@pytest.mark.parametrize("n_ind", N_IND)
def test_kernel_equals_host_decoder(eng, n_ind):
    rng = np.random.default_rng(1100 + n_ind)
    sample_ct = n_ind + 9
    seen, kinds, split_bases = set(), set(), 0
    for n_sites in N_SITES:
        data, table = typed_case(rng, n_sites, sample_ct)
        kinds |= {t[2] & 7 for t in table}
        split_bases += sum(1 for cut in (37, 64) if cut < n_sites and 0 <= table[cut][3] < cut)
        rec, base = tables_of(table)
        if n_sites > 2:  # one reserved and one truncated record among them: BAD_RECORD, zeros, and the neighbours intact
            rec[1] = [rec[1][0], rec[1][1], 5]
            rec[n_sites - 1][1] = max(0, rec[n_sites - 1][1] - 1) if (rec[n_sites - 1][2] & 7) == 0 else 0
        flip = rng.integers(0, 2, size=n_sites).astype(np.uint8)  # flipped and unflipped rows mixed
        for first_col, cols in column_lists(n_ind, sample_ct, rng):
            for ploidy in (1, 2):
                _, st, uf = check_against_host(eng, data, rec, base, flip, sample_ct, cols, first_col, ploidy, (n_ind, n_sites, first_col, ploidy))
                seen |= {"het"} if ((st > 0) & (st < BAD_RECORD)).any() else set()
                seen |= {"unfit"} if uf.any() else set()
                seen |= {"bad"} if (st == BAD_RECORD).any() else set()
    assert seen == {"het", "unfit", "bad"} and kinds == set(ALL_TYPES) and split_bases >= 4


def test_kernel_on_many_groups_and_bad_columns(eng):
    """More than 64 groups on the general path (a lane takes a second group from the same LDS window), a run that starts
    deep inside the row, and columns outside the samples: flagged, written as 0, never dereferenced."""
    rng = np.random.default_rng(31)
    sample_ct, n_sites = 300, 70
    data, table = typed_case(rng, n_sites, sample_ct)
    rec, base = tables_of(table)
    flip = rng.integers(0, 2, size=n_sites).astype(np.uint8)
    many = rng.integers(0, sample_ct, size=4200).astype(np.int32)
    for ploidy in (1, 2):
        check_against_host(eng, data, rec, base, flip, sample_ct, many, -1, ploidy, ("many", ploidy))
        check_against_host(eng, data, rec, base, flip, sample_ct, np.arange(157, 300, dtype=np.int32), 157, ploidy, ("deep run", ploidy))
    cols = rng.integers(0, sample_ct, size=130).astype(np.int32)
    cols[[0, 77, 129]] = [sample_ct, -1, 1 << 30]
    _, st, _ = check_against_host(eng, data, rec, base, flip, sample_ct, cols, -1, 2, "bad columns")
    assert (st == 0x7FFFFFFF).all()


def int8_block(eng, data, rec, base, flip, sample_ct, ploidy):
    """The device int8 [record][sample] block of ``sai_pgen_decode``, every sample at ``ploidy``."""
    import torch

    from sai_amd import _ffi, _ffi_pgen

    lib = _ffi_pgen.load()
    dev = lambda a, t: torch.from_numpy(np.array(a, dtype=t)).to(eng.device)  # noqa: E731 -- a writable copy
    d_data, d_rec, d_base, d_flip = dev(np.frombuffer(bytes(data), dtype=np.uint8), np.uint8), dev(rec, np.int64), dev(base, np.int64), dev(flip, np.uint8)
    out = torch.empty((len(rec), sample_ct), dtype=torch.int8, device=eng.device)
    status = torch.empty((len(rec),), dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_pgen_decode(eng.ctx, eng._ptr(d_data), len(data), len(rec), eng._ptr(d_rec), eng._ptr(d_base), eng._ptr(d_flip), sample_ct,
                                   sample_ct, None, 0, None, ploidy, C.c_void_p(out.data_ptr()), 0, eng._ptr(status),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n_ind,n_sites", [(17, 65), (130, 130), (2002, 200)])
def test_kernel_equals_pack2_of_the_int8_kernel(eng, n_ind, n_sites):
    """The second, independent expectation: ``eng.pack2(eng.tile_columns(d, cols))`` with d the int8 block of
    ``sai_pgen_decode`` -- where every dosage fits, i.e. kept rows at ploidy 2 and any row at ploidy 1."""
    rng = np.random.default_rng(n_ind)
    sample_ct = n_ind + 6
    matrix = random_matrix(rng, n_sites, sample_ct)
    data, table = B.build_pgen(matrix, random_types(rng, n_sites), wide_types=True, len_bytes=4)
    rec, base = tables_of(table)
    runs = [(3, np.arange(3, 3 + n_ind, dtype=np.int32)), (-1, rng.permutation(sample_ct)[:n_ind].astype(np.int32))]
    for ploidy, flip in ((2, np.zeros(n_sites, np.uint8)), (1, rng.integers(0, 2, size=n_sites).astype(np.uint8))):
        d = int8_block(eng, data, rec, base, flip, sample_ct, ploidy)
        assert int(d.max()) <= 2
        for first_col, cols in runs:
            want = eng.pack2(eng.tile_columns(d, cols.tolist())).data.cpu().numpy()
            picked = d.cpu().numpy()[:, cols]
            assert np.array_equal(want, packed_of(picked))
            call = DeviceCall(eng, data, rec, base, flip, sample_ct, cols, first_col, ploidy)
            assert np.array_equal(call.run(0, n_sites), want), (n_ind, n_sites, ploidy, first_col)


def test_rows_wider_than_one_lds_window(eng):
    """16 384 + 600 samples: the smallest shape with two windows (a row is 4.2 KiB).  All columns from column 3 on (266
    groups: the fast path's second window, a group astride sample 16 384), 300 and 4 200 permuted columns drawn from
    both windows (the general path: one and two rounds of groups).  Difflists of more than 64 entries whose groups
    cross sample 16 384, dense and one-bit rows, rows that differ from a base, one damaged record among them."""
    rng = np.random.default_rng(16384)
    n, n_sites = 16384 + 600, 70
    matrix = np.zeros((n_sites, n), dtype=np.uint8)
    types = []
    for r in range(n_sites):
        style = r % 7
        if style == 0:  # dense
            matrix[r] = rng.integers(0, 4, n)
            types.append(0)
            continue
        if style == 1:  # one bit per sample and a difflist
            matrix[r] = np.where(rng.random(n) < 0.3, 2, 0)
            types.append(1)
        elif style in (2, 3):  # differs from the row before / from its 0 <-> 2 exchange
            matrix[r] = matrix[r - 1] if style == 2 else B.swap02(matrix[r - 1])
            types.append(style)
        else:  # a constant and a difflist
            matrix[r] = {4: 0, 5: 2, 6: 3}[style]
            types.append({4: 4, 5: 6, 6: 7}[style])
        where = np.sort(rng.choice(np.arange(16384 - 700, n), size=int(rng.integers(130, 400)), replace=False))
        where = np.union1d(where, rng.integers(0, n, size=20))  # two to seven groups, one of them across sample 16 384
        matrix[r, where] = (matrix[r, where] + rng.integers(1, 4, len(where))) % 4
    data, table = B.build_pgen(matrix, types, wide_types=True, len_bytes=2)
    assert all((t[2] & 7) == want for t, want in zip(table, types))
    rec, base = tables_of(table)
    victim = 41  # a type 7 record, its difflist cut short
    assert types[victim] == 7
    rec[victim][1] -= 3
    flip = rng.integers(0, 2, size=n_sites).astype(np.uint8)
    for first_col, cols in ((3, np.arange(3, n, dtype=np.int32)), (-1, rng.permutation(n)[:300].astype(np.int32)),
                            (-1, rng.integers(0, n, size=4200).astype(np.int32))):  # fmt: skip
        assert first_col >= 0 or ((cols < 16384).any() and (cols >= 16384).any())
        for ploidy in (2, 1):
            _, st, uf = check_against_host(eng, data, rec, base, flip, n, cols, first_col, ploidy, (len(cols), ploidy))
            assert st[victim] == BAD_RECORD and (st == BAD_RECORD).sum() == 1 and (uf.any() == (ploidy == 2))


def test_streaming_reader_equals_pack2_of_the_int8_reader(eng, tmp_path):
    from sai_amd.utils import pgen

    compared = flipped = refused = 0
    for seed in READER_SEEDS:
        case, prefix, longest, asks = reader_cases(seed, tmp_path)
        for pops, anc, start, end, dosages in asks:
            fits = all(int(d[1].max(initial=0)) <= 2 for d in dosages)
            for cap in (2 * longest, 4096, None):  # a record or two per batch (a base and its rows part), 4 KiB, one batch
                if not fits:  # a missing call in a flipped diploid row: dosage 4 -- where the host reader says so
                    with pytest.raises(ValueError, match=r"missing call of sample s\d+ at variant rs\d+_\d+ \(position \d+\) in a row flipped") as host:
                        pgen.load_packed(prefix, "7", pops, start, end, anc, buffer_bytes=cap)
                    with pytest.raises(ValueError) as device:
                        pgen.load_packed_device(eng, prefix, "7", pops, start, end, anc, buffer_bytes=cap)
                    assert str(device.value) == str(host.value) and str(host.value).endswith("read this fileset with --layout int8")
                    refused += 1
                    continue
                pos, packed, n_matched, n_anc = pgen.load_packed_device(eng, prefix + ".pgen", "7", pops, start, end, anc, buffer_bytes=cap)
                assert pos.dtype == np.int32 and pos.tolist() == dosages[0][0].tolist() and (n_matched, n_anc) == dosages[0][2:]
                for got, (_, d, _, _) in zip(packed, dosages):
                    assert (got.n_sites, got.n_ind) == d.shape
                    want = eng.pack2(eng.tile(d)).data.cpu().numpy() if d.size else np.zeros(0, np.uint8)
                    assert np.array_equal(got.data.cpu().numpy(), want), (seed, anc, start, cap)
                    compared += 1
                    flipped += int(anc is not None and d.size > 0)
    assert compared >= 18 and refused >= 1 and flipped
    pgen.release_buffers(eng)


FORCED_TYPES = (0, 4, 2, 1, 3, 6, 2, 7)  # every record type in turn: one encoding per row keeps the writer quick


@pytest.fixture(scope="module")
def pblock(block):
    """The seeded 20 000-site block of test_bed_pack2_device as PLINK 2 filesets: the one with 1 % missing calls and the
    copy without."""
    n = block["n_rows"]
    types = [FORCED_TYPES[k % len(FORCED_TYPES)] for k in range(n)]
    out = dict(block)
    for key in ("prefix", "clean"):
        out["p" + key] = block[key] + "_p"
        table = B.from_bed_fileset(block[key], out["p" + key], types, len_bytes=2)
        assert {t[2] & 7 for t in table} == set(ALL_TYPES)
    return out


def test_the_int8_block_never_exists(eng, pblock):
    import torch

    from sai_amd.utils import filesets, pgen

    filesets.release_buffers(eng)  # the staging counts too
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pos, packed, _, _ = pgen.load_packed_device(eng, pblock["pprefix"], "4", POPS, buffer_bytes=64 << 10)
    rise = torch.cuda.max_memory_allocated() - base
    n_rows, n_slots = len(pos), sum(len(names) for names, _ in POPS)
    print(f"rise of max_memory_allocated: {rise} bytes; int8 block: {n_rows * n_slots} bytes")
    assert (n_rows, n_slots) == (20000, 122) and rise < n_rows * n_slots
    d = pgen.load_dosage(pblock["pprefix"], "4", POPS[1][0], [2] * 60)[1]
    assert np.array_equal(packed[1].data.cpu().numpy(), pack_numpy(np.where(d < 0, 3, d).astype(np.uint8)))
    pgen.release_buffers(eng)


def test_score_packed2_writes_the_files_of_the_int8_run(eng, in_repo_root, pblock, monkeypatch):
    from sai_amd import sai as sai_mod

    tmp, prefix, pprefix, cfg = pblock["tmp"], pblock["prefix"], pblock["pprefix"], pblock["cfg"]
    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    want = score_files(pprefix + ".pgen", cfg, None, tmp / "p_int8" / "s.tsv", "int8")
    assert set(want) == {".tsv", ".U.log", ".Q.log"} and len(want[".tsv"].splitlines()) > 150
    assert len(want[".U.log"].splitlines()) > 1 and len(want[".Q.log"].splitlines()) > 1
    assert score_files(prefix + ".bed", cfg, None, tmp / "p_bed_int8" / "s.tsv", "int8") == want  # the .bed it was made from
    assert score_files(pprefix + ".pgen", cfg, None, tmp / "p_one" / "s.tsv", "packed2") == want
    monkeypatch.setenv("SAI_AMD_LAYOUT", "packed2")  # the environment's default, through the bare prefix
    assert score_files(pprefix, cfg, None, tmp / "p_env" / "s.tsv", None) == want
    monkeypatch.delenv("SAI_AMD_LAYOUT")
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "250000")  # 20 000 variants x ceil(122 / 4) = 620 000 bytes: three chunks
    assert sai_mod.chunks_for_memory(pprefix + ".pgen", "packed2") == 3
    assert score_files(pprefix + ".pgen", cfg, None, tmp / "p_three" / "s.tsv", "packed2") == want


def test_score_packed2_with_ancestral_alleles(eng, in_repo_root, pblock, monkeypatch):
    """Flipped rows: the files of the int8 run on the copy without missing calls; with the 1 % missing calls a flipped row
    holds a dosage of 4, which is the reader's error.  The host decoder says beforehand which case is which."""
    from sai_amd.utils import pgen

    tmp, cfg, anc = pblock["tmp"], pblock["cfg"], pblock["anc"]
    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    pos, blocks, n_matched, n_anc = pgen.load_packed(pblock["pclean"], "4", POPS, anc_allele_file=anc)  # no unfit row: no error
    assert len(pos) == n_matched == n_anc == pblock["n_rows"]
    with pytest.raises(ValueError, match="its dosage is 4"):  # at least one unfit row
        pgen.load_packed(pblock["pprefix"], "4", POPS, anc_allele_file=anc)
    want = score_files(pblock["pclean"] + ".pgen", cfg, anc, tmp / "p_anc_int8" / "s.tsv", "int8")
    assert len(want[".tsv"].splitlines()) > 150
    assert score_files(pblock["clean"] + ".bed", cfg, anc, tmp / "p_anc_bed" / "s.tsv", "int8") == want
    assert score_files(pblock["pclean"] + ".pgen", cfg, anc, tmp / "p_anc_one" / "s.tsv", "packed2") == want
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "250000")
    assert score_files(pblock["pclean"], cfg, anc, tmp / "p_anc_three" / "s.tsv", "packed2") == want
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES")
    with pytest.raises(ValueError, match=r"block_p.pgen: missing call of sample [rtn]\d+ at variant v\d+ \(position \d+\) in a row flipped by the "
                       r"ancestral allele: its dosage is 4, which the 2-bit layout cannot hold; read this fileset with --layout int8"):
        score_files(pblock["pprefix"] + ".pgen", cfg, anc, tmp / "p_anc_unfit" / "s.tsv", "packed2")
