"""PLINK 2 ``.pgen`` records decoded straight into the packed2 layout, on the host: ``sai_pgen_pack2_host`` against a
numpy statement of the layout formula of saihip.h and of the table of saihip_pgen_packed.h, the host reader
(``pgen.load_packed``), what ``score(..., layout="packed2")`` refuses before it reads anything, and the chunk budget."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_checks
import native_build
import pgen_builder as B
from conftest import ROOT
from test_bed_pack2_cpu import pack_numpy, site_words, tile_words
from test_eigenstrat_cpu import eigenstrat_from_plink
from test_pgen_builder_cpu import EXAMPLE_CODES, EXAMPLE_TYPES, example_bytes
from test_pgen_cpu import ALL_TYPES, BAD_INDEX, BAD_RECORD, corrupted_records, random_matrix, random_types, tables_of
from test_plink_cpu import random_case, small_fileset

# the table of saihip_pgen_packed.h by code 0, 1, 2, 3: a field, "het" (refused) or "unfit" (dosage 4)
TABLE = {(2, 0): [0, 1, 2, 3], (2, 1): [2, 1, 0, "unfit"], (1, 0): [0, "het", 1, 3], (1, 1): [1, "het", 0, 2]}
N_IND = [1, 15, 16, 17, 63, 64, 65, 130]
N_SITES = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def expect(codes, flip, cols, ploidy):
    """(fields [rows][individuals], status, unfit) from TABLE, cell by cell.  ``codes`` = per row the codes of every
    sample, or None for a record that does not parse (a zero row with BAD_RECORD)."""
    n_ind = len(cols)
    fields = np.zeros((len(codes), n_ind), dtype=np.uint8)
    status, unfit = np.zeros(len(codes), dtype=np.int32), np.zeros(len(codes), dtype=np.int32)
    for r, row in enumerate(codes):
        if row is None:
            status[r] = BAD_RECORD
            continue
        for i in range(n_ind):
            col = int(cols[i])
            if not 0 <= col < len(row):
                status[r] = BAD_INDEX
                continue
            got = TABLE[(ploidy, int(flip[r] != 0))][int(row[col])]
            if got == "het":
                status[r] = max(status[r], n_ind - i)
            elif got == "unfit":
                unfit[r] = max(unfit[r], n_ind - i)
            else:
                fields[r, i] = got
    return fields, status, unfit


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack_host(data, rec, base, flip, sample_ct, cols, first_col, ploidy, packed, n_sites, out_row0, n_threads=3):
    """One ``sai_pgen_pack2_host`` call into ``packed``; returns (status, unfit)."""
    from sai_amd import _ffi, _ffi_pgen_packed

    lib = _ffi_pgen_packed.load_host()
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    rec, base = np.ascontiguousarray(rec, dtype=np.int64).reshape(-1, 3), np.ascontiguousarray(base, dtype=np.int64).reshape(-1, 3)
    flip, cols = np.ascontiguousarray(flip, dtype=np.uint8), np.ascontiguousarray(cols, dtype=np.int32)
    status, unfit = np.full(len(rec), -5, dtype=np.int32), np.full(len(rec), -5, dtype=np.int32)
    _ffi.check(lib.sai_pgen_pack2_host(ptr(buf), len(data), len(rec), ptr(rec), ptr(base), ptr(flip), sample_ct, len(cols),
                                       None if first_col >= 0 else ptr(cols), first_col, ploidy, ptr(packed), n_sites, out_row0,
                                       ptr(status), ptr(unfit), n_threads), lib)  # fmt: skip
    return status, unfit


def column_lists(n_ind, sample_ct, rng):
    """(first_col or -1, columns): a run from column 0, 1 and 3, and a permuted list with repeats."""
    out = [(f, np.arange(f, f + n_ind, dtype=np.int32)) for f in (0, 1, 3)]
    out.append((-1, rng.integers(0, sample_ct, size=n_ind).astype(np.int32)))
    return out


def check_whole_and_cut(data, rec, base, flip, sample_ct, cols, first_col, ploidy, codes, where):
    """The block written in one call equals the numpy statement; written in two calls cut inside a tile it is the same
    block, and a call writes the words of its own sites and no other."""
    n_sites, n_ind = len(rec), len(cols)
    fields, want_st, want_uf = expect(codes, flip, cols, ploidy)
    want = pack_numpy(fields)
    whole = np.full(want.size, 0xA5, dtype=np.uint8)
    st, uf = pack_host(data, rec, base, flip, sample_ct, cols, first_col, ploidy, whole, n_sites, 0)
    assert np.array_equal(st, want_st) and np.array_equal(uf, want_uf) and np.array_equal(whole, want), where
    cut = min(37, n_sites // 2)  # inside the first tile
    if cut:
        parts = np.full(want.size, 0xA5, dtype=np.uint8)
        for lo, hi in ((cut, n_sites), (0, cut)):  # the later sites first: the order of the calls does not matter
            before = parts.copy()
            st, uf = pack_host(data, rec[lo:hi], base[lo:hi], flip[lo:hi], sample_ct, cols, first_col, ploidy, parts, n_sites, lo)
            assert np.array_equal(st, want_st[lo:hi]) and np.array_equal(uf, want_uf[lo:hi]), (where, lo)
            mine = np.zeros(want.size // 4, dtype=bool)
            mine[site_words(n_sites, n_ind, lo, hi)] = True
            assert np.array_equal(parts.view(np.uint32)[~mine], before.view(np.uint32)[~mine]), (where, lo)  # nothing else is written
        assert np.array_equal(parts, whole), where
    return want_st, want_uf


def test_worked_example():
    """tests/golden/pgen_worked_example.hex: 5 samples, records of type 0, 4, 2, 1, 3."""
    data, table = B.build_pgen(EXAMPLE_CODES, EXAMPLE_TYPES)
    assert data == example_bytes() and [t[2] for t in table] == [0, 4, 2, 1, 3]
    rec, base = tables_of(table)
    codes = [np.array(row, dtype=np.uint8) for row in EXAMPLE_CODES]
    for first_col, cols in ((0, np.arange(5, dtype=np.int32)), (1, np.arange(1, 4, dtype=np.int32)), (-1, np.array([4, 0, 0, 2], np.int32))):
        for ploidy in (1, 2):
            for flip in ([0] * 5, [1] * 5, [0, 1, 1, 0, 1]):
                check_whole_and_cut(data, rec, base, np.array(flip, np.uint8), 5, cols, first_col, ploidy, codes, (first_col, ploidy, flip))
    # spelled out: ploidy 2, kept -- the field is the code; padding individuals 0, padding sites all ones
    packed = np.zeros(tile_words(5) * 4, dtype=np.uint8)
    st, uf = pack_host(data, rec, base, np.zeros(5, np.uint8), 5, np.arange(5), 0, 2, packed, 5, 0)
    words = packed.view(np.uint32)
    assert [[(int(words[s]) >> (2 * i)) & 3 for i in range(5)] for s in range(5)] == EXAMPLE_CODES
    assert all(int(words[s]) >> 10 == 0 for s in range(5)) and (words[5:] == 0xFFFFFFFF).all() and not st.any() and not uf.any()


@pytest.mark.parametrize("n_ind", N_IND)
def test_host_decoder_equals_the_numpy_statement(n_ind):
    rng = np.random.default_rng(700 + n_ind)
    sample_ct = n_ind + 9  # more samples than the run
    seen_het = seen_unfit = 0
    kinds = set()
    for n_sites in N_SITES:
        matrix = random_matrix(rng, n_sites, sample_ct)
        data, table = B.build_pgen(matrix, random_types(rng, n_sites), wide_types=bool(n_sites & 1), len_bytes=2)
        kinds |= {t[2] & 7 for t in table}
        rec, base = tables_of(table)
        flip = rng.integers(0, 2, size=n_sites).astype(np.uint8)  # flipped and unflipped rows mixed
        for first_col, cols in column_lists(n_ind, sample_ct, rng):
            for ploidy in (1, 2):
                st, uf = check_whole_and_cut(data, rec, base, flip, sample_ct, cols, first_col, ploidy, list(matrix), (n_ind, n_sites, first_col, ploidy))
                seen_het += int(st.any())
                seen_unfit += int(uf.any())
                assert not (st.any() and ploidy == 2) and not (uf.any() and ploidy == 1)
    assert kinds == set(ALL_TYPES) and seen_het and seen_unfit


def test_the_table_row_by_row_and_the_lowest_individual():
    data = bytes([0b11100100])  # samples 0..3 hold the codes 0, 1, 2, 3
    cols = np.arange(4, dtype=np.int32)
    for (ploidy, flipped), line in TABLE.items():
        for first_col in (0, -1):
            packed = np.full(tile_words(4) * 4, 0x5A, dtype=np.uint8)
            st, uf = pack_host(data, [[0, 1, 0]], [[-1] * 3], [flipped], 4, cols, first_col, ploidy, packed, 1, 0)
            words = packed.view(np.uint32)
            assert [(int(words[0]) >> (2 * i)) & 3 for i in range(4)] == [v if isinstance(v, int) else 0 for v in line]
            assert int(words[0]) >> 8 == 0  # padding individuals hold 0
            assert (words[1:] == 0xFFFFFFFF).all()  # padding sites: all ones
            assert st.tolist() == [4 - line.index("het") if "het" in line else 0]
            assert uf.tolist() == [4 - line.index("unfit") if "unfit" in line else 0]
    # the LOWEST individual is named: het at individuals 1 and 3 of 5 (ploidy 1); missing at 2 and 4 (flipped, ploidy 2)
    matrix = np.array([[2, 1, 0, 1, 2], [0, 2, 3, 0, 3]], dtype=np.uint8)
    data, table = B.build_pgen(matrix, [0, 7])
    rec, base = tables_of(table)
    packed = np.zeros(tile_words(5) * 4, dtype=np.uint8)
    st, uf = pack_host(data, rec, base, np.zeros(2, np.uint8), 5, np.arange(5), 0, 1, packed, 2, 0)
    assert st.tolist() == [5 - 1, 0] and uf.tolist() == [0, 0]
    st, uf = pack_host(data, rec, base, np.ones(2, np.uint8), 5, np.arange(5), 0, 2, packed, 2, 0)
    assert st.tolist() == [0, 0] and uf.tolist() == [0, 5 - 2]
    assert [(int(packed.view(np.uint32)[1]) >> (2 * i)) & 3 for i in range(5)] == [2, 0, 0, 2, 0]  # the unfit fields are 0
    # a column outside the samples: flagged, written as 0, never read
    st, uf = pack_host(data, rec, base, np.zeros(2, np.uint8), 5, np.array([0, 5, 4, -2], np.int32), -1, 2, packed, 2, 0)
    assert st.tolist() == [BAD_INDEX] * 2 and uf.tolist() == [0, 0]
    assert [(int(packed.view(np.uint32)[0]) >> (2 * i)) & 3 for i in range(4)] == [2, 0, 2, 0]


def test_corrupted_records_are_zero_rows_between_intact_neighbours():
    """The damaged records of test_pgen_cpu -- a difflist truncated inside every part, type 5, an index that does not
    increase among them: each a zero row with BAD_RECORD, every sound record between them as the table says."""
    n = 300
    data, rec, base, codes, what = corrupted_records(n)
    named = " / ".join(what)
    assert "truncated inside deltas 1" in named and "type 5" in named and "a delta of zero: an index twice" in named
    assert "a group starts on the last index of the group before" in named
    assert sum(c is None for c in codes) >= 45 and sum(c is not None for c in codes) >= 8
    rng = np.random.default_rng(3)
    flip = rng.integers(0, 2, len(rec)).astype(np.uint8)
    for first_col, cols in ((0, np.arange(n, dtype=np.int32)), (40, np.arange(40, 73, dtype=np.int32)), (-1, rng.permutation(n)[:17].astype(np.int32))):
        for ploidy in (1, 2):
            st, uf = check_whole_and_cut(data, rec, base, flip, n, cols, first_col, ploidy, codes, (first_col, ploidy))
            assert all((st[r] == BAD_RECORD) == (codes[r] is None) for r in range(len(rec))) and not uf[[c is None for c in codes]].any()


def test_argument_errors():
    from sai_amd import _ffi, _ffi_pgen_packed

    lib = _ffi_pgen_packed.load_host()
    data, rec, base, flip = np.zeros(4, np.uint8), np.array([[0, 2, 0]], np.int64), np.full((1, 3), -1, np.int64), np.zeros(1, np.uint8)
    cols, packed, st, uf = np.zeros(3, np.int32), np.zeros(tile_words(3) * 4, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32)

    def call(**kw):
        a = dict(data=ptr(data), n_bytes=4, n_out=1, rec=ptr(rec), base=ptr(base), flip=ptr(flip), sample_ct=8, n_ind=3, cols=ptr(cols),
                 first_col=-1, ploidy=2, packed=ptr(packed), n_sites=1, out_row0=0, st=ptr(st), uf=ptr(uf), n_threads=1)  # fmt: skip
        a.update(kw)
        rc = lib.sai_pgen_pack2_host(*a.values())
        return rc, lib.sai_last_error().decode()

    assert call()[0] == 0
    for kw, message in [(dict(cols=None), "NULL buffer"), (dict(uf=None), "NULL buffer"), (dict(base=None), "NULL buffer"),
                        (dict(first_col=6), "first_col + n_slots exceeds sample_ct"), (dict(ploidy=3), "ploidy must be 1 or 2"),
                        (dict(out_row0=1), "size out of range"), (dict(n_ind=0), "size out of range"), (dict(sample_ct=0), "size out of range")]:  # fmt: skip
        rc, text = call(**kw)
        assert rc == _ffi.SAI_ERR_ARG and message in text, (kw, text)


def test_header_binding_and_library_agree_and_the_other_headers_are_untouched():
    from sai_amd import _build, _ffi, _ffi_packed_ingest, _ffi_pgen, _ffi_pgen_packed

    names = abi_checks.declared_names("saihip_pgen_packed.h")
    assert names == sorted(_ffi_pgen_packed.SIGNATURES) == ["sai_pgen_pack2", "sai_pgen_pack2_host", "sai_pgen_packed_abi_version"]
    lib = _ffi_pgen_packed.load()
    version = abi_checks.header_macro("saihip_pgen_packed.h", "SAI_PGEN_PACKED_ABI_VERSION")
    assert lib.sai_pgen_packed_abi_version() == _ffi_pgen_packed.SAI_PGEN_PACKED_ABI_VERSION == version == 1
    assert lib.sai_pgen_pack2(None, None, 0, 0, None, None, None, 1, 1, None, -1, 2, None, 0, 0, None, None, None) == _ffi.SAI_ERR_ARG
    assert b"ctx is NULL" in lib.sai_last_error()
    # the headers beside it, their bindings and the version numbers are as they were
    assert len(abi_checks.declared_names("saihip_pgen.h")) == len(_ffi_pgen.SIGNATURES) == 8
    assert len(abi_checks.declared_names("saihip_packed_ingest.h")) == len(_ffi_packed_ingest.SIGNATURES) == 3
    assert lib.sai_abi_version() == _ffi.SAI_ABI_VERSION == 16 and lib.sai_pgen_abi_version() == 1 and lib.sai_packed_ingest_abi_version() == 1
    assert "pgen/pgen_pack2.hip" in _build.UNITS and "pgen/pgen_pack2_host.cpp" in _build.HOST_UNITS
    assert ROOT / "include" / "saihip_pgen_packed.h" in _build.PUBLIC_HEADERS


def anc_file(path, chrom, positions, alleles):
    path.write_text("".join(f"{chrom}\t{p - 1}\t{p}\t{a}\n" for p, a in zip(positions, alleles)))
    return str(path)


def packed_of(dos):
    return pack_numpy(np.where(dos < 0, 3, dos).astype(np.uint8)) if dos.size else np.zeros(0, np.uint8)


def test_host_reader_blocks_and_errors(tmp_path):
    """``pgen.load_packed`` against ``pack_numpy`` of ``pgen.load_dosage``, and its data errors: the unfit sentence in
    full; a heterozygous call at ploidy 1 (the int8 route's words) wins over a call that does not fit in the same row."""
    from sai_amd.utils import pgen

    bed_prefix, _ = small_fileset(tmp_path)
    prefix = str(tmp_path / "smallp")
    B.from_bed_fileset(bed_prefix, prefix, [0, 4, 2])
    pops = [(["e", "a"], 2), (["d", "a", "c"], 2)]
    pos, blocks, n_matched, n_anc = pgen.load_packed(prefix, "3", pops)
    assert pos.tolist() == [100, 200, 300] and (n_matched, n_anc) == (3, 0)
    for (names, ploidy), block in zip(pops, blocks):
        assert np.array_equal(block, packed_of(pgen.load_dosage(prefix, "3", names, [ploidy] * len(names))[1]))
    # rows 100 and 200 flipped, 300 kept
    anc = anc_file(tmp_path / "anc.bed", "3", [100, 200, 300], ["A", "C", "A"])
    assert pgen.load_dosage(prefix, "3", ["d", "e"], [2, 2], anc_allele_file=anc)[1].tolist() == [[4, 0], [0, 4], [0, 0]]
    with pytest.raises(ValueError, match=r"smallp.pgen: missing call of sample d at variant v1 \(position 100\) in a row flipped by the "
                       r"ancestral allele: its dosage is 4, which the 2-bit layout cannot hold; read this fileset with --layout int8$"):
        pgen.load_packed(prefix, "3", [(["a", "b"], 2), (["c", "d", "e"], 2)], anc_allele_file=anc)
    with pytest.raises(ValueError, match="missing call of sample e at variant v2"):
        pgen.load_packed(prefix + ".pgen", "3", [(["e"], 2)], anc_allele_file=anc, start=150)  # a type 2 row: its base lies before the region
    pos, blocks, _, _ = pgen.load_packed(prefix, "3", [(["d", "e"], 1)], anc_allele_file=anc, end=250)  # ploidy 1: missing flipped is 2
    assert np.array_equal(blocks[0], pack_numpy(np.array([[2, 0], [0, 2]], dtype=np.uint8)))
    # row 100 holds a missing call of d (flipped, ploidy 2: unfit) and a heterozygous call of b (ploidy 1): the het is reported
    with pytest.raises(ValueError, match="heterozygous call of sample b at variant v1 .position 100., but the sample is configured with ploidy 1"):
        pgen.load_packed(prefix, "3", [(["d", "a"], 2), (["a", "b"], 1)], anc_allele_file=anc)
    with pytest.raises(ValueError, match="SAI_AMD_INGEST_BUFFER of 1 bytes is smaller than one record"):
        pgen.load_packed(prefix, "3", pops, buffer_bytes=1)


def populations_of(request):
    """The request of a random case as populations: the diploid samples in two of them, the haploid ones in a third."""
    two = [s for s, p in request if p == 2]
    one = [s for s, p in request if p == 1]
    return [(names, ploidy) for names, ploidy in ((two[: len(two) // 2 + 1], 2), (two[len(two) // 2 + 1 :], 2), (one, 1)) if names]


def seeded_pgen(seed, tmp_path):
    """The random case ``seed`` of test_plink_cpu as a PLINK 2 fileset with forced record types of every kind."""
    case = random_case(seed, tmp_path)
    rng = np.random.default_rng(seed)
    prefix = str(tmp_path / f"p{seed}")
    types = random_types(rng, len(case["chroms"]), kinds=(None, 0, 1, 2, 2, 3, 3, 4, 6, 7))
    table = B.from_bed_fileset(case["prefix"], prefix, types, wide_types=bool(seed & 1), len_bytes=1 + seed % 3)
    return case, prefix, table


READER_SEEDS = (3, 4, 11)


def reader_cases(seed, tmp_path):
    """Per seed: (case, prefix, longest record, [(populations, anc, start, end, dosages per population)]).  With the
    ancestral-allele file the haploid samples are asked for on their own as well: flipped rows in which every dosage
    fits, whatever the diploid samples hold."""
    from sai_amd.utils import pgen

    case, prefix, table = seeded_pgen(seed, tmp_path)
    pops = populations_of(case["request"])
    here = case["positions"]
    asks = []
    for anc in (None, case["anc"]):
        for start, end in [(None, None), (here[2], here[-2])]:
            for ask in [pops] + ([[pop for pop in pops if pop[1] == 1]] if anc else []):
                if ask:
                    dosages = [pgen.load_dosage(prefix, "7", names, [ploidy] * len(names), start, end, anc) for names, ploidy in ask]
                    asks.append((ask, anc, start, end, dosages))
    return case, prefix, max(t[1] for t in table), asks


def test_host_reader_equals_the_pack_of_the_int8_reader(tmp_path):
    """With and without a region and an ancestral-allele file, in batches of a few records and in one.  These are the
    seeds of the device test: that enough of them can be compared, some of them flipped, and that one is refused, is
    settled here."""
    from sai_amd.utils import pgen

    compared = flipped = refused = 0
    for seed in READER_SEEDS:
        case, prefix, longest, asks = reader_cases(seed, tmp_path)
        for pops, anc, start, end, dosages in asks:
            fits = all(int(d[1].max(initial=0)) <= 2 for d in dosages)
            for cap in (2 * longest, None):
                if not fits:
                    with pytest.raises(ValueError, match=r"missing call of sample s\d+ at variant rs\d+_\d+ \(position \d+\) in a row flipped"):
                        pgen.load_packed(prefix, "7", pops, start, end, anc, buffer_bytes=cap)
                    refused += 1
                    continue
                pos, blocks, n_matched, n_anc = pgen.load_packed(prefix, "7", pops, start, end, anc, buffer_bytes=cap)
                assert pos.dtype == np.int32 and pos.tolist() == dosages[0][0].tolist() and (n_matched, n_anc) == dosages[0][2:]
                for block, (_, d, _, _) in zip(blocks, dosages):
                    assert np.array_equal(block, packed_of(d)), (seed, anc, start, cap)
                    compared += 1
                    flipped += int(anc is not None and d.size > 0)
    assert compared >= 18 and flipped and refused


def test_what_packed2_accepts_and_refuses_before_reading(tmp_path, in_repo_root, monkeypatch):
    from sai_amd import sai as sai_mod

    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SAI_AMD_INGEST", "SAI_AMD_LAYOUT"):
        monkeypatch.delenv(name, raising=False)
    bed_prefix, _ = small_fileset(tmp_path)
    prefix = str(tmp_path / "smallp")
    B.from_bed_fileset(bed_prefix, prefix, [0, 4, 2])
    geno = eigenstrat_from_plink(bed_prefix, str(tmp_path / "smallg"), "packed")
    with open(prefix + ".pgen", "r+b") as f:
        f.truncate(12)  # nothing may be read: this .pgen holds its header and no record at all
    uq = "tests/data/example.u_and_q.config.yaml"
    dd = str(tmp_path / "with_dd.yaml")
    with open(dd, "w") as f:
        f.write(open(uq).read().replace("\nploidies:", "  DD: true\nploidies:", 1))
    assert sai_mod.require_packed2_input(prefix, uq, 1) is None and sai_mod.require_packed2_input(prefix + ".pgen", uq, 1) is None
    ask = dict(chr_name="3", win_len=100, win_step=50, anc_allele_file=None, output_file=str(tmp_path / "o" / "s.tsv"))
    with pytest.raises(ValueError, match=r"^layout 'packed2' serves the U and Q statistics only, but DD is configured\.$"):
        sai_mod.score(vcf_file=prefix + ".pgen", config=dd, num_workers=1, layout="packed2", **ask)
    with pytest.raises(ValueError, match=r"^layout 'packed2' runs in one process on one GPU: use num_workers=1 outside a rank job"):
        sai_mod.score(vcf_file=prefix, config=uq, num_workers=2, layout="packed2", **ask)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match=r"^layout 'packed2' runs in one process on one GPU"):
        sai_mod.score(vcf_file=prefix, config=uq, num_workers=1, layout="packed2", **ask)
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.delenv("RANK")
    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    monkeypatch.setenv("SAI_AMD_LAYOUT", "packed2")  # the environment's default counts like the argument
    with pytest.raises(ValueError, match=r"^layout 'packed2' is decoded on the GPU: it cannot be combined with SAI_AMD_INGEST=host\.$"):
        sai_mod.score(vcf_file=prefix, config=uq, num_workers=1, **ask)
    monkeypatch.delenv("SAI_AMD_INGEST")
    monkeypatch.delenv("SAI_AMD_LAYOUT")
    for path in (geno, geno + ".geno"):  # an EIGENSOFT fileset keeps the sentence as it was
        with pytest.raises(ValueError, match=rf"^layout 'packed2' reads a PLINK 1 fileset \(.bed \+ .bim \+ .fam\) only, which {re.escape(path)} is not\.$"):
            sai_mod.score(vcf_file=path, config=uq, num_workers=1, layout="packed2", **ask)
    assert not (tmp_path / "o").exists()  # refused before the output files are opened


def test_memory_estimate_counts_two_bits_per_call(tmp_path, monkeypatch):
    """variant_ct x ceil(sample_ct / 4) of the header, not the size of the compressed file."""
    from sai_amd import sai as sai_mod

    rng = np.random.default_rng(5)
    matrix = np.zeros((40, 13), dtype=np.uint8)
    matrix[rng.random(matrix.shape) < 0.03] = 1  # sparse rows: difflist records of a few bytes each
    prefix = str(tmp_path / "sparse")
    samples = [f"s{i}" for i in range(13)]
    B.write_fileset(prefix, ["1"] * 40, list(range(1, 41)), [f"v{k}" for k in range(40)], ["A"] * 40, ["C"] * 40, matrix, samples)
    resident = 40 * 4  # ceil(13 / 4) = 4 bytes per variant
    assert os.path.getsize(prefix + ".pgen") < resident  # the file's own size would under-count
    for budget, chunks in ((resident, 1), (resident - 1, 2), (resident // 2, 2), (resident // 2 - 1, 3), (resident // 3, 4)):
        monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", str(budget))
        assert sai_mod.chunks_for_memory(prefix, "packed2") == sai_mod.chunks_for_memory(prefix + ".pgen", layout="packed2") == chunks, budget
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", str(resident))
    assert sai_mod.chunks_for_memory(prefix, "int8") == -(-40 * 13 // resident) == 4  # the int8 route: a byte per call


def test_command_line_names_the_pfile_in_the_layout_help():
    from test_plink_cpu import sai_cli

    res = sai_cli("score", "--help")
    text = " ".join(res.stdout.split())
    assert res.returncode == 0 and "--layout {int8,packed2}" in res.stdout and "a PLINK 2 fileset given with --pfile" in text


@pytest.fixture(scope="module")
def pack2_program(tmp_path_factory):
    """tests/native/pgen_pack2_dump.cpp + the host units of libsaihip under ASan + UBSan, the runtimes linked in."""
    import __graft_entry__ as entry

    assert "pgen/pgen_pack2_host.cpp" in entry.HOST_UNITS
    return native_build.dump_program("pgen_pack2_dump", tmp_path_factory)["san"]


def test_host_decoder_is_clean_under_asan_ubsan(tmp_path, pack2_program):
    """The host decoder run (not only compiled) under the sanitizers as a program of its own: the worked example and
    the batch of damaged records, read from a heap block of exactly the batch's size -- the same block, status and
    unfit as the numpy statement and as the library."""
    example, table = B.build_pgen(EXAMPLE_CODES, EXAMPLE_TYPES)
    ex_rec, ex_base = tables_of(table)
    n = 300
    damaged, rec, base, codes, _ = corrupted_records(n)
    rng = np.random.default_rng(9)
    runs = [(example, ex_rec, ex_base, [np.array(r, np.uint8) for r in EXAMPLE_CODES], 5, np.arange(5), 0, 2, 0),
            (example, ex_rec, ex_base, [np.array(r, np.uint8) for r in EXAMPLE_CODES], 5, np.array([4, 1, 1, 0, 7, -1]), -1, 1, 3),
            (damaged, rec, base, codes, n, np.arange(3, 3 + 130), 3, 2, 37),
            (damaged, rec, base, codes, n, rng.integers(0, n, size=65), -1, 1, 0)]  # fmt: skip
    for data, rec_, base_, codes_, sample_ct, cols, first_col, ploidy, cut in runs:
        flip = (np.arange(len(rec_)) % 2).astype(np.uint8)
        (tmp_path / "bytes.bin").write_bytes(bytes(data))
        (tmp_path / "records.txt").write_text("".join(" ".join(str(int(v)) for v in [*rec_[r], *base_[r], flip[r]]) + "\n" for r in range(len(rec_))))
        res = native_build.run_native(pack2_program, [tmp_path / "bytes.bin", tmp_path / "records.txt", sample_ct, ploidy, first_col, cut, 3,
                                                      ",".join(map(str, cols))])  # fmt: skip
        assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
        lines = res.stdout.splitlines()
        fields, want_st, want_uf = expect(codes_, flip, cols, ploidy)
        assert [int(v) for v in lines[0].split()] == want_st.tolist() and [int(v) for v in lines[1].split()] == want_uf.tolist()
        assert bytes.fromhex(lines[2]) == pack_numpy(fields).tobytes()
        packed = np.zeros(pack_numpy(fields).size, dtype=np.uint8)
        st, uf = pack_host(data, rec_, base_, flip, sample_ct, cols, first_col, ploidy, packed, len(rec_), 0)
        assert st.tolist() == want_st.tolist() and uf.tolist() == want_uf.tolist() and packed.tobytes() == bytes.fromhex(lines[2])
        assert (want_st == BAD_RECORD).any() == (data is damaged)
    res = native_build.run_native(pack2_program, [tmp_path / "bytes.bin", tmp_path / "records.txt", 300, 2, 299, 0, 1, "0,1"])
    assert res.returncode == 3 and "first_col + n_slots exceeds sample_ct" in res.stderr and "Sanitizer" not in res.stderr
