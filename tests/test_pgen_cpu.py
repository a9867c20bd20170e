"""PLINK 2 filesets on the host: the index of PREFIX.psam / PREFIX.pvar / the .pgen header, the host decoder of
.pgen records and the dispatch of the readers.  The filesets are written by tests/pgen_builder.py (pure Python,
written from the rules alone); the expectation comes from the code matrix through the dosage table restated here,
from the PLINK 1 route on the same genotypes, or from the worked example committed as hex."""

import os
import shutil

import numpy as np
import pytest

import abi_checks
import native_build
import pgen_builder as B
from conftest import ROOT
from test_pgen_builder_cpu import EXAMPLE_CODES, EXAMPLE_TYPES, example_bytes
from test_plink_cpu import random_case, run_dump, sai_cli, small_fileset

BAD_INDEX, BAD_RECORD = 0x7FFFFFFF, 0x7FFFFFFE
# the dosage table of DESIGN_INGEST.md: [ploidy][flipped][code]; a het at ploidy 1 is flagged, its byte is 0
TABLE = {2: {0: [0, 1, 2, -2], 1: [2, 1, 0, 4]}, 1: {0: [0, 0, 1, -1], 1: [1, 0, 0, 2]}}
ALL_TYPES = (0, 1, 2, 3, 4, 6, 7)


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def expected(codes, cols, ploidies, flips):
    """(out int8 [rows][slots], status int32 [rows]) of a code matrix by the table."""
    codes = np.asarray(codes, dtype=np.uint8)
    cols, ploidies, flips = np.asarray(list(cols), dtype=np.int64), np.asarray(list(ploidies), dtype=np.int64), np.asarray(flips, dtype=np.int64)
    valid = (cols >= 0) & (cols < codes.shape[1]) & ((ploidies == 1) | (ploidies == 2))
    picked = codes[:, np.where(valid, cols, 0)].astype(np.int64)  # [rows][slots]
    table = np.array([[TABLE[pl][f] for f in (0, 1)] for pl in (1, 2)], dtype=np.int8)
    out = np.where(valid[None, :], table[np.where(valid, ploidies, 1)[None, :] - 1, flips[:, None], picked], 0).astype(np.int8)
    het = valid[None, :] & (ploidies == 1)[None, :] & (picked == 1)
    status = np.where(het.any(axis=1), len(cols) - het.argmax(axis=1), 0).astype(np.int32)
    if not valid.all():
        status[:] = BAD_INDEX
    return out.reshape(codes.shape[0], len(cols)), status


def decode_host(data: bytes, rec, base, flips, sample_ct, cols, ploidies, n_threads=2):
    """``sai_pgen_decode_host`` on raw bytes and a record table."""
    import ctypes as C

    from sai_amd import _ffi, _ffi_pgen

    lib = _ffi_pgen.load_host()
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    rec, base = np.ascontiguousarray(rec, dtype=np.int64).reshape(-1, 3), np.ascontiguousarray(base, dtype=np.int64).reshape(-1, 3)
    flips = np.ascontiguousarray(flips, dtype=np.uint8)
    cols, ploidies = np.ascontiguousarray(cols, dtype=np.int32), np.ascontiguousarray(ploidies, dtype=np.int32)
    out = np.full((len(rec), len(cols)), 99, dtype=np.int8)
    status = np.full(len(rec), -7, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _ffi.check(lib.sai_pgen_decode_host(p(buf), len(data), len(rec), p(rec), p(base), p(flips), sample_ct, len(cols), p(cols), p(ploidies),
                                        p(out), p(status), n_threads))  # fmt: skip
    return out, status


def tables_of(table):
    """(rec, base) of ``build_pgen``'s table, every variant selected, offsets counted from the start of the file."""
    rec = np.array([[off, length, vr] for off, length, vr, _ in table], dtype=np.int64)
    base = np.array([list(table[b][:3]) if b >= 0 else [-1, -1, -1] for _, _, _, b in table], dtype=np.int64)
    return rec, base


def random_types(rng, n_var, kinds=(None, *ALL_TYPES)):
    types = [kinds[int(rng.integers(len(kinds)))] for _ in range(n_var)]
    if types and types[0] in (2, 3):
        types[0] = 0
    return types


def random_matrix(rng, n_var, n, similar=True):
    """Rows that resemble their predecessor (so that difference records are short) with a few dense ones in between."""
    m = np.zeros((n_var, n), dtype=np.uint8)
    row = rng.integers(0, 4, n).astype(np.uint8)
    for v in range(n_var):
        style = rng.integers(4) if similar else 0
        if style == 0:
            row = rng.integers(0, 4, n).astype(np.uint8)
        elif style == 1:
            row = np.full(n, [0, 2, 3][int(rng.integers(3))], dtype=np.uint8)
        hit = rng.random(n) < rng.choice([0.0, 0.01, 0.1, 0.5])
        row = row.copy()
        row[hit] = rng.integers(0, 4, int(hit.sum()))
        m[v] = row
    return m


def simple_fileset(prefix, matrix, types=None, chrom="1", **options):
    n_var, n = np.asarray(matrix).shape
    samples = [f"s{i}" for i in range(n)]
    positions = [100 * (k + 1) for k in range(n_var)]
    table = B.write_fileset(prefix, [chrom] * n_var, positions, [f"v{k}" for k in range(n_var)], ["A"] * n_var, ["C"] * n_var, matrix, samples,
                            types, **options)  # fmt: skip
    return samples, positions, table


# ---- worked example and types ----


def test_worked_example(tmp_path):
    from sai_amd.utils import pgen

    prefix = str(tmp_path / "ex")
    samples, positions, _ = simple_fileset(prefix, EXAMPLE_CODES, EXAMPLE_TYPES)
    assert open(prefix + ".pgen", "rb").read() == example_bytes()  # the committed bytes are what is read below
    want, _ = expected(EXAMPLE_CODES, range(5), [2] * 5, [0] * 5)
    pos, dos, n_matched, n_anc = pgen.load_dosage(prefix, "1", samples, [2] * 5)
    assert pos.tolist() == positions and (n_matched, n_anc) == (5, 0) and dos.dtype == np.int8 and np.array_equal(dos, want)
    assert want.tolist() == [[0, 1, 2, -2, 1], [0, 0, 0, 2, 0], [0, 1, 0, 2, 0], [2, 2, -2, 2, 0], [0, 0, -2, 1, 2]]
    idx = pgen._Index(pgen._ffi_pgen.load_host(), prefix, "1", samples, [2] * 5, None, None, None, 2)
    assert idx.rec.tolist() == [[28, 2, 0], [30, 3, 4], [33, 3, 2], [36, 5, 1], [41, 3, 3]]
    assert idx.base.tolist() == [[-1] * 3, [-1] * 3, [30, 3, 4], [-1] * 3, [36, 5, 1]]
    assert (idx.sample_ct, idx.variant_ct, idx.mode) == (5, 5, 0x10) and pgen.scan_first_last(prefix, "1") == (100, 500)
    # a region that starts on a record of type 2 / 3: its base lies before the region and is fetched too
    for start, rows in ((300, [2, 3, 4]), (500, [4])):
        for cap in (None, 8):
            pos, dos, n_matched, _ = pgen.load_dosage(prefix, "1", samples, [2] * 5, start=start, buffer_bytes=cap)
            assert pos.tolist() == [positions[r] for r in rows] and n_matched == len(rows) and np.array_equal(dos, want[rows])


@pytest.mark.parametrize("seed", range(6))
def test_every_type_and_every_base_type(tmp_path, seed):
    """Random matrices with random forced types: bases 1 and several records back, of every type; regions that
    start anywhere (also on a type 2 / 3 record whose base lies before the region), batches of a few records."""
    from sai_amd.utils import pgen

    rng = np.random.default_rng(100 + seed)
    n = [1, 5, 37, 64, 130, 300][seed]
    n_var = 60
    matrix = random_matrix(rng, n_var, n)
    types = random_types(rng, n_var)
    for v in range(10, 50, 8):  # runs of difference records behind a base of every kind
        types[v : v + 6] = [ALL_TYPES[(v // 8 + seed) % 7] if ALL_TYPES[(v // 8 + seed) % 7] not in (2, 3) else 4, 2, 3, 2, 3, 3]
    prefix = str(tmp_path / "t")
    samples, positions, table = simple_fileset(prefix, matrix, types, wide_types=bool(seed % 2), len_bytes=1 + seed % 4)
    kinds = {(t[2] & 7, table[t[3]][2] & 7 if t[3] >= 0 else -1) for t in table}
    assert {k for k, _ in kinds} >= {0, 1, 2, 3} and {b for k, b in kinds if k in (2, 3)} - {-1}
    cols = rng.permutation(n)[: min(n, 9)].tolist() + [0]
    names, ploidies = [samples[c] for c in cols], [2] * len(cols)
    want, _ = expected(matrix, cols, ploidies, [0] * n_var)
    for start_row in (0, 11, 12, 13, 29, 59):
        for cap in (None, 3 * max(t[1] for t in table)):
            pos, dos, n_matched, _ = pgen.load_dosage(prefix, "1", names, ploidies, start=positions[start_row], buffer_bytes=cap)
            assert pos.tolist() == positions[start_row:] and n_matched == n_var - start_row
            assert np.array_equal(dos, want[start_row:]), (seed, start_row, cap)


def test_bases_of_every_type_at_several_distances(tmp_path):
    from sai_amd.utils import pgen

    rng = np.random.default_rng(5)
    n = 70
    seen = set()
    for base_type in (0, 1, 4, 6, 7):
        for distance in (1, 2, 5):
            matrix = random_matrix(rng, distance + 2, n)
            types = [0] + [base_type] + [2, 3][distance % 2 :][:1] * (distance - 1) + [2 + (base_type + distance) % 2]
            types = (types + [3] * distance)[: distance + 2]
            prefix = str(tmp_path / f"b{base_type}_{distance}")
            samples, positions, table = simple_fileset(prefix, matrix, types)
            assert table[-1][3] == 1 and table[-1][2] & 7 in (2, 3) and table[1][2] == base_type
            seen.add((table[-1][2], base_type, distance))
            want, _ = expected(matrix, range(n), [2] * n, [0] * len(matrix))
            pos, dos, _, _ = pgen.load_dosage(prefix, "1", samples, [2] * n, start=positions[-1])  # the base lies before the region
            assert pos.tolist() == positions[-1:] and np.array_equal(dos, want[-1:])
            assert np.array_equal(pgen.load_dosage(prefix, "1", samples, [2] * n)[1], want)
    assert {t for t, _, _ in seen} == {2, 3}


# ---- header forms ----


def test_header_forms(tmp_path):
    from sai_amd.utils import pgen

    rng = np.random.default_rng(9)
    n, n_var = 21, 40
    matrix = random_matrix(rng, n_var, n)
    types = random_types(rng, n_var)
    want, _ = expected(matrix, range(n), [2] * n, [0] * n_var)
    sizes = set()
    for wide in (False, True):
        for len_bytes in (1, 2, 3, 4):
            for allele_bytes, flags in ((0, False), (1, True), (2, False), (3, True)):
                prefix = str(tmp_path / f"h{int(wide)}{len_bytes}{allele_bytes}")
                junk = [bytes(rng.integers(0, 256, int(rng.integers(0, 4))).astype(np.uint8)) for _ in range(n_var)] if wide else None
                samples, positions, table = simple_fileset(prefix, matrix, types, wide_types=wide, len_bytes=len_bytes,
                                                           allele_bytes=allele_bytes, flags=flags, junk=junk)  # fmt: skip
                sizes.add(os.path.getsize(prefix + ".pgen"))
                if wide:
                    assert any(t[2] & 0x10 for t in table)  # trailing tracks that are never read
                pos, dos, _, _ = pgen.load_dosage(prefix, "1", samples, [2] * n)
                assert pos.tolist() == positions and np.array_equal(dos, want), (wide, len_bytes, allele_bytes, flags)
    assert len(sizes) >= 12
    # the fixed-width mode, and the three forms of the two text files
    for k, (pvar, psam) in enumerate([(dict(header=True), "#FID IID"), (dict(header=True, extra_columns=True, meta_lines=False), "#IID"),
                                      (dict(header=False, meta_lines=False), "fam"), (dict(header=False, meta_lines=True), "#IID")]):  # fmt: skip
        prefix = str(tmp_path / f"fixed{k}")
        samples, positions, table = simple_fileset(prefix, matrix, None, mode=0x02, pvar=pvar, psam=psam)
        assert os.path.getsize(prefix + ".pgen") == 12 + n_var * 6
        pos, dos, n_matched, _ = pgen.load_dosage(prefix, "1", samples[::-1], [2] * n, start=positions[3], end=positions[30])
        assert pos.tolist() == positions[3:31] and n_matched == 28 and np.array_equal(dos, want[3:31, ::-1])
        assert pgen.scan_first_last(prefix + ".pgen", "1") == (positions[0], positions[-1]) and pgen.scan_first_last(prefix, "2") == (None, None)


def test_two_blocks_of_65536_variants(tmp_path):
    from sai_amd.utils import pgen

    rng = np.random.default_rng(3)
    n_var, n = 65540, 5
    matrix = rng.integers(0, 4, (n_var, n)).astype(np.uint8)
    matrix[rng.random(n_var) < 0.7] = 0
    types = [None] * n_var
    types[65534:65540] = [4, 2, 0, 2, 3, 2]  # 65536 opens the second block: its base is itself a new record
    prefix = str(tmp_path / "two")
    samples, positions, table = simple_fileset(prefix, matrix, types)
    header = open(prefix + ".pgen", "rb").read(28)
    assert int.from_bytes(header[12:20], "little") == table[0][0] and int.from_bytes(header[20:28], "little") == table[65536][0]
    want, _ = expected(matrix[65500:], range(n), [2] * n, [0] * 40)
    pos, dos, n_matched, _ = pgen.load_dosage(prefix, "1", samples, [2] * n, start=positions[65500])
    assert pos.tolist() == positions[65500:] and n_matched == 40 and np.array_equal(dos, want)
    idx = pgen._Index(pgen._ffi_pgen.load_host(), prefix, "1", samples, [2] * n, positions[65535], None, None, 2)
    assert idx.rec[:, 0].tolist() == [t[0] for t in table[65535:]] and idx.base[:, 0].tolist() == [table[65534][0], -1, table[65536][0], table[65536][0], table[65536][0]]
    whole = pgen.load_dosage(prefix, "1", samples[:2], [2, 2])
    assert np.array_equal(whole[1], expected(matrix, [0, 1], [2, 2], [0] * n_var)[0])
    # a block whose first record is of type 2 / 3 has nothing to differ from
    types[65536] = 2
    simple_fileset(str(tmp_path / "bad"), matrix, types, allow_bad_first=True)
    with pytest.raises(ValueError, match=r"bad.pgen: variant 65537, the first of block 1, is of type 2: it has no record to differ from"):
        pgen.load_dosage(str(tmp_path / "bad"), "1", samples, [2] * n)


# ---- agreement with the PLINK 1 route ----


@pytest.mark.parametrize("seed", range(8))
def test_agreement_with_the_bed_route(tmp_path, seed):
    """Positions, rows, flips, counts and dosages equal those of the .bed route on the same genotypes, with and
    without an ancestral-allele file, whole and in regions, in one batch and in many."""
    from sai_amd.utils import pgen, plink

    case = random_case(seed, tmp_path)
    rng = np.random.default_rng(seed)
    n_var = len(case["chroms"])
    prefix = str(tmp_path / f"p{seed}")
    B.from_bed_fileset(case["prefix"], prefix, random_types(rng, n_var), wide_types=bool(seed & 1), len_bytes=1 + seed % 3,
                       pvar=dict(header=seed % 3 != 0, extra_columns=seed % 2 == 0), psam=["#FID IID", "#IID", "fam"][seed % 3])  # fmt: skip
    names, ploidies = [s for s, _ in case["request"]], [p for _, p in case["request"]]
    here = case["positions"]
    lib = pgen._ffi_pgen.load_host()
    for anc in (None, case["anc"]):
        for start, end in [(None, None), (here[len(here) // 3], here[-2] + 1), (here[0] + 1, None)]:
            want = plink.load_dosage(case["prefix"], "7", names, ploidies, start, end, anc)
            for cap in (None, 256):  # a few records per batch
                got = pgen.load_dosage(prefix, "7", names, ploidies, start, end, anc, buffer_bytes=cap)
                assert got[0].dtype == np.int32 and got[1].dtype == np.int8
                assert got[0].tolist() == want[0].tolist() and got[2:] == want[2:] and np.array_equal(got[1], want[1]), (seed, start, end, anc)
            a = pgen._Index(lib, prefix, "7", names, ploidies, start, end, anc, 2)
            b = plink._Index(plink._ffi_plink.load_host(), case["prefix"], "7", names, ploidies, start, end, anc, 2)
            assert a.file_row.tolist() == b.file_row.tolist() and a.flip.tolist() == b.flip.tolist() and a.col_of_slot.tolist() == b.col_of_slot.tolist()
            assert (a.first_col, a.uniform_ploidy, a.first, a.last) == (b.first_col, b.uniform_ploidy, b.first, b.last)
    assert pgen.scan_first_last(prefix, "7") == plink.scan_first_last(case["prefix"], "7")
    assert pgen.scan_first_last(prefix + ".pgen", "nope") == (None, None)


def test_fixture_fileset_reads_like_its_vcf(in_repo_root, tmp_path):
    from test_plink_cpu import fileset_from_vcf

    from sai_amd.generators import ChunkGenerator
    from sai_amd.sai import load_config
    from sai_amd.utils.native_vcf import scan_first_last
    from sai_amd.utils.read_data import read_dosage_data

    vcf, chrom, cfgfile, anc = "tests/data/test.data.vcf", "21", "tests/data/test.uq.config.yaml", "tests/data/test.anc.allele.bed"
    bed = str(tmp_path / "fx")
    fileset_from_vcf(vcf, bed)
    prefix = str(tmp_path / "pfx")
    B.from_bed_fileset(bed, prefix)
    cfg = load_config(cfgfile)
    groups = dict(ref_ind_file=cfg.populations.get_population("ref"), tgt_ind_file=cfg.populations.get_population("tgt"),
                  src_ind_file=cfg.populations.get_population("src"), out_ind_file=cfg.populations.get_population("outgroup"))  # fmt: skip
    compared = 0
    for anc_file in (None, anc):
        kw = dict(chr_name=chrom, ploidy_config=cfg.ploidies, anc_allele_file=anc_file, **groups)
        want = read_dosage_data(vcf_file=vcf, **kw)
        for source in (prefix + ".pgen", prefix):
            got = read_dosage_data(vcf_file=source, **kw)
            assert set(got) == set(want)
            for group in want:
                assert got[group][1] == want[group][1] and (got[group][0] is None) == (want[group][0] is None)
                for pop, block in (want[group][0] or {}).items():
                    mine = got[group][0][pop]
                    assert mine.POS.tolist() == block.POS.tolist() and mine.GT.dtype == np.int8 and np.array_equal(mine.GT, block.GT)
                    compared += 1
    assert compared >= 4
    assert scan_first_last(prefix + ".pgen", chrom) == scan_first_last(vcf, chrom)
    a = ChunkGenerator(vcf_file=prefix + ".pgen", chr_name=chrom, window_size=5000, step_size=2500, num_chunks=3)
    b = ChunkGenerator(vcf_file=vcf, chr_name=chrom, window_size=5000, step_size=2500, num_chunks=3)
    assert a.chunks == b.chunks and a.windows == b.windows


def test_the_table_row_by_row(tmp_path):
    """The dosage table, restated: ploidy 2 and 1, kept and flipped rows, repeated and permuted requests."""
    from sai_amd.utils import pgen

    prefix = str(tmp_path / "tab")
    codes = [[2, 1, 0, 3, 2], [0, 0, 1, 2, 3], [1, 2, 2, 0, 0]]
    B.write_fileset(prefix, ["3"] * 3, [100, 200, 300], ["v1", "v2", "v3"], ["T", "G", "A"], ["A", "C", "G"], codes, list("abcde"), [0, 4, 1])
    pos, dos, n_matched, n_anc = pgen.load_dosage(prefix, "3", ["e", "a", "d", "a"], [2, 2, 2, 2])
    assert pos.tolist() == [100, 200, 300] and (n_matched, n_anc) == (3, 0)
    assert dos.tolist() == [[2, 2, -2, 2], [-2, 0, 2, 0], [0, 1, 0, 1]]
    anc = tmp_path / "anc.bed"
    anc.write_text("3\t99\t100\tA\n3\t199\t200\tG\n3\t299\t300\tC\n9\t1\t2\tA\n")  # ALT: flip; REF: keep; neither: drop
    pos, dos, n_matched, n_anc = pgen.load_dosage(prefix, "3", list("abcde"), [2] * 5, anc_allele_file=str(anc))
    assert pos.tolist() == [100, 200] and (n_matched, n_anc) == (3, 3)
    assert dos.tolist() == [[0, 1, 2, 4, 0], [0, 0, 1, 2, -2]]
    pos, dos, _, _ = pgen.load_dosage(prefix, "3", ["d", "e", "a"], [1, 1, 1], start=100, end=100, anc_allele_file=str(anc))
    assert pos.tolist() == [100] and dos.tolist() == [[2, 0, 0]]  # flipped: missing 2, ALT ALT 0
    pos, dos, _, _ = pgen.load_dosage(prefix, "3", ["d", "e", "a"], [1, 1, 2], start=150, end=250)
    assert pos.tolist() == [200] and dos.tolist() == [[1, -1, 0]]


# ---- refusals ----


def example_fileset(tmp_path, name, **kw):
    prefix = str(tmp_path / name)
    args = dict(chroms=["3"] * 5, positions=[100, 200, 300, 400, 500], ids=[f"v{k}" for k in range(1, 6)], ref=["A"] * 5, alt=["C"] * 5,
                matrix=EXAMPLE_CODES, samples=list("abcde"), types=EXAMPLE_TYPES)  # fmt: skip
    args.update(kw)
    B.write_fileset(prefix, **args)
    return prefix


def patched(prefix, at, value: bytes):
    with open(prefix + ".pgen", "r+b") as f:
        f.seek(at)
        f.write(value)
    return prefix


def test_refusals(tmp_path, in_repo_root):
    from sai_amd.sai import load_config
    from sai_amd.utils import filesets, pgen
    from sai_amd.utils.read_data import read_data, read_dosage_data

    ask = dict(chr_name="3", samples=["a", "b"], ploidies=[2, 2])
    good = example_fileset(tmp_path, "good")
    assert pgen.load_dosage(good, **ask)[1].tolist() == [[0, 1], [0, 0], [0, 1], [2, 2], [0, 0]]
    # storage modes
    bad = patched(example_fileset(tmp_path, "bedmode"), 2, b"\x01")
    assert not pgen.is_fileset(bad) and not filesets.is_fileset(bad)
    with pytest.raises(ValueError, match=r"bedmode.pgen: storage mode 0x01: this is a PLINK 1 .bed file, give its fileset with --bfile"):
        pgen.load_dosage(bad + ".pgen", **ask)
    for mode in (0x03, 0x04, 0x11, 0x20, 0x21, 0x00, 0x12):
        bad = patched(example_fileset(tmp_path, f"mode{mode:02x}"), 2, bytes([mode]))
        with pytest.raises(ValueError, match=rf"mode{mode:02x}.pgen: storage mode 0x{mode:02X} is not supported"):
            pgen.load_dosage(bad, **ask)
    bad = patched(example_fileset(tmp_path, "magic"), 1, b"\x1c")
    assert not pgen.is_fileset(bad)
    with pytest.raises(ValueError, match="magic.pgen: not a PLINK 2 .pgen file"):
        pgen.load_dosage(bad, **ask)
    # the control nibble
    for control in (0x08, 0x0F):
        bad = patched(example_fileset(tmp_path, f"control{control}"), 11, bytes([control]))
        with pytest.raises(ValueError, match=rf"control byte {control:02X} has a vrtype and record-length code of {control}"):
            pgen.load_dosage(bad, **ask)
    # counts against the two text files
    bad = patched(example_fileset(tmp_path, "nvar"), 3, (6).to_bytes(4, "little"))
    with pytest.raises(ValueError, match="nvar.pgen: the header counts 6 variants, the .pvar has 5"):
        pgen.load_dosage(bad, **ask)
    bad = patched(example_fileset(tmp_path, "nsam"), 7, (4).to_bytes(4, "little"))
    with pytest.raises(ValueError, match="nsam.pgen: the header counts 4 samples, the .psam has 5"):
        pgen.load_dosage(bad, **ask)
    # block offsets and record lengths that leave the file or overlap
    bad = patched(example_fileset(tmp_path, "offset"), 12, (45).to_bytes(8, "little"))
    with pytest.raises(ValueError, match="offset.pgen: block 0 starts at byte 45, which is outside the file"):
        pgen.load_dosage(bad, **ask)
    bad = patched(example_fileset(tmp_path, "inhead"), 12, (20).to_bytes(8, "little"))
    with pytest.raises(ValueError, match=r"inhead.pgen: block 0 starts at byte 20, inside the header \(28 bytes\)"):
        pgen.load_dosage(bad, **ask)
    bad = patched(example_fileset(tmp_path, "length"), 27, b"\x04")
    with pytest.raises(ValueError, match=r"length.pgen: the record of variant 5 \(4 bytes from byte 41\) leaves the file"):
        pgen.load_dosage(bad, **ask)
    bad = example_fileset(tmp_path, "cut")
    with open(bad + ".pgen", "r+b") as f:
        f.truncate(25)
    with pytest.raises(ValueError, match="cut.pgen: truncated inside the header of block 0"):
        pgen.load_dosage(bad, **ask)
    rng = np.random.default_rng(1)
    two = rng.integers(0, 4, (65537, 5)).astype(np.uint8)
    samples, _, table = simple_fileset(str(tmp_path / "lap"), two, [0] * 65537, chrom="3")
    bad = patched(str(tmp_path / "lap"), 20, (table[65536][0] - 1).to_bytes(8, "little"))
    with pytest.raises(ValueError, match="lap.pgen: block 1 starts at byte .*, which overlaps the records of the block before"):
        pgen.load_dosage(bad, "3", samples[:2], [2, 2])
    # the fixed-width mode has one size
    fixed = example_fileset(tmp_path, "fixed", types=None, mode=0x02)
    assert pgen.load_dosage(fixed, **ask)[1].tolist() == [[0, 1], [0, 0], [0, 1], [2, 2], [0, 0]]
    with open(fixed + ".pgen", "ab") as f:
        f.write(b"\x00")
    with pytest.raises(ValueError, match=r"fixed.pgen: 23 bytes, expected 22 \(12 \+ 5 variants x 2 bytes for 5 samples\)"):
        pgen.load_dosage(fixed, **ask)
    # missing files, and a compressed .pvar
    for ext in (".pvar", ".psam"):
        bad = example_fileset(tmp_path, "no" + ext[1:])
        os.remove(bad + ext)
        assert not pgen.is_fileset(bad)
        with pytest.raises(ValueError, match=rf"no{ext[1:]}\{ext} is not found"):
            pgen.load_dosage(bad + ".pgen", **ask)
    bad = example_fileset(tmp_path, "zst")
    os.rename(bad + ".pvar", bad + ".pvar.zst")
    with pytest.raises(ValueError, match=r"zst.pvar is not found, but .*zst.pvar.zst is: decompress it first"):
        pgen.load_dosage(bad, **ask)
    with pytest.raises(ValueError, match=r"zst.pvar is not found, but .*zst.pvar.zst is: decompress it first"):
        pgen.scan_first_last(bad, "3")
    # a header line that begins otherwise
    bad = example_fileset(tmp_path, "pvarhead")
    text = open(bad + ".pvar").read().replace("#CHROM\tPOS\tID\tREF\tALT", "#CHROM\tID\tPOS\tREF\tALT")
    open(bad + ".pvar", "w").write(text)
    with pytest.raises(ValueError, match="pvarhead.pvar: the header line does not begin with #CHROM POS ID REF ALT"):
        pgen.load_dosage(bad, **ask)
    bad = example_fileset(tmp_path, "psamhead")
    open(bad + ".psam", "w").write("#SID\tIID\n" + "".join(f"x\t{s}\n" for s in "abcde"))
    with pytest.raises(ValueError, match="psamhead.psam: the header line does not begin with #FID IID or #IID"):
        pgen.load_dosage(bad, **ask)
    # samples: the VCF reader's words; a name twice
    with pytest.raises(ValueError) as absent:
        pgen.load_dosage(good, "3", ["a", "zz"], [2, 2])
    assert str(absent.value) == f"samples not found in {good}.psam: zz"
    twice = example_fileset(tmp_path, "twice", samples=["a", "b", "c", "b", "e"])
    with pytest.raises(ValueError, match="sample b occurs twice in .*twice.psam"):
        pgen.load_dosage(twice, **ask)
    assert pgen.load_dosage(twice, "3", ["a", "c"], [2, 2])[1].tolist() == [[0, 2], [0, 0], [0, 0], [2, -2], [0, -2]]
    # a selected multiallelic variant: a comma in ALT, or bit 3 of the vrtype; an unselected one does not matter
    multi = example_fileset(tmp_path, "comma", alt=["C", "C", "C,G", "C", "C"])
    with pytest.raises(ValueError, match=r"comma.pvar: variant 3 is multiallelic \(a comma in ALT\)"):
        pgen.load_dosage(multi, **ask)
    assert pgen.load_dosage(multi, end=250, **ask)[1].tolist() == [[0, 1], [0, 0]]
    multi = patched(example_fileset(tmp_path, "patch"), 21, b"\x1a")  # vrtypes 2, 1 -> 10 (2 + bit 3), 1
    with pytest.raises(ValueError, match=r"patch.pgen: variant 3 \(position 300\) is multiallelic"):
        pgen.load_dosage(multi, **ask)
    assert pgen.load_dosage(multi, start=350, **ask)[1].tolist() == [[2, 2], [0, 0]]
    # ploidy above 2: before anything is read (this fileset does not exist)
    with pytest.raises(ValueError, match="sample b is configured with ploidy 4: a PLINK 2 fileset is read as haploid and diploid hard calls only"):
        pgen.load_dosage(str(tmp_path / "absent"), "3", ["a", "b"], [2, 4])
    # a het in a ploidy-1 slot names the variant and the sample
    with pytest.raises(ValueError, match="heterozygous call of sample b at variant v1 .position 100., but the sample is configured with ploidy 1"):
        pgen.load_dosage(good, "3", ["a", "b"], [1, 1])
    with pytest.raises(ValueError, match="heterozygous call of sample d at variant v5"):
        pgen.load_dosage(good, "3", ["a", "d"], [2, 1], start=450)
    # a selected record that does not parse (a type 1 byte that names no pair of codes); unselected, it does not matter
    bad = patched(example_fileset(tmp_path, "parse"), 36, b"\x04")
    with pytest.raises(ValueError, match=r"parse.pgen: the record of variant v4 \(position 400, vrtype 1, 5 bytes at byte 36\) does not parse"):
        pgen.load_dosage(bad, **ask)
    assert pgen.load_dosage(bad, end=300, **ask)[1].tolist() == [[0, 1], [0, 0], [0, 1]]
    with pytest.raises(ValueError, match=r"the record of variant v5 .* does not parse"):  # ... but as a base it does
        pgen.load_dosage(bad, start=500, **ask)
    # read_data's other options, as for the other filesets
    cfg = load_config("tests/data/test_mixed_ploidy.config.yaml")
    names = sorted({s for g in ("ref", "tgt", "src") for line in open(cfg.populations.get_population(g)) for s in line.split()[1:2]})
    tetra = str(tmp_path / "tetra")
    B.write_fileset(tetra, ["21"] * 3, [1, 2, 3], ["x", "y", "z"], ["A"] * 3, ["C"] * 3, np.zeros((3, len(names)), np.uint8), names)
    kw = dict(chr_name="21", ploidy_config=cfg.ploidies, ref_ind_file=cfg.populations.get_population("ref"),
              tgt_ind_file=cfg.populations.get_population("tgt"), src_ind_file=cfg.populations.get_population("src"))  # fmt: skip
    with pytest.raises(ValueError, match="Failed to read VCF file .*tetra.pgen from 21: sample .* is configured with ploidy 4"):
        read_dosage_data(vcf_file=tetra + ".pgen", **kw)
    with pytest.raises(ValueError, match="a PLINK 2 fileset is read as unphased dosages only"):
        read_data(vcf_file=tetra + ".pgen", **kw)
    # a buffer smaller than a record (and its base)
    with pytest.raises(ValueError, match=r"SAI_AMD_INGEST_BUFFER of 1 bytes is smaller than one record of .*good.pgen \(2 bytes\)"):
        pgen.load_dosage(good, buffer_bytes=1, **ask)
    with pytest.raises(ValueError, match=r"SAI_AMD_INGEST_BUFFER of 5 bytes is smaller than one record of .*good.pgen \(3 bytes and its base of 3\)"):
        pgen.load_dosage(good, buffer_bytes=5, start=300, **ask)


# ---- dispatch, command line, ABI ----


def test_dispatch_order_resident_bytes_and_rank_arguments(tmp_path, monkeypatch):
    from sai_amd import sai as sai_mod
    from sai_amd.utils import eigenstrat, filesets, pgen, plink

    assert filesets.READERS == (plink, eigenstrat, pgen)
    prefix = example_fileset(tmp_path, "d")
    assert pgen.is_fileset(prefix) and pgen.fileset_prefix(prefix + ".pgen") == prefix and not plink.is_fileset(prefix) and not eigenstrat.is_fileset(prefix)
    assert filesets.reader_for(prefix) is pgen and filesets.reader_for(prefix + ".pgen") is pgen and filesets.reader_for(prefix + ".pvar") is None
    assert filesets.name_of(prefix) == "a PLINK 2 fileset" and filesets.cli_source(prefix + ".pgen") == ["--pfile", prefix]
    # resident bytes: variant_ct x sample_ct from the header, whatever the file size (44 bytes here)
    assert os.path.getsize(prefix + ".pgen") == 44 and filesets.resident_bytes(prefix) == filesets.resident_bytes(prefix + ".pgen") == 25
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "10")
    assert sai_mod.chunks_for_memory(prefix + ".pgen") == sai_mod.chunks_for_memory(prefix) == 3
    assert sai_mod._reads_in_one_pass(prefix + ".pgen") is False and sai_mod._reads_in_one_pass(prefix) is False
    argv = sai_mod._score_cli_arguments(prefix + ".pgen", "3", 10, 5, None, "o.tsv", "c.yaml", 2)
    assert argv[:3] == ["score", "--pfile", prefix] and not {"--vcf", "--bfile", "--eigenstrat"} & set(argv)
    assert sai_mod._score_cli_arguments("x.vcf", "3", 10, 5, None, "o.tsv", "c.yaml", 2)[:3] == ["score", "--vcf", "x.vcf"]
    # a bare prefix that also has a .bed keeps the reader it has today; with its extension it is what the extension says
    bed, _ = small_fileset(tmp_path, "both")
    for ext in (".pgen", ".pvar", ".psam"):
        shutil.copy(prefix + ext, bed + ext)
    assert filesets.reader_for(bed) is plink and filesets.reader_for(bed + ".bed") is plink and filesets.reader_for(bed + ".pgen") is pgen
    assert plink.fileset_prefix(bed) == bed and pgen.fileset_prefix(bed) is None and pgen.fileset_prefix(bed + ".pgen") == bed
    # a .bed renamed .pgen is not a PLINK 2 fileset (third byte 01)
    shutil.copy(bed + ".bed", bed + ".pgen")
    assert filesets.reader_for(bed + ".pgen") is None


def test_command_line(tmp_path):
    prefix = example_fileset(tmp_path, "cli")
    bfile, _ = small_fileset(tmp_path, "bed")
    res = sai_cli("score", "--help")
    assert res.returncode == 0 and all(flag in res.stdout for flag in ("--vcf VCF", "--bfile PREFIX", "--eigenstrat PREFIX", "--pfile PREFIX"))
    rest = ["--chr-name", "3", "--output", str(tmp_path / "o.tsv"), "--config", "tests/data/test_sai.config.yaml"]
    # without --pfile the usage errors keep their words
    res = sai_cli("score", *rest)
    assert res.returncode == 2 and "exactly one of the arguments --vcf and --bfile is required" in res.stderr
    res = sai_cli("score", "--vcf", "tests/data/example.vcf", "--bfile", bfile, *rest)
    assert res.returncode == 2 and "exactly one of the arguments --vcf and --bfile is required" in res.stderr and "--pfile" not in res.stderr.split("error:")[1]
    for other in (["--vcf", "tests/data/example.vcf"], ["--bfile", bfile], ["--vcf", "tests/data/example.vcf", "--bfile", bfile]):
        res = sai_cli("score", "--pfile", prefix, *other, *rest)
        assert res.returncode == 2 and "exactly one of the arguments --vcf, --bfile, --eigenstrat and --pfile is required" in res.stderr
    # PREFIX.pgen is taken for PREFIX; a missing file is a usage error, as is a compressed .pvar
    os.remove(prefix + ".psam")
    res = sai_cli("score", "--pfile", prefix + ".pgen", *rest)
    assert res.returncode == 2 and f"{prefix}.psam is not found" in res.stderr
    os.rename(prefix + ".pvar", prefix + ".pvar.zst")
    res = sai_cli("score", "--pfile", prefix, *rest)
    assert res.returncode == 2 and f"{prefix}.pvar is not found, but {prefix}.pvar.zst is: decompress it first" in res.stderr
    assert not (tmp_path / "o.tsv").exists()


def test_header_and_binding_agree():
    """include/saihip_pgen.h, sai_amd/_ffi_pgen.py and the library name the same entry points; the three earlier
    headers and their versions are as they were."""
    from sai_amd import _ffi, _ffi_eigenstrat, _ffi_pgen, _ffi_plink

    names = abi_checks.declared_names("saihip_pgen.h")
    assert names == sorted(_ffi_pgen.SIGNATURES) and len(names) == 8 and all(n.startswith("sai_pgen_") for n in names)
    lib = _ffi_pgen.load()
    version = abi_checks.header_macro("saihip_pgen.h", "SAI_PGEN_ABI_VERSION")
    assert lib.sai_pgen_abi_version() == _ffi_pgen.SAI_PGEN_ABI_VERSION == version == 1
    assert abi_checks.header_macro("saihip_pgen.h", "SAI_PGEN_STATUS_BAD_INDEX") == _ffi_pgen.SAI_PGEN_STATUS_BAD_INDEX == BAD_INDEX
    assert abi_checks.header_macro("saihip_pgen.h", "SAI_PGEN_STATUS_BAD_RECORD") == _ffi_pgen.SAI_PGEN_STATUS_BAD_RECORD == BAD_RECORD
    # the earlier headers: versions, the number of their entry points, and no name of theirs is new
    assert lib.sai_abi_version() == _ffi.SAI_ABI_VERSION == 16
    assert _ffi_plink.load().sai_plink_abi_version() == 1 and _ffi_eigenstrat.load().sai_eigenstrat_abi_version() == 1
    assert len(abi_checks.declared_names("saihip_plink.h")) == 8 == len(_ffi_plink.SIGNATURES)
    assert len(abi_checks.declared_names("saihip_eigenstrat.h")) == 9 == len(_ffi_eigenstrat.SIGNATURES)
    for other in ("saihip.h", "saihip_plink.h", "saihip_eigenstrat.h"):
        assert "pgen" not in (ROOT / "include" / other).read_text().lower()
    assert not any(n.startswith("sai_pgen") for n in [*_ffi.SIGNATURES, *_ffi_plink.SIGNATURES, *_ffi_eigenstrat.SIGNATURES])
    assert not any(n.startswith(("sai_plink_", "sai_eigenstrat_")) for n in _ffi_pgen.SIGNATURES)
    assert lib.sai_pgen_decode(None, None, 0, 0, None, None, None, 1, 1, None, -1, None, 0, None, 0, None, None) == _ffi.SAI_ERR_ARG
    assert b"ctx is NULL" in lib.sai_last_error()


def test_packaging_and_build_lists():
    import __graft_entry__ as entry

    assert "pgen/pgen_index.cpp" in entry.HOST_UNITS
    from sai_amd import _build

    assert "pgen/pgen_decode.hip" in _build.UNITS and "pgen/pgen_index.cpp" in _build.UNITS
    assert {f"csrc/pgen/*.{ext}" for ext in ("hip", "hpp", "cpp")} <= set(abi_checks.package_data_patterns())
    assert ROOT / "include" / "saihip_pgen.h" in _build.PUBLIC_HEADERS
    assert {_build.CSRC / "pgen" / "pgen_codes.hpp", ROOT / "include" / "saihip_pgen.h"} <= set(_build.staleness_inputs())


# ---- corrupted records ----


def corrupted_records(sample_ct=300):
    """-> (bytes, rec, base, codes, bad): a batch of records laid back to back, valid ones (``codes[r]`` = their
    genotypes) between damaged ones (``bad[r]`` = a word on what was done).  A valid type 4 record with three
    groups of a difflist is taken apart and, in turn, truncated inside every part, given a larger L, an index
    past the samples, a repeated index, a varint that runs past the record, wrong group sizes; then the other ways
    a record cannot be read: the byte of type 1, type 5, a base that is missing, of type 2, or outside the batch."""
    rng = np.random.default_rng(77)
    n = sample_ct
    row = np.zeros(n, dtype=np.uint8)
    where = np.sort(rng.permutation(n - 2)[:130])
    row[where] = rng.integers(1, 4, 130)
    where = np.flatnonzero(row)
    L, firsts, sizes, code_bytes, deltas = B.difflist_parts(where, row[where], n)
    assert len(L) == 2 and len(firsts) == 6 and len(sizes) == 2 and len(deltas) == 3
    join = lambda L=L, firsts=firsts, sizes=sizes, code_bytes=code_bytes, deltas=deltas: L + firsts + sizes + code_bytes + b"".join(deltas)  # noqa: E731
    valid = join()
    assert valid == B.encode(row, 4)
    entries = []  # (what, vrtype, record bytes, base entry index or None, codes or None)

    def good(what, kind, codes, base=None):
        entries.append((what, kind, B.encode(codes, kind, entries[base][4] if base is not None else None), base, np.asarray(codes, dtype=np.uint8)))
        return len(entries) - 1

    def bad(what, kind, data, base=None):
        entries.append((what, kind, bytes(data), base, None))

    g4 = good("valid type 4", 4, row)
    part_ends = np.cumsum([len(L), len(firsts), len(sizes), len(code_bytes), len(deltas[0]), len(deltas[1]), len(deltas[2])]).tolist()
    for name, end, size in zip(("L", "firsts", "sizes", "codes", "deltas 0", "deltas 1", "deltas 2"), part_ends, np.diff([0] + part_ends).tolist()):
        bad(f"truncated inside {name}", 4, valid[: end - 1])
        if size > 2:
            bad(f"truncated in the middle of {name}", 4, valid[: end - size // 2])
    bad("empty record", 4, b"")
    bad("L raised by one", 4, join(L=B.varint(131)))
    bad("L raised by a group", 4, join(L=B.varint(130 + 64)))
    bad("L above the sample count", 4, join(L=B.varint(n + 1)))
    bad("L of six varint bytes", 4, b"\x82\x80\x80\x80\x80\x00" + valid[2:])
    bad("first index of the last group past the samples", 4, join(firsts=firsts[:4] + n.to_bytes(2, "little")))
    assert len(B.varint(int(where[-1] - where[-2]))) == 1
    last = deltas[2][:-1] + B.varint(n - int(where[-2]))
    bad("last delta reaches sample_ct", 4, join(deltas=[deltas[0], deltas[1], last]))
    big = deltas[2][:-1] + b"\xff\xff\xff\xff\x0f"
    bad("a delta past 2^32", 4, join(deltas=[deltas[0], deltas[1], big]))
    bad("a delta of zero: an index twice", 4, join(deltas=[deltas[0], b"\x00" + deltas[1][1:], deltas[2]]))
    again = int(where[63]).to_bytes(2, "little")
    bad("a group starts on the last index of the group before", 4, join(firsts=firsts[:2] + again + firsts[4:]))
    bad("a group starts before the group before it ends", 4, join(firsts=firsts[:2] + (0).to_bytes(2, "little") + firsts[4:]))
    bad("the last varint runs past the record", 4, valid[:-1] + bytes([valid[-1] | 0x80]))
    bad("a varint of six bytes", 4, join(deltas=[deltas[0], deltas[1], deltas[2][:-1] + b"\x81\x80\x80\x80\x80\x00"]))
    bad("group size one too small", 4, join(sizes=bytes([sizes[0] - 1 if sizes[0] else 1, sizes[1]])))
    bad("group size one too large", 4, join(sizes=bytes([sizes[0], sizes[1] + 1])))
    bad("group size far too large", 4, join(sizes=bytes([sizes[0], 255])))
    g1 = good("valid type 1", 1, np.where(rng.random(n) < 0.3, 2, 0).astype(np.uint8) | (rng.random(n) < 0.02))
    one = entries[g1][2]
    for b in (0, 4, 7, 8, 10, 12, 255):
        bad(f"type 1 byte {b}", 1, bytes([b]) + one[1:])
    bad("type 1 without its bits", 1, one[: 1 + n // 8 - 3])
    bad("type 1 without its difflist", 1, one[: 1 + -(-n // 8)])
    g0 = good("valid type 0", 0, rng.integers(0, 4, n))
    bad("type 0 one byte short", 0, entries[g0][2][:-1])
    bad("type 5", 5, valid)
    g2 = good("valid type 2 from the type 4", 2, np.where(rng.random(n) < 0.05, 3, row), base=g4)
    g3 = good("valid type 3 from the type 1", 3, B.swap02(entries[g1][4]) ^ (rng.random(n) < 0.03), base=g1)
    bad("type 2 without a base", 2, entries[g2][2])
    bad("type 2 from a type 2", 2, entries[g2][2], base=g2)
    bad("type 3 from a type 5", 3, entries[g3][2], base=len(entries) - 5)
    assert entries[len(entries) - 6][0] == "type 5"
    bad("type 2 from a damaged base", 2, entries[g2][2], base=2)
    bad("type 2 with a damaged difflist", 2, entries[g2][2][:-1], base=g4)
    good("valid type 6", 6, np.where(rng.random(n) < 0.1, 1, 2))
    good("valid type 7, the last record of the batch", 7, np.where(rng.random(n) < 0.01, 0, 3))
    data = b"".join(e[2] for e in entries)
    offsets = np.concatenate(([0], np.cumsum([len(e[2]) for e in entries])))
    rec = [[int(offsets[i]), len(e[2]), e[1]] for i, e in enumerate(entries)]
    base = [[int(offsets[e[3]]), len(entries[e[3]][2]), entries[e[3]][1]] if e[3] is not None else [-1, -1, -1] for e in entries]
    what = [e[0] for e in entries]
    codes = [e[4] for e in entries]
    # spans that do not lie inside the batch
    for name, r, b in (("record past the end of the batch", [len(data) - 3, 4, 7], [-1] * 3), ("record at a negative offset", [-1, 3, 4], [-1] * 3),
                       ("record of negative length", [0, -1, 4], [-1] * 3), ("record far outside", [1 << 40, 3, 4], [-1] * 3),
                       ("base past the end of the batch", rec[g2], [len(data) - 1, 2, 4]), ("base of negative length", rec[g2], [0, -5, 4])):  # fmt: skip
        rec.append(r), base.append(b), what.append(name), codes.append(None)
    rec.append(rec[g4]), base.append([-1] * 3), what.append("valid type 4 once more"), codes.append(row)
    return data, np.array(rec, dtype=np.int64), np.array(base, dtype=np.int64), codes, what


def check_corrupted(out, status, codes, what, cols, ploidies, flips):
    for r, name in enumerate(what):
        if codes[r] is None:
            assert status[r] == BAD_RECORD and not out[r].any(), name
        else:
            want, want_status = expected(codes[r][None, :], cols, ploidies, flips[r : r + 1])
            assert status[r] == want_status[0] and np.array_equal(out[r], want[0]), name


def test_corrupted_records_are_flagged_and_zeroed():
    n = 300
    data, rec, base, codes, what = corrupted_records(n)
    assert sum(c is None for c in codes) >= 45 and sum(c is not None for c in codes) >= 8
    rng = np.random.default_rng(2)
    flips = rng.integers(0, 2, len(rec)).astype(np.uint8)
    for cols, ploidies in ((list(range(n)), [2] * n), (rng.permutation(n)[:17].tolist(), [2] * 17)):
        out, status = decode_host(data, rec, base, flips, n, cols, ploidies)
        check_corrupted(out, status, codes, what, cols, ploidies, flips)
    # caller's mistakes are BAD_INDEX on a sound record, and a het at ploidy 1 is the lowest such slot
    good = [r for r, c in enumerate(codes) if c is not None]
    cols, ploidies = [0, n, 5, -1, 7], [2, 2, 3, 2, 1]
    out, status = decode_host(data, rec[good], base[good], flips[good], n, cols, ploidies)
    want, want_status = expected(np.stack([codes[r] for r in good]), cols, ploidies, flips[good])
    assert np.array_equal(out, want) and np.array_equal(status, want_status) and (status == BAD_INDEX).all()
    cols, ploidies = list(range(n)), [1] * n
    out, status = decode_host(data, rec[good], base[good], flips[good], n, cols, ploidies)
    want, want_status = expected(np.stack([codes[r] for r in good]), cols, ploidies, flips[good])
    assert np.array_equal(out, want) and np.array_equal(status, want_status) and (status > 0).any() and (status < n).all()


# ---- the sanitizer run ----


@pytest.fixture(scope="module")
def dump_program(tmp_path_factory):
    """tests/native/pgen_dump.cpp + the host units of libsaihip under ASan + UBSan, the runtimes linked in."""
    return native_build.dump_program("pgen_dump", tmp_path_factory)["san"]


def test_host_code_is_clean_under_asan_ubsan(tmp_path, dump_program):
    """The index and the host decoder, run (not only compiled) under the sanitizers: on the filesets of the random
    cases the same positions, rows, flips and dosages as the library; on the corrupted records the same statuses,
    read from a heap block of exactly the batch's size."""
    from sai_amd.utils import pgen

    for seed in (1, 2, 3, 5):
        case = random_case(seed, tmp_path)
        rng = np.random.default_rng(seed)
        prefix = str(tmp_path / f"p{seed}")
        B.from_bed_fileset(case["prefix"], prefix, random_types(rng, len(case["chroms"])), wide_types=bool(seed & 1), len_bytes=1 + seed % 3,
                           pvar=dict(header=seed != 2), psam=["#FID IID", "#IID", "fam"][seed % 3])  # fmt: skip
        here = case["positions"]
        names, ploidies = [s for s, _ in case["request"]], [p for _, p in case["request"]]
        for anc in (None, case["anc"]):
            for start, end in [(None, None), (here[1], here[-1] - 1)]:
                res = run_dump(dump_program, prefix, "7", start, end, anc, case["request"])
                assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
                lines = res.stdout.splitlines()
                pos, dos, n_matched, n_anc = pgen.load_dosage(prefix, "7", names, ploidies, start, end, anc)
                first, last = pgen.scan_first_last(prefix, "7")
                assert lines[0].split()[:6] == ["info", str(len(pos)), str(n_matched), str(n_anc), str(first), str(last)]
                assert lines[0].split()[6:] == [str(len(case["samples"])), str(len(case["chroms"])), "16"]
                table = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], dtype=np.int64).reshape(len(pos), 4 + len(names))
                assert table[:, 0].tolist() == pos.tolist() and not table[:, 3].any() and np.array_equal(table[:, 4:], dos)
    n = 300
    data, rec, base, codes, what = corrupted_records(n)
    flips = np.arange(len(rec)) % 2
    (tmp_path / "records.bin").write_bytes(data)
    (tmp_path / "records.txt").write_text("".join(" ".join(str(int(v)) for v in [*rec[r], *base[r], flips[r]]) + "\n" for r in range(len(rec))))
    res = native_build.run_native(dump_program, ["--records", tmp_path / "records.bin", tmp_path / "records.txt", n])
    assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
    table = np.array([[int(v) for v in ln.split()] for ln in res.stdout.splitlines()], dtype=np.int64)
    check_corrupted(table[:, 1:].astype(np.int8), table[:, 0], codes, what, list(range(n)), [2] * n, flips.astype(np.uint8))
    # refusals come back as a status and a message, also there
    res = run_dump(dump_program, prefix, "7", None, None, None, [("nobody", 2)])
    assert res.returncode == 3 and "samples not found" in res.stderr and "Sanitizer" not in res.stderr
    res = run_dump(dump_program, str(tmp_path / "absent"), "7", None, None, None, [("s0", 2)])
    assert res.returncode == 3 and "is not found" in res.stderr and "Sanitizer" not in res.stderr
