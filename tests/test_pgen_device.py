"""PLINK 2 filesets on the GPU: ``sai_pgen_decode`` against the host decoder byte for byte (every record type and
base type, the index-width and packing boundaries of the sample count, the group boundaries of a difflist, damaged
records), the streaming reader against the host reader, and ``score`` on a fileset against ``score`` on the VCF of
the same genotypes (byte-identical TSV, .U.log and .Q.log), one process and two ranks."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pgen_builder as B
from conftest import ROOT
from test_pgen_cpu import ALL_TYPES, BAD_INDEX, BAD_RECORD, check_corrupted, corrupted_records, expected, random_matrix, random_types, tables_of
from test_plink_cpu import FIXTURES, fileset_from_vcf, random_case
from test_plink_device import score_files, slot_lists

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


def decode_both(eng, data, rec, base, flip, n, cols, ploidies, first_col=-1, uniform=0, out_row0=0, tail_rows=0):
    """(host out, host status, device out, device status, the untouched rows around the device call)."""
    import torch

    from sai_amd import _ffi, _ffi_pgen

    lib = _ffi_pgen.load()
    data = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    rec, base = np.ascontiguousarray(rec, dtype=np.int64), np.ascontiguousarray(base, dtype=np.int64)
    flip, cols, ploidies = np.ascontiguousarray(flip, np.uint8), np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(ploidies, np.int32)
    n_out, n_slots = len(rec), len(cols)
    h_out = np.empty((n_out, n_slots), dtype=np.int8)
    h_st = np.empty(n_out, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _ffi.check(lib.sai_pgen_decode_host(p(data), len(data), n_out, p(rec), p(base), p(flip), n, n_slots, p(cols), p(ploidies), p(h_out),
                                        p(h_st), 3))  # fmt: skip
    dev = lambda a: torch.from_numpy(a).to(eng.device)  # noqa: E731
    d_data, d_rec, d_base, d_flip, d_cols, d_pl = dev(data), dev(rec), dev(base), dev(flip), dev(cols), dev(ploidies)
    d_out = torch.full((out_row0 + n_out + tail_rows, n_slots), 77, dtype=torch.int8, device=eng.device)
    d_st = torch.full((n_out,), -5, dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_pgen_decode(eng.ctx, eng._ptr(d_data), len(data), n_out, eng._ptr(d_rec), eng._ptr(d_base), eng._ptr(d_flip), n, n_slots,
                                   None if first_col >= 0 else eng._ptr(d_cols), first_col, None if uniform else eng._ptr(d_pl), uniform,
                                   C.c_void_p(d_out.data_ptr()), out_row0, eng._ptr(d_st),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    around = np.concatenate([got[:out_row0].ravel(), got[out_row0 + n_out :].ravel()])
    return h_out, h_st, got[out_row0 : out_row0 + n_out], d_st.cpu().numpy(), around


DIFFLIST_LENGTHS = (0, 1, 63, 64, 65, 128, 129)


def kernel_case(n, rng):
    """-> (matrix, types): every type behind every base type, then rows whose difflists have the lengths at the
    group boundaries and the longest the row allows, against a constant and against a base."""
    rows, types = [], []
    for base_type in (0, 1, 4, 6, 7):
        block = random_matrix(rng, 6, n)
        if base_type in (4, 6, 7):
            block[0] = np.where(rng.random(n) < 0.05, rng.integers(0, 4, n), {4: 0, 6: 2, 7: 3}[base_type])
        block[1:] = block[0]
        for r in range(1, 6):
            hit = rng.random(n) < [0.0, 0.02, 0.3, 0.02, 1.0][r - 1]
            block[r][hit] = rng.integers(0, 4, int(hit.sum()))
        block[4] = B.swap02(block[4])
        rows.extend(block)
        types.extend([base_type, 2, 2, 3, 3, 2])
    for L in sorted({min(L, n) for L in DIFFLIST_LENGTHS} | {n}):
        where = np.sort(rng.permutation(n)[:L])
        for kind, fill in ((4, 0), (6, 2), (7, 3), (2, None), (1, None)):
            start = rows[-1].copy() if fill is None else np.full(n, fill, dtype=np.uint8)
            if kind == 1:
                start = np.where(rng.random(n) < 0.4, 3, 1).astype(np.uint8)
            row = start.copy()
            row[where] = (start[where] + rng.integers(1, 4, L)) % 4  # L entries that differ
            if kind == 1:
                row[where] = np.where(np.isin(row[where], (1, 3)), 0, row[where])  # ... from both common codes
            rows.append(row.astype(np.uint8))
            types.append(kind)
    rows.extend(random_matrix(rng, 8, n))
    types.extend([None] * 8)
    return np.array(rows, dtype=np.uint8), types


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2002, 65537])
def test_kernel_equals_host_decoder(eng, n):
    rng = np.random.default_rng(2000 + n)
    matrix, types = kernel_case(n, rng)
    if n == 65537:  # a few dozen rows, with deltas of three varint bytes
        keep = list(range(0, 12)) + list(range(30, len(matrix), 3))
        matrix, types = matrix[keep[:36]], [types[k] for k in keep[:36]]
        types[0] = 0
        types = [t if t not in (2, 3) or k else 0 for k, t in enumerate(types)]
        sparse = np.zeros(n, dtype=np.uint8)
        sparse[[0, 20000, 40000, 65536]] = [1, 2, 3, 1]
        matrix = np.vstack([matrix, sparse, sparse])
        types += [4, 2]
        assert B.encode(sparse, 4).endswith(b"\xa0\x9c\x01" * 2 + b"\xc0\xc7\x01")
    data, table = B.build_pgen(matrix, types, wide_types=True, len_bytes=4)
    kinds = {(t[2] & 7, table[t[3]][2] & 7 if t[3] >= 0 else -1) for t in table}
    if n != 65537:
        assert {k for k, _ in kinds} == set(ALL_TYPES) and {b for k, b in kinds if k in (2, 3)} == {0, 1, 4, 6, 7}
    rec, base = tables_of(table)
    # one damaged and one reserved record among them: BAD_RECORD, zeros, and the neighbours untouched
    rec = np.vstack([rec, [rec[1][0], rec[1][1], 5], [rec[0][0], max(0, rec[0][1] - 1), rec[0][2]]])
    base = np.vstack([base, [[-1] * 3] * 2])
    codes = np.vstack([matrix, matrix[:2]])
    broken = np.zeros(len(rec), dtype=bool)
    broken[-2:] = True
    no_het = np.where(codes == 1, 2, codes).astype(np.uint8)
    clean_data, clean_table = B.build_pgen(no_het[:-2], types, wide_types=True, len_bytes=4)
    clean_rec, clean_base = tables_of(clean_table)
    clean_rec = np.vstack([clean_rec, [clean_rec[1][0], clean_rec[1][1], 5], [clean_rec[0][0], max(0, clean_rec[0][1] - 1), clean_rec[0][2]]])
    clean_base = np.vstack([clean_base, [[-1] * 3] * 2])
    subsets = [np.arange(len(rec)), np.sort(rng.choice(len(rec), size=len(rec) // 3, replace=False)), np.array([len(rec) - 3])]
    seen_flag = seen_clean = 0
    for name, cols in slot_lists(n, rng):
        for rows in subsets:
            flip = rng.integers(0, 2, size=len(rows)).astype(np.uint8)  # flipped and unflipped rows mixed
            for kind in ("two", "one", "one-clean", "mixed"):
                use = (clean_data, clean_rec, clean_base, no_het) if kind == "one-clean" else (data, rec, base, codes)
                ploidies = {"two": np.full(len(cols), 2), "one": np.ones(len(cols)), "one-clean": np.ones(len(cols)),
                            "mixed": rng.integers(1, 3, size=len(cols))}[kind].astype(np.int32)  # fmt: skip
                uniform = int(ploidies[0]) if (ploidies == ploidies[0]).all() else 0
                consecutive = bool(np.array_equal(cols, np.arange(cols[0], cols[0] + len(cols))))
                for promise in ([False, True] if (consecutive or uniform) else [False]):
                    first_col = int(cols[0]) if promise and consecutive else -1
                    uni = uniform if promise else 0
                    row0, tail = (int(rng.integers(0, 9)), 2) if promise else (0, 0)
                    h_out, h_st, d_out, d_st, around = decode_both(eng, use[0], use[1][rows], use[2][rows], flip, n, cols, ploidies, first_col,
                                                                   uni, row0, tail)  # fmt: skip
                    where = (n, name, len(rows), kind, promise)
                    assert np.array_equal(d_out, h_out), where
                    assert np.array_equal(d_st, h_st), where
                    assert (around == 77).all(), where  # nothing outside the call's rows is written
                    assert (h_st[broken[rows]] == BAD_RECORD).all() and not h_out[broken[rows]].any() and not (h_st == BAD_INDEX).any()
                    sound = ~broken[rows]  # the host decoder against the table restated in test_pgen_cpu
                    want, want_st = expected(use[3][rows][sound], cols, ploidies, flip[sound])
                    assert np.array_equal(h_out[sound], want) and np.array_equal(h_st[sound], want_st), where
                    if kind in ("two", "one-clean"):
                        assert not h_st[~broken[rows]].any()
                        seen_clean += 1
                    elif ((h_st > 0) & (h_st < BAD_RECORD)).any():
                        seen_flag += 1
    assert seen_clean and (seen_flag or n == 1)


def test_kernel_restates_the_table_and_refuses_bad_indices(eng):
    """Independent of the host decoder: the four codes at both ploidies, kept and flipped; a column or a ploidy
    outside its range is flagged, written as 0 and never dereferenced."""
    table = {(2, 0): [0, 1, 2, -2], (2, 1): [2, 1, 0, 4], (1, 0): [0, 0, 1, -1], (1, 1): [1, 0, 0, 2]}
    data = bytes([0b11100100])  # samples 0..3 hold the codes 0, 1, 2, 3
    cols = np.arange(4, dtype=np.int32)
    for (ploidy, flipped), want in table.items():
        pl = np.full(4, ploidy, dtype=np.int32)
        for uniform in (0, ploidy):
            h_out, h_st, d_out, d_st, _ = decode_both(eng, data, [[0, 1, 0]], [[-1] * 3], [flipped], 4, cols, pl, 0 if uniform else -1, uniform)
            assert d_out.tolist() == [want] == h_out.tolist()
            assert d_st.tolist() == h_st.tolist() == [4 - 1 if ploidy == 1 else 0]
    data = bytes([0xAA] * 5)  # 20 samples of code 2: rows wide enough for the fast path
    h_out, h_st, d_out, d_st, _ = decode_both(eng, data, [[0, 5, 0], [0, 5, 0]], [[-1] * 3] * 2, [0, 1], 20, [0, 20, 6, -2, 3], [2, 2, 3, 2, 2])
    assert h_st.tolist() == d_st.tolist() == [BAD_INDEX] * 2 and h_out.tolist() == d_out.tolist() == [[2, 0, 0, 0, 2], [0, 0, 0, 0, 0]]
    h_out, h_st, d_out, d_st, _ = decode_both(eng, data, [[0, 5, 0], [1, 5, 0], [0, 5, 4]], [[-1] * 3] * 3, [1, 1, 1], 20, np.arange(20), [2] * 20, 0, 2)
    assert h_st.tolist() == d_st.tolist() == [0, BAD_RECORD, BAD_RECORD] and h_out.tolist() == d_out.tolist() == [[0] * 20] * 3


def test_corrupted_records_on_the_kernel(eng):
    """The damaged records of test_pgen_cpu: the host's statuses, zeroed rows, nothing written outside the rows."""
    n = 300
    data, rec, base, codes, what = corrupted_records(n)
    rng = np.random.default_rng(4)
    flips = rng.integers(0, 2, len(rec)).astype(np.uint8)
    for cols, ploidies, first_col, uniform, row0 in ((np.arange(n), [2] * n, -1, 0, 0), (np.arange(n), [2] * n, 0, 2, 3),
                                                      (rng.permutation(n)[:17], [2] * 17, -1, 2, 1), (np.arange(40, 73), [2] * 33, 40, 0, 5)):  # fmt: skip
        h_out, h_st, d_out, d_st, around = decode_both(eng, data, rec, base, flips, n, cols, ploidies, first_col, uniform, row0, 2)
        check_corrupted(h_out, h_st, codes, what, list(cols), ploidies, flips)
        assert np.array_equal(d_st, h_st) and np.array_equal(d_out, h_out) and (around == 77).all()


def test_streaming_reader_equals_host_reader(eng, tmp_path, monkeypatch):
    from sai_amd.utils import pgen

    split_bases = 0
    for seed in (3, 4, 11):
        case = random_case(seed, tmp_path)
        rng = np.random.default_rng(seed)
        prefix = str(tmp_path / f"p{seed}")
        types = random_types(rng, len(case["chroms"]), kinds=(None, 0, 1, 2, 2, 3, 3, 4, 6, 7))
        table = B.from_bed_fileset(case["prefix"], prefix, types, wide_types=bool(seed & 1), len_bytes=1 + seed % 3)
        longest = max(t[1] for t in table)
        names, ploidies = [s for s, _ in case["request"]], [p for _, p in case["request"]]
        here = case["positions"]
        for anc in (None, case["anc"]):
            for chrom, start, end in [("7", None, None), ("7", here[2], here[-2]), ("absent", None, None), ("7", here[-1] + 1, None)]:
                want = pgen.load_dosage(prefix, chrom, names, ploidies, start, end, anc)
                if chrom == "absent":
                    assert want[0].size == 0 and want[2] == 0
                for cap in (2 * longest, 4096, None):  # a record or two per batch (a base and its rows part), a few KiB, one batch
                    if cap == 4096:
                        monkeypatch.setenv("SAI_AMD_INGEST_BUFFER", "4096")
                        got = pgen.load_dosage_device(eng, prefix + ".pgen", chrom, names, ploidies, start, end, anc)
                        monkeypatch.delenv("SAI_AMD_INGEST_BUFFER")
                    else:
                        got = pgen.load_dosage_device(eng, prefix, chrom, names, ploidies, start, end, anc, buffer_bytes=cap)
                    assert got[0].dtype == np.int32 and got[0].tolist() == want[0].tolist() and got[2:] == want[2:]
                    assert tuple(got[1].shape) == want[1].shape and np.array_equal(got[1].cpu().numpy(), want[1]), (seed, chrom, start, anc, cap)
        idx = pgen._Index(eng.lib, prefix, "7", names, ploidies, None, None, None, 2)
        split_bases += sum(1 for b in idx.batches(2 * longest) if b[5][0][0] == 0 and b[3][0][0] == 0 and len(b[5]) > 1)
    assert split_bases > 3  # batches whose first row's base went out with an earlier batch and is fetched again
    # a wide fileset: many batches, the consecutive-run fast path and a gather, het at ploidy 1, a damaged record
    rng = np.random.default_rng(8)
    n_samples, n = 2002, 1500
    samples = [f"w{i}" for i in range(n_samples)]
    matrix = random_matrix(rng, n, n_samples)
    prefix = str(tmp_path / "wide")
    types = random_types(rng, n)  # the smallest encoding and every forced type, mixed
    table = B.write_fileset(prefix, ["5"] * n, np.cumsum(rng.integers(1, 30, n)).tolist(), [f"v{k}" for k in range(n)], ["A"] * n, ["C"] * n,
                            matrix, samples, types, len_bytes=2)  # fmt: skip
    assert {t[2] for t in table} == set(ALL_TYPES)
    for pick in (samples[100:1900], [samples[i] for i in rng.permutation(n_samples)[:300]], samples[7:9]):
        want = pgen.load_dosage(prefix, "5", pick, [2] * len(pick))
        cols = [samples.index(s) for s in pick]
        assert np.array_equal(want[1], expected(matrix, cols, [2] * len(cols), [0] * n)[0])
        for cap in (20000, None):
            trace = {}
            got = pgen.load_dosage_device(eng, prefix, "5", pick, [2] * len(pick), buffer_bytes=cap, trace=trace)
            assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1].cpu().numpy(), want[1])
            assert trace["index"] > 0 and trace["file_read"] > 0 and 0 < trace["pgen_bytes"] and "h2d" not in trace
    trace = {"serial": True}
    pgen.load_dosage_device(eng, prefix, "5", samples[:64], [2] * 64, buffer_bytes=20000, trace=trace)
    assert trace["h2d"] > 0 and trace["decode"] > 0
    with pytest.raises(ValueError, match=r"heterozygous call of sample w\d at variant v\d+ .*configured with ploidy 1"):
        pgen.load_dosage_device(eng, prefix, "5", samples[:10], [1] * 10, buffer_bytes=20000)
    with pytest.raises(ValueError, match=r"SAI_AMD_INGEST_BUFFER of 3 bytes is smaller than one record of .*wide.pgen"):
        pgen.load_dosage_device(eng, prefix, "5", samples[:10], [2] * 10, buffer_bytes=3)
    victim = next(k for k, t in enumerate(table) if t[2] == 1 and k > 700)
    with open(prefix + ".pgen", "r+b") as f:
        f.seek(table[victim][0])
        f.write(b"\x07")
    with pytest.raises(ValueError, match=rf"wide.pgen: the record of variant v{victim} .*vrtype 1.* does not parse"):
        pgen.load_dosage_device(eng, prefix, "5", samples[:10], [2] * 10, buffer_bytes=20000)
    got = pgen.load_dosage_device(eng, prefix, "5", samples[:10], [2] * 10, end=int(want[0][victim - 1]))  # the staging survives an error
    assert np.array_equal(got[1].cpu().numpy(), expected(matrix[:victim], range(10), [2] * 10, [0] * victim)[0])


SCORE_CASES = [("tests/data/example.vcf", "21", "tests/data/test_sai.config.yaml", None), *FIXTURES]


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", SCORE_CASES)
def test_score_on_a_fileset_writes_the_files_of_the_vcf(eng, in_repo_root, tmp_path, monkeypatch, vcf, chrom, cfgfile, anc):
    """With and without --anc-alleles (the cases), both ingest routes, PREFIX.pgen and the bare PREFIX."""
    bed = str(tmp_path / "fx")
    fileset_from_vcf(vcf, bed)
    prefix = str(tmp_path / "pfx")
    n_var = sum(1 for line in open(bed + ".bim") if line.strip())
    table = B.from_bed_fileset(bed, prefix, random_types(np.random.default_rng(len(vcf)), n_var))
    assert len({t[2] for t in table}) > 3
    monkeypatch.setenv("SAI_AMD_INGEST", "device")
    want = score_files(vcf, chrom, cfgfile, anc, tmp_path / "vcf" / "s.tsv")
    assert len(want[".tsv"].splitlines()) > 1
    for mode, source in (("device", prefix + ".pgen"), ("host", prefix)):
        monkeypatch.setenv("SAI_AMD_INGEST", mode)
        got = score_files(source, chrom, cfgfile, anc, tmp_path / f"set_{mode}" / "s.tsv")
        assert got == want, (mode, source)


def test_score_with_two_ranks(eng, in_repo_root, tmp_path, monkeypatch):
    """Two ranks on this box's one GPU, gloo for the gather; started by ``score`` itself as a child job with --pfile."""
    vcf, chrom, cfgfile, anc = FIXTURES[1][0], FIXTURES[1][1], FIXTURES[1][2], None
    win = (10000, 5000)
    bed = str(tmp_path / "fx")
    fileset_from_vcf(vcf, bed)
    prefix = str(tmp_path / "pfx")
    B.from_bed_fileset(bed, prefix)
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES", raising=False)
    want = score_files(vcf, chrom, cfgfile, anc, tmp_path / "vcf" / "s.tsv", win)
    assert len(want[".tsv"].splitlines()) > 1
    assert score_files(prefix + ".pgen", chrom, cfgfile, anc, tmp_path / "one" / "s.tsv", win) == want
    out = tmp_path / "two" / "s.tsv"
    code = ("import sai_amd.stats; from sai_amd.sai import score; "
            f"score(vcf_file={prefix + '.pgen'!r}, chr_name={chrom!r}, win_len={win[0]}, win_step={win[1]}, anc_allele_file={anc!r}, "
            f"output_file={str(out)!r}, config={cfgfile!r}, num_workers=2)")  # fmt: skip
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SAI_AMD_DIST_BACKEND="gloo")
    res = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert {p.name[1:]: p.read_bytes() for p in out.parent.glob("s*")} == want
