"""EIGENSOFT filesets on the GPU: ``sai_eigenstrat_decode`` (text and packed) and
``sai_eigenstrat_decode_transposed`` against the host decoder byte for byte, the table restated without the host
decoder, the streaming reader against the host reader, and ``score`` on each of the three encodings against
``score`` on the VCF of the same genotypes (byte-identical TSV, .U.log and .Q.log), one process and two ranks."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_eigenstrat_cpu import ENCODINGS, eigenstrat_from_plink, eigenstrat_of_case, write_eigenstrat
from test_plink_cpu import FIXTURES, fileset_from_vcf, random_case
from test_plink_device import score_files, seeded_block, slot_lists

pytestmark = pytest.mark.gpu

TEXT, PACKED, TRANSPOSED = 1, 2, 3
HET = 1  # g = 1: one copy of each allele
BAD_INDEX, BAD_CHAR = 0x7FFFFFFF, 0x7FFFFFFE
# by g = 0, 1, 2, missing
TABLE = {(2, 0): [2, 1, 0, -2], (2, 1): [0, 1, 2, 4], (1, 0): [1, 0, 0, -1], (1, 1): [0, 0, 1, 2]}


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


def decode_both(eng, encoding, records, record_bytes, n_batch, first_code, rib, flip, n_cols, cols, ploidies, first_col=-1, uniform=0,
                out_row0=0, tail_rows=0):  # fmt: skip
    """(host out, host status, device out, device status, the untouched rows around the device call)."""
    import torch

    from sai_amd import _ffi, _ffi_eigenstrat

    lib = _ffi_eigenstrat.load()
    n_out, n_slots = len(rib), len(cols)
    h_out = np.empty((n_out, n_slots), dtype=np.int8)
    h_st = np.empty(n_out, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _ffi.check(lib.sai_eigenstrat_decode_host(encoding, p(records), n_batch, record_bytes, first_code, n_out, p(rib), p(flip), n_cols,
                                              n_slots, p(cols), p(ploidies), p(h_out), p(h_st), 3))  # fmt: skip
    dev = lambda a: torch.from_numpy(a).to(eng.device)  # noqa: E731
    d_rec, d_rib, d_flip, d_cols, d_pl = dev(records), dev(rib), dev(flip), dev(cols), dev(ploidies)
    d_out = torch.full((out_row0 + n_out + tail_rows, n_slots), 77, dtype=torch.int8, device=eng.device)
    d_st = torch.full((n_out,), -5, dtype=torch.int32, device=eng.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if encoding == TRANSPOSED:
        _ffi.check(lib.sai_eigenstrat_decode_transposed(eng.ctx, eng._ptr(d_rec), n_cols, record_bytes, first_code, n_batch, n_out,
                                                        eng._ptr(d_rib), eng._ptr(d_flip), n_slots, eng._ptr(d_cols), eng._ptr(d_pl),
                                                        C.c_void_p(d_out.data_ptr()), out_row0, eng._ptr(d_st), stream))  # fmt: skip
    else:
        _ffi.check(lib.sai_eigenstrat_decode(eng.ctx, encoding, eng._ptr(d_rec), n_batch, record_bytes, n_out, eng._ptr(d_rib),
                                             eng._ptr(d_flip), n_cols, n_slots, None if first_col >= 0 else eng._ptr(d_cols), first_col,
                                             None if uniform else eng._ptr(d_pl), uniform, C.c_void_p(d_out.data_ptr()), out_row0,
                                             eng._ptr(d_st), stream))  # fmt: skip
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    around = np.concatenate([got[:out_row0].ravel(), got[out_row0 + n_out :].ravel()])
    return h_out, h_st, got[out_row0 : out_row0 + n_out], d_st.cpu().numpy(), around


def packed_without_het(records):
    """Every 01 pair of the bytes turned into 11 (missing)."""
    out = records | ((records & 0x55) << 1)
    assert not (out & ~(out >> 1) & 0x55).any()
    return out


def ploidies_of(kind, n, rng):
    return {"two": np.full(n, 2), "one": np.ones(n), "one-clean": np.ones(n), "mixed": rng.integers(1, 3, size=n)}[kind].astype(np.int32)


@pytest.mark.parametrize("encoding", [PACKED, TEXT], ids=["packed", "text"])
@pytest.mark.parametrize("n_ind", [1, 3, 4, 5, 63, 64, 65, 191, 193, 2002])
def test_variant_major_kernel_equals_host_decoder(eng, n_ind, encoding):
    rng = np.random.default_rng(3000 + 7 * n_ind + encoding)
    n_batch = 41 if n_ind > 1000 else 173
    if encoding == PACKED:  # 191 and 193 individuals straddle the 48-byte minimum record
        record_bytes = max(48, (n_ind + 3) // 4)
        records = rng.integers(0, 256, size=n_batch * record_bytes, dtype=np.uint8)  # any byte string is a valid record
        no_het = packed_without_het(records)
        code = lambda data, r, c: (int(data[r * record_bytes + c // 4]) >> (6 - 2 * (c % 4))) & 3  # noqa: E731
    else:
        record_bytes = n_ind + 1
        lines = np.frombuffer(b"0129", dtype=np.uint8)[rng.integers(0, 4, size=(n_batch, n_ind))]
        records = np.concatenate([lines, np.full((n_batch, 1), 10, dtype=np.uint8)], axis=1).ravel()
        no_het = np.where(records == ord("1"), ord("2"), records).astype(np.uint8)
        code = lambda data, r, c: "0129".index(chr(data[r * record_bytes + c]))  # noqa: E731
    subsets = [np.arange(n_batch), np.sort(rng.choice(n_batch, size=n_batch // 3, replace=False)), np.array([n_batch - 1])]
    seen_flag = seen_clean = 0
    for name, cols in slot_lists(n_ind, rng):
        for rib in subsets:
            rib = np.ascontiguousarray(rib, dtype=np.int32)
            flip = rng.integers(0, 2, size=len(rib)).astype(np.uint8)  # flipped and unflipped rows mixed
            for kind in ("two", "one", "one-clean", "mixed"):
                data = no_het if kind == "one-clean" else records
                ploidies = ploidies_of(kind, len(cols), rng)
                uniform = int(ploidies[0]) if (ploidies == ploidies[0]).all() else 0
                consecutive = bool(np.array_equal(cols, np.arange(cols[0], cols[0] + len(cols))))
                for promise in ([False, True] if (consecutive or uniform) else [False]):
                    first_col = int(cols[0]) if promise and consecutive else -1
                    uni = uniform if promise else 0
                    row0, tail = (int(rng.integers(1, 9)), 2) if promise else (0, 0)
                    h_out, h_st, d_out, d_st, around = decode_both(eng, encoding, data, record_bytes, n_batch, 0, rib, flip, n_ind, cols,
                                                                   ploidies, first_col, uni, row0, tail)  # fmt: skip
                    where = (n_ind, name, len(rib), kind, promise)
                    assert np.array_equal(d_out, h_out), where
                    assert np.array_equal(d_st, h_st), where
                    assert (around == 77).all(), where  # nothing outside the call's rows is written
                    assert not (h_st >= BAD_CHAR).any()
                    if kind in ("two", "one-clean"):
                        assert not h_st.any()
                        seen_clean += 1
                    elif h_st.any():
                        seen_flag += 1
                        r = int(np.flatnonzero(h_st)[0])  # the flag names the lowest ploidy-1 slot of the row that holds g = 1
                        s = len(cols) - int(h_st[r])
                        assert ploidies[s] == 1 and code(data, int(rib[r]), int(cols[s])) == HET
                        assert not any(ploidies[t] == 1 and code(data, int(rib[r]), int(cols[t])) == HET for t in range(s))
    assert seen_clean and (seen_flag or n_ind == 1)


@pytest.mark.parametrize("n_variants", [1, 3, 4, 5, 63, 64, 65, 1021])
@pytest.mark.parametrize("n_staged", [1, 3, 64, 65, 300])
def test_transposed_kernel_equals_host_decoder(eng, n_staged, n_variants):
    rng = np.random.default_rng(5000 + 13 * n_staged + n_variants)
    seen_flag = seen_clean = 0
    for first_code in range(4):  # the first variant of the batch at every place inside its byte
        stride = -(-((first_code + n_variants + 3) // 4) // 16) * 16
        staged = rng.integers(0, 256, size=n_staged * stride, dtype=np.uint8)
        no_het = packed_without_het(staged)
        ribs = [np.arange(n_variants), np.sort(rng.choice(n_variants, size=max(1, n_variants // 3), replace=False)),  # dense, sparse,
                rng.permutation(n_variants)[: max(1, n_variants // 2)]]  # any order  # fmt: skip
        lists = slot_lists(n_staged, rng) + [("one slot", np.array([n_staged // 2], dtype=np.int32))]
        for k, (name, cols) in enumerate(lists):
            rib = np.ascontiguousarray(ribs[(k + first_code) % 3], dtype=np.int32)
            flip = rng.integers(0, 2, size=len(rib)).astype(np.uint8)
            for kind in ("two", "one-clean", "mixed"):
                data = no_het if kind == "one-clean" else staged
                ploidies = ploidies_of(kind, len(cols), rng)
                row0, tail = (int(rng.integers(1, 9)), 2) if kind != "two" else (0, 0)
                h_out, h_st, d_out, d_st, around = decode_both(eng, TRANSPOSED, data, stride, n_variants, first_code, rib, flip, n_staged,
                                                               cols, ploidies, out_row0=row0, tail_rows=tail)  # fmt: skip
                where = (n_staged, n_variants, first_code, name, kind)
                assert np.array_equal(d_out, h_out), where
                assert np.array_equal(d_st, h_st), where
                assert (around == 77).all(), where
                assert not (h_st >= BAD_CHAR).any()
                if kind != "mixed":
                    assert not h_st.any()
                    seen_clean += 1
                elif h_st.any():
                    seen_flag += 1
                    r = int(np.flatnonzero(h_st)[0])
                    s = len(cols) - int(h_st[r])
                    at = first_code + int(rib[r])
                    code = lambda c: (int(data[c * stride + at // 4]) >> (6 - 2 * (at % 4))) & 3  # noqa: E731
                    assert ploidies[s] == 1 and code(int(cols[s])) == HET
                    assert not any(ploidies[t] == 1 and code(int(cols[t])) == HET for t in range(s))
    assert seen_clean and (seen_flag or n_staged * n_variants < 10)


def test_kernels_restate_the_table_and_refuse_bad_indices(eng):
    """Independent of the host decoder: the four values at both ploidies, kept and flipped, in all three encodings;
    an index outside its range is flagged, written as 0 and never dereferenced; so is a character that is no call."""
    z = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    packed = np.zeros(48, dtype=np.uint8)
    packed[0] = 0b00011011  # individuals 0..3 hold g = 0, 1, 2, missing
    text = np.frombuffer(b"0129\n", dtype=np.uint8).copy()
    turned = np.zeros(4 * 16, dtype=np.uint8)  # four staged individuals, one variant each: g = 0, 1, 2, missing at code 2 of the byte
    turned[0::16] = np.array([0, 1, 2, 3], dtype=np.uint8) << 2
    cols = np.arange(4, dtype=np.int32)
    for (ploidy, flipped), want in TABLE.items():
        pl = np.full(4, ploidy, dtype=np.int32)
        flip = np.array([flipped], np.uint8)
        status = [4 - 1 if ploidy == 1 else 0]
        for uniform in (0, ploidy):
            for encoding, data, record_bytes in ((PACKED, packed, 48), (TEXT, text, 5)):
                h_out, h_st, d_out, d_st, _ = decode_both(eng, encoding, data, record_bytes, 1, 0, z(0), flip, 4, cols, pl,
                                                          0 if uniform else -1, uniform)  # fmt: skip
                assert d_out.tolist() == [want] == h_out.tolist() and d_st.tolist() == h_st.tolist() == status
        h_out, h_st, d_out, d_st, _ = decode_both(eng, TRANSPOSED, turned, 16, 1, 2, z(0), flip, 4, cols, pl)
        assert d_out.tolist() == [want] == h_out.tolist() and d_st.tolist() == h_st.tolist() == status
    # variant-major: a record, a column or a ploidy outside its range
    rows = np.full(2 * 48, 0xAA, dtype=np.uint8)  # g = 2 everywhere
    h_out, h_st, d_out, d_st, _ = decode_both(eng, PACKED, rows, 48, 2, 0, z(0, 3, -1, 1), np.zeros(4, np.uint8), 7, z(0, 7, 6, -2),
                                              z(2, 2, 3, 2))  # fmt: skip
    assert h_st.tolist() == d_st.tolist() == [BAD_INDEX] * 4 and h_out.tolist() == d_out.tolist() == [[0] * 4] * 4
    wide = np.full(3 * 48, 0xAA, dtype=np.uint8)  # records wide enough for the fast path
    h_out, h_st, d_out, d_st, _ = decode_both(eng, PACKED, wide, 48, 3, 0, z(2, 3), np.ones(2, np.uint8), 20, np.arange(20, dtype=np.int32),
                                              np.full(20, 2, np.int32), 0, 2)  # fmt: skip
    assert h_st.tolist() == d_st.tolist() == [0, BAD_INDEX] and h_out.tolist() == d_out.tolist() == [[2] * 20, [0] * 20]
    # text: a character outside 0 1 2 9, on the general and on the fast path
    line = np.frombuffer(b"012901290129012X0129\n" + b"2" * 20 + b"\n", dtype=np.uint8).copy()
    for first_col, uniform in ((-1, 0), (0, 2)):
        h_out, h_st, d_out, d_st, _ = decode_both(eng, TEXT, line, 21, 2, 0, z(0, 1), np.zeros(2, np.uint8), 20, np.arange(20, dtype=np.int32),
                                                  np.full(20, 2, np.int32), first_col, uniform)  # fmt: skip
        assert h_st.tolist() == d_st.tolist() == [BAD_CHAR, 0]
        assert h_out.tolist() == d_out.tolist() == [[2, 1, 0, -2] * 3 + [2, 1, 0, 0] + [2, 1, 0, -2], [0] * 20]
    # transposed: a variant, a staged individual or a ploidy outside its range
    staged = np.full(3 * 16, 0xAA, dtype=np.uint8)
    h_out, h_st, d_out, d_st, around = decode_both(eng, TRANSPOSED, staged, 16, 9, 1, z(0, 9, -1, 8), np.zeros(4, np.uint8), 3, z(0, 3, 2, -2, 1),
                                                   z(2, 2, 3, 2, 2), out_row0=3, tail_rows=1)  # fmt: skip
    assert h_st.tolist() == d_st.tolist() == [BAD_INDEX] * 4 and (around == 77).all()
    assert h_out.tolist() == d_out.tolist() == [[0, 0, 0, 0, 0], [0] * 5, [0] * 5, [0, 0, 0, 0, 0]]
    h_out, h_st, d_out, d_st, _ = decode_both(eng, TRANSPOSED, staged, 16, 9, 1, z(0, 9, 8), np.ones(3, np.uint8), 3, z(2, 0, 1), z(2, 1, 2))
    assert h_st.tolist() == d_st.tolist() == [0, BAD_INDEX, 0] and h_out.tolist() == d_out.tolist() == [[2, 1, 2], [0, 0, 0], [2, 1, 2]]


def test_streaming_reader_equals_host_reader(eng, tmp_path, monkeypatch):
    from sai_amd.utils import eigenstrat

    for seed in (3, 4, 11):
        case = random_case(seed, tmp_path)
        names, ploidies = [s for s, _ in case["request"]], [p for _, p in case["request"]]
        here = case["positions"]
        for encoding in ENCODINGS:
            prefix = eigenstrat_of_case(case, encoding, final_newline=seed != 4)
            for anc in (None, case["anc"]):
                for chrom, start, end in [("7", None, None), ("7", here[2], here[-2]), ("absent", None, None), ("7", here[-1] + 1, None)]:
                    want = eigenstrat.load_dosage(prefix, chrom, names, ploidies, start, end, anc)
                    if chrom == "absent":
                        assert want[0].size == 0 and want[2] == 0
                    for cap in (230, 4096, None):  # three or four records (16 bytes per individual when transposed), a few KiB, one batch
                        if cap == 4096:
                            monkeypatch.setenv("SAI_AMD_INGEST_BUFFER", "4096")
                            got = eigenstrat.load_dosage_device(eng, prefix + ".geno", chrom, names, ploidies, start, end, anc)
                            monkeypatch.delenv("SAI_AMD_INGEST_BUFFER")
                        else:
                            got = eigenstrat.load_dosage_device(eng, prefix, chrom, names, ploidies, start, end, anc, buffer_bytes=cap)
                        assert got[0].dtype == np.int32 and got[0].tolist() == want[0].tolist() and got[2:] == want[2:]
                        assert tuple(got[1].shape) == want[1].shape and np.array_equal(got[1].cpu().numpy(), want[1]), (seed, encoding, cap)
    # a wide fileset: many batches of several records, the consecutive-run fast path and a gather; the transposed
    # batches are 16 bytes per individual wide: 61 variants, so every batch boundary but each fourth falls inside a byte
    rng = np.random.default_rng(8)
    samples = [f"w{i}" for i in range(2002)]
    n = 3000
    g = rng.integers(0, 4, size=(n, 2002)).astype(np.uint8)
    kw = dict(chroms=["5"] * n, positions=np.cumsum(rng.integers(1, 30, n)).tolist(), ids=[f"v{k}" for k in range(n)], ref=["C"] * n, alt=["A"] * n,
              g=g, samples=samples)  # fmt: skip
    for encoding in ENCODINGS:
        prefix = str(tmp_path / f"wide_{encoding}")
        write_eigenstrat(prefix, encoding, **kw)
        for pick in (samples[100:1900], [samples[i] for i in rng.permutation(2002)[:300]], samples[7:9]):
            want = eigenstrat.load_dosage(prefix, "5", pick, [2] * len(pick))
            for cap in (40000, None):
                trace = {}
                got = eigenstrat.load_dosage_device(eng, prefix, "5", pick, [2] * len(pick), buffer_bytes=cap, trace=trace)
                assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1].cpu().numpy(), want[1]), (encoding, len(pick), cap)
                assert trace["index"] > 0 and trace["file_read"] > 0 and trace["geno_bytes"] > 0 and "h2d" not in trace
        if encoding == "transposed":
            idx = eigenstrat._Index(eng.lib, prefix, "5", samples[100:1900], [2] * 1800, None, None, None, 4)
            firsts = [b.first_code for b in idx.batches(40000)]
            assert len(firsts) > 40 and set(firsts) == {0, 1, 2, 3}
        trace = {"serial": True}
        eigenstrat.load_dosage_device(eng, prefix, "5", samples[:64], [2] * 64, buffer_bytes=40000, trace=trace)
        assert trace["h2d"] > 0 and trace["decode"] > 0
        with pytest.raises(ValueError, match=r"heterozygous call .* of sample w\d at variant v\d+ .*configured with ploidy 1"):
            eigenstrat.load_dosage_device(eng, prefix, "5", samples[:10], [1] * 10, buffer_bytes=40000)
    with pytest.raises(ValueError, match=r"SAI_AMD_INGEST_BUFFER of 500 bytes is smaller than one row of .*wide_packed.geno \(501 bytes\)"):
        eigenstrat.load_dosage_device(eng, str(tmp_path / "wide_packed"), "5", samples[:10], [2] * 10, buffer_bytes=500)
    with pytest.raises(ValueError, match=r"SAI_AMD_INGEST_BUFFER of 9 bytes is smaller than one byte for each of the 10 requested individuals"):
        eigenstrat.load_dosage_device(eng, str(tmp_path / "wide_transposed"), "5", samples[:10], [2] * 10, buffer_bytes=9)


SCORE_CASES = [("tests/data/example.vcf", "21", "tests/data/test_sai.config.yaml", None), *FIXTURES]


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", SCORE_CASES)
def test_score_on_a_fileset_writes_the_files_of_the_vcf(eng, in_repo_root, tmp_path, monkeypatch, vcf, chrom, cfgfile, anc):
    """With and without --anc-alleles (the cases), all three encodings, both ingest routes."""
    bed = str(tmp_path / "fx")
    fileset_from_vcf(vcf, bed)
    monkeypatch.setenv("SAI_AMD_INGEST", "device")
    want = score_files(vcf, chrom, cfgfile, anc, tmp_path / "vcf" / "s.tsv")
    assert len(want[".tsv"].splitlines()) > 1
    for encoding in ENCODINGS:
        prefix = eigenstrat_from_plink(bed, str(tmp_path / encoding), encoding)
        for mode, source in (("device", prefix + ".geno"), ("host", prefix)):
            monkeypatch.setenv("SAI_AMD_INGEST", mode)
            got = score_files(source, chrom, cfgfile, anc, tmp_path / f"{encoding}_{mode}" / "s.tsv")
            assert got == want, (encoding, mode)


@pytest.fixture(scope="module")
def block(tmp_path_factory):
    """The seeded block of test_plink_device, and the files ``score`` writes for its VCF."""
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    tmp = tmp_path_factory.mktemp("block")
    vcf, bed, cfg = seeded_block(tmp)
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        want = score_files(vcf, "4", cfg, None, tmp / "vcf" / "s.tsv", (5000, 2500))
    finally:
        os.chdir(cwd)
    assert set(want) == {".tsv", ".U.log", ".Q.log"} and len(want[".tsv"].splitlines()) > 150
    return tmp, bed, cfg, want


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_score_on_a_seeded_block_one_process_three_chunks_and_two_ranks(eng, in_repo_root, block, monkeypatch, encoding):
    tmp, bed, cfg, want = block
    win = (5000, 2500)
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES", raising=False)
    prefix = eigenstrat_from_plink(bed, str(tmp / f"block_{encoding}"), encoding)
    assert score_files(prefix + ".geno", "4", cfg, None, tmp / f"one_{encoding}" / "s.tsv", win) == want
    from sai_amd import sai as sai_mod

    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "900000")  # 2.44 MB of int8 genotypes: three chunks or more (48-byte minimum record)
    resident = os.path.getsize(prefix + ".geno") * (1 if encoding == "text" else 4)
    assert sai_mod.chunks_for_memory(prefix + ".geno") == -(-resident // 900000) >= 3
    assert score_files(prefix, "4", cfg, None, tmp / f"three_{encoding}" / "s.tsv", win) == want
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES")
    # two ranks on this box's one GPU, gloo for the gather; started by `score` itself as a child job with --eigenstrat
    out = tmp / f"two_{encoding}" / "s.tsv"
    code = ("import sai_amd.stats; from sai_amd.sai import score; "
            f"score(vcf_file={prefix + '.geno'!r}, chr_name='4', win_len={win[0]}, win_step={win[1]}, anc_allele_file=None, "
            f"output_file={str(out)!r}, config={cfg!r}, num_workers=2)")  # fmt: skip
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SAI_AMD_DIST_BACKEND="gloo")
    res = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert {p.name[1:]: p.read_bytes() for p in out.parent.glob("s*")} == want
