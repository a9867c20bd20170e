"""BCF files on the GPU: ``sai_bcf_decode`` against the host decoder byte for byte (status included), the streaming
reader against the host reader, and ``score`` on a BCF against ``score`` on the VCF it was written from
(byte-identical TSV, .U.log and .Q.log): one process, three chunks, the host route and two ranks."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bcf_builder as B
from conftest import ROOT
from test_bcf_cpu import FILES, SHAPES, anc_file, region_of, samples_of, small_buffer, vcf_text

pytestmark = pytest.mark.gpu

RANGE, BAD_VALUE, BAD_INDEX = 1, 2, 3
DTYPE = {1: np.int8, 2: np.int16, 4: np.int32}
N_ROWS = 48
GUARD = 64


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


_batches = {}


def batch_of(width, length, n_cols):
    """(bytes, gt_off, flip): N_ROWS GT arrays of n_cols samples x `length` values, packed WITHOUT the alignment padding
    -- a few junk bytes between them instead, so that they start at every offset mod 16.  Ordinary calls of
    alleles 0 .. 3; every fourth row also holds end-of-vector, both missing forms, the largest allele that fits int8, one
    that overflows it (wider types; a triploid sum of 62s at width 1) and a reserved value.  Computed once per shape."""
    key = (width, length, n_cols)
    if key not in _batches:
        rng = np.random.default_rng(1000 * width + 10 * length + n_cols)
        info = np.iinfo(DTYPE[width])
        top = 62 if width == 1 else 126  # the largest allele whose haploid dosage (and the value itself) fits
        special = [info.min + 1, info.min, 0, 1, (top + 1) << 1, (top + 1) << 1 | 1, info.min + 2, -3] + ([(300 + 1) << 1] if width > 1 else [])
        parts, offs, at = [], [], 1
        for r in range(N_ROWS):
            v = ((rng.integers(0, 4, size=(n_cols, length)) + 1) << 1 | rng.integers(0, 2, size=(n_cols, length))).astype(np.int64)
            if r % 4 == 0:
                hit = rng.random((n_cols, length)) < (0.6 if r % 8 == 0 else 0.1)
                v[hit] = rng.choice(special[:6] if r % 8 else special, size=int(hit.sum()))
            if r == 12:
                v[4 % n_cols, :] = (top + 1) << 1  # one sample all of whose alleles are the largest: three of 62 leave int8
            end = at + n_cols * length * width
            gap = (7 * (r + 1) + 1 - end) % 16  # row r starts at 7 r + 1 mod 16: every residue, three times
            parts += [v.astype(DTYPE[width]).tobytes(), bytes(rng.integers(0, 256, size=gap, dtype=np.uint8))]
            offs.append(at)
            at = end + gap
        data = np.frombuffer(b"\x5a" + b"".join(parts), dtype=np.uint8).copy()
        off = np.array(offs, dtype=np.int64)
        assert len(set((off % 16).tolist())) == 16
        _batches[key] = (data, off, (rng.random(N_ROWS) < 0.5).astype(np.uint8))
    return _batches[key]


def decode_both(eng, data, off, width, length, flip, n_cols, cols, ploidies, first_col=-1, uniform=0, out_row0=0, tail_rows=2):
    """(host out, host status, device out, device status, the block around the device call, the guards intact)."""
    import torch

    from sai_amd import _ffi, _ffi_bcf

    lib = _ffi_bcf.load()
    n_out, n_slots = len(off), len(cols)
    h_out = np.empty((n_out, n_slots), dtype=np.int8)
    h_st = np.empty(n_out, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _ffi.check(lib.sai_bcf_decode_host(p(data), len(data), n_out, p(off), p(width), p(length), p(flip), n_cols, n_slots, p(cols), p(ploidies),
                                       p(h_out), p(h_st), 3))  # fmt: skip
    dev = lambda a: torch.from_numpy(a).to(eng.device)  # noqa: E731
    guarded = np.concatenate([np.full(GUARD, 0xA5, np.uint8), data, np.full(GUARD, 0xA5, np.uint8)])
    d_data, d_off, d_width, d_len, d_flip, d_cols, d_pl = dev(guarded), dev(off), dev(width), dev(length), dev(flip), dev(cols), dev(ploidies)
    d_out = torch.full((out_row0 + n_out + tail_rows, n_slots), 77, dtype=torch.int8, device=eng.device)
    d_st = torch.full((n_out,), -5, dtype=torch.int32, device=eng.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _ffi.check(lib.sai_bcf_decode(eng.ctx, C.c_void_p(d_data.data_ptr() + GUARD), len(data), n_out, eng._ptr(d_off), eng._ptr(d_width), eng._ptr(d_len),
                                  eng._ptr(d_flip), n_cols, n_slots, None if first_col >= 0 else eng._ptr(d_cols), first_col,
                                  None if uniform else eng._ptr(d_pl), uniform, C.c_void_p(d_out.data_ptr()), out_row0, eng._ptr(d_st), stream))  # fmt: skip
    torch.cuda.synchronize()
    block = d_out.cpu().numpy()
    intact = np.array_equal(d_data.cpu().numpy(), guarded) and (block[:out_row0] == 77).all() and (block[out_row0 + n_out :] == 77).all()
    return h_out, h_st, block[out_row0 : out_row0 + n_out], d_st.cpu().numpy(), intact


@pytest.mark.parametrize("length", [1, 2, 3])
@pytest.mark.parametrize("width", [1, 2, 4])
def test_decode_equals_the_host_decoder(eng, width, length):
    """n_samples in {1, 15, 16, 17, 65, 130}; ploidy uniform 1, 2, 3 and mixed; consecutive columns from 0 and 3 (the promised
    form) and a permuted list with repeats; out_row0 in {0, 23}; rows flipped and not; guard bytes around both buffers."""
    seen = set()
    for n in (1, 15, 16, 17, 65, 130):
        n_cols = n + 5
        data, off, flip = batch_of(width, length, n_cols)
        widths, lengths = np.full(N_ROWS, width, np.uint8), np.full(N_ROWS, length, np.int32)
        rng = np.random.default_rng(n)
        for form in (1, 2, 3, "mixed"):
            ploidies = np.full(n, form, np.int32) if form != "mixed" else rng.integers(1, 5, size=n).astype(np.int32)
            for columns in (0, 3, "list"):
                cols = np.arange(columns, columns + n, dtype=np.int32) if columns != "list" else rng.integers(0, n_cols, size=n).astype(np.int32)
                for out_row0 in (0, 23):
                    h_out, h_st, d_out, d_st, intact = decode_both(
                        eng, data, off, widths, lengths, flip, n_cols, cols, ploidies, first_col=-1 if columns == "list" else columns,
                        uniform=0 if form == "mixed" else form, out_row0=out_row0)  # fmt: skip
                    where = (width, length, n, form, columns, out_row0)
                    assert np.array_equal(d_st, h_st) and np.array_equal(d_out, h_out) and intact, where
                    seen |= set(h_st.tolist())
    assert {0, BAD_VALUE} <= seen and BAD_INDEX not in seen and (RANGE in seen or (width == 1 and length < 3))


def test_decode_mixed_widths_and_lengths_in_one_batch(eng):
    """A row names its own width and length: rows of all nine shapes in one batch, in the promised form and not."""
    n, n_cols = 33, 38
    parts, off, widths, lengths, at = [], [], [], [], 0
    for width in (1, 2, 4):
        for length in (1, 2, 3):
            data, o, _ = batch_of(width, length, n_cols)
            parts.append(data)
            off.append(o + at)
            widths.append(np.full(N_ROWS, width, np.uint8))
            lengths.append(np.full(N_ROWS, length, np.int32))
            at += len(data)
    rng = np.random.default_rng(9)
    order = rng.permutation(9 * N_ROWS)
    data, off, widths, lengths = np.concatenate(parts), np.concatenate(off)[order], np.concatenate(widths)[order], np.concatenate(lengths)[order]
    flip = (rng.random(len(off)) < 0.5).astype(np.uint8)
    for uniform in (1, 2, 0):
        ploidies = np.full(n, uniform, np.int32) if uniform else rng.integers(1, 5, size=n).astype(np.int32)
        for first_col in (2, -1):
            cols = np.arange(2, 2 + n, dtype=np.int32) if first_col >= 0 else rng.permutation(n_cols)[:n].astype(np.int32)
            h_out, h_st, d_out, d_st, intact = decode_both(eng, data, off, widths, lengths, flip, n_cols, cols, ploidies, first_col, uniform, out_row0=5)
            assert np.array_equal(d_st, h_st) and np.array_equal(d_out, h_out) and intact, (uniform, first_col)


def test_decode_checks_every_index_before_use(eng):
    """Offsets, lengths and widths that leave the batch, columns and ploidies outside their range: BAD_INDEX, zeros, and the
    rows next to them as the host writes them."""
    n, n_cols = 20, 24
    data, off, flip = batch_of(1, 2, n_cols)
    widths, lengths = np.full(N_ROWS, 1, np.uint8), np.full(N_ROWS, 2, np.int32)
    off, widths, lengths = off.copy(), widths.copy(), lengths.copy()
    off[3], off[7], off[11] = -1, len(data) - 10, len(data) + 1
    widths[5], widths[9] = 3, 0
    lengths[13], lengths[17] = -2, 1 << 30
    bad_rows = [3, 5, 7, 9, 11, 13, 17]
    for first_col, uniform in ((2, 2), (-1, 0)):
        cols, ploidies = np.arange(2, 2 + n, dtype=np.int32), np.full(n, 2, np.int32)
        h_out, h_st, d_out, d_st, intact = decode_both(eng, data, off, widths, lengths, flip, n_cols, cols, ploidies, first_col, uniform, out_row0=1)
        assert np.array_equal(d_st, h_st) and np.array_equal(d_out, h_out) and intact
        assert (h_st[bad_rows] == BAD_INDEX).all() and not h_out[bad_rows].any() and (np.delete(h_st, bad_rows) != BAD_INDEX).all()
    cols, ploidies = np.arange(2, 2 + n, dtype=np.int32), np.full(n, 2, np.int32)
    cols[4], cols[6], ploidies[8], ploidies[10] = -1, n_cols, 0, 65
    h_out, h_st, d_out, d_st, intact = decode_both(eng, data, batch_of(1, 2, n_cols)[1], np.full(N_ROWS, 1, np.uint8), np.full(N_ROWS, 2, np.int32),
                                                   flip, n_cols, cols, ploidies)
    assert np.array_equal(d_st, h_st) and np.array_equal(d_out, h_out) and intact
    assert (h_st == BAD_INDEX).all() and not h_out[:, [4, 6, 8, 10]].any() and h_out[:, [0, 1, 2, 3]].any()


@pytest.mark.parametrize("name,chrom,given_anc", FILES, ids=[f[0] for f in FILES])
def test_load_dosage_device_equals_load_dosage(eng, tmp_path, monkeypatch, name, chrom, given_anc):
    """The CPU test's files, with the default staging buffer and one of a few KiB, so that batches are cut between any two rows."""
    from sai_amd.utils import bcf

    samples = samples_of(name)
    anc, region = anc_file(name, chrom, given_anc, tmp_path), region_of(name, chrom)
    requests = [(samples, [2] * len(samples)), (samples[1:], [1] * (len(samples) - 1)), (samples[::-1], [1 + k % 4 for k in range(len(samples))]),
                (samples + samples[:2], [3] * len(samples) + [1, 2])]  # fmt: skip
    for k, shape in enumerate(SHAPES[1:3]):
        path = B.write_bcf(tmp_path / f"{k}.bcf", vcf_text(name), **shape)
        for cap in (None, small_buffer(name)):
            if cap is None:
                monkeypatch.delenv("SAI_AMD_INGEST_BUFFER", raising=False)
            else:
                monkeypatch.setenv("SAI_AMD_INGEST_BUFFER", str(cap))
            for names, ploidies in requests:
                for a, (start, end) in ((None, (None, None)), (anc, region)):
                    want = bcf.load_dosage(path, chrom, names, ploidies, start, end, a)
                    got = bcf.load_dosage_device(eng, path, chrom, names, ploidies, start, end, a)
                    assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1].cpu().numpy(), want[1]) and got[2:] == want[2:], (shape, cap)
    bcf.release_buffers(eng)


def test_a_flagged_row_is_named_by_the_host_route(eng, tmp_path):
    from sai_amd.utils import bcf
    from test_bcf_cpu import _gt

    samples = samples_of("example.vcf")
    hook = lambda i, r: i == 4 and _gt(r)["values"].__setitem__(2 * 6 + 1, -126)  # noqa: E731
    path = B.write_bcf(tmp_path / "reserved.bcf", vcf_text("example.vcf"), on_record=hook)
    with pytest.raises(ValueError, match=r"record 21:\d+: the GT vector of sample ind7 holds a reserved value: the record is damaged"):
        bcf.load_dosage_device(eng, path, "21", samples, [2] * len(samples))
    assert bcf.load_dosage_device(eng, path, "21", samples, [1] * len(samples))[1].shape[0] > 4


def score_files(source, chrom, cfgfile, anc, out, win=(20000, 10000), num_workers=1):
    from sai_amd.sai import score

    score(vcf_file=source, chr_name=chrom, win_len=win[0], win_step=win[1], anc_allele_file=anc, output_file=str(out), config=cfgfile,
          num_workers=num_workers)  # fmt: skip
    return {p.name[len(out.stem) :]: p.read_bytes() for p in out.parent.glob(out.stem + "*")}


SCORE_CASES = [
    ("tests/data/example.vcf", "21", "tests/data/test_sai.config.yaml", None),
    ("tests/data/test.with.outgroup.vcf.gz", "1", "tests/data/test.with.outgroup.config.yaml", "tests/data/test.with.outgroup.anc.alleles"),
    ("tests/data/test.mixed.ploidy.data.vcf.gz", "21", "tests/data/test_mixed_ploidy.config.yaml", "tests/data/test.mixed.ploidy.data.anc.alleles"),
]  # fmt: skip


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", SCORE_CASES)
def test_score_on_a_bcf_writes_the_files_of_the_vcf(eng, in_repo_root, tmp_path, monkeypatch, vcf, chrom, cfgfile, anc):
    """With and without --anc-alleles (the cases), both ingest routes, two shapes of the file."""
    monkeypatch.setenv("SAI_AMD_INGEST", "device")
    want = score_files(vcf, chrom, cfgfile, anc, tmp_path / "vcf" / "s.tsv")
    assert len(want[".tsv"].splitlines()) > 1
    for k, shape in enumerate((dict(), dict(width=2, idx=True, extra_before=True, extra_after=True, member_size=977, eof=False))):
        path = B.write_bcf(tmp_path / f"calls{k}.bcf", B.read_vcf_text(vcf), **shape)
        for mode in ("device", "host"):
            monkeypatch.setenv("SAI_AMD_INGEST", mode)
            assert score_files(path, chrom, cfgfile, anc, tmp_path / f"bcf{k}_{mode}" / "s.tsv") == want, (shape, mode)


def seeded_block(tmp_path):
    """4 000 sites x (16 + 16 + 2) diploids with 1 % missing calls as VCF text, and a U + Q + DD configuration over it."""
    rng = np.random.default_rng(20261)
    n, sizes = 4000, (16, 16, 2)
    p = rng.random(n) ** 3
    ref = rng.binomial(2, p[:, None] * 0.2, size=(n, sizes[0]))
    tgt = rng.binomial(2, np.clip(p[:, None] * 2, 0, 1), size=(n, sizes[1]))
    src = np.repeat(np.where(rng.random((n, 1)) < 0.5, 2, 0), sizes[2], axis=1)
    calls = np.array(["0|0", "0|1", "1|1", ".|."])[np.where(rng.random((n, sum(sizes))) < 0.01, 3, np.concatenate([ref, tgt, src], axis=1))]
    samples = [f"r{i}" for i in range(sizes[0])] + [f"t{i}" for i in range(sizes[1])] + [f"n{i}" for i in range(sizes[2])]
    positions = np.cumsum(rng.integers(1, 50, n)).tolist()
    lines = ["##fileformat=VCFv4.2", "##contig=<ID=4>", '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples)]  # fmt: skip
    lines += [f"4\t{pos}\tv{k}\tG\tT\t.\tPASS\t.\tGT\t" + "\t".join(row) for k, (pos, row) in enumerate(zip(positions, calls))]
    text = "\n".join(lines) + "\n"
    vcf = tmp_path / "block.vcf"
    vcf.write_text(text)
    for group, pop, members in (("ref", "R", samples[:16]), ("tgt", "T", samples[16:32]), ("src", "S", samples[32:])):
        (tmp_path / f"{group}.list").write_text("".join(f"{pop}\t{s}\n" for s in members))
    uq = "    ref:\n      R: 0.3\n    tgt:\n      T: {x}\n    src:\n      S: \"=1\"\n"
    cfg = tmp_path / "block.yaml"
    cfg.write_text("statistics:\n  U:\n" + uq.format(x=0.2) + "  Q:\n" + uq.format(x=0.95) + "  DD: true\n"
                   "ploidies:\n  ref:\n    R: 2\n  tgt:\n    T: 2\n  src:\n    S: 2\n"
                   f"populations:\n  ref: \"{tmp_path}/ref.list\"\n  tgt: \"{tmp_path}/tgt.list\"\n  src: \"{tmp_path}/src.list\"\n")  # fmt: skip
    return str(vcf), B.write_bcf(tmp_path / "block.bcf", text), str(cfg), n * sum(sizes)


def test_score_on_a_seeded_block_three_chunks_and_two_ranks(eng, in_repo_root, tmp_path, monkeypatch):
    from sai_amd import sai as sai_mod

    vcf, path, cfg, n_genotypes = seeded_block(tmp_path)
    win = (5000, 2500)
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES", raising=False)
    monkeypatch.delenv("SAI_AMD_INGEST", raising=False)
    want = score_files(vcf, "4", cfg, None, tmp_path / "vcf" / "s.tsv", win)
    assert set(want) == {".tsv", ".U.log", ".Q.log"} and len(want[".tsv"].splitlines()) > 30
    assert len(want[".U.log"].splitlines()) > 1 and len(want[".Q.log"].splitlines()) > 1
    assert score_files(path, "4", cfg, None, tmp_path / "one" / "s.tsv", win) == want
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", str(-(-n_genotypes // 3)))  # n_records_total x n_samples int8 genotypes: three chunks
    assert sai_mod.chunks_for_memory(path) == 3
    assert score_files(path, "4", cfg, None, tmp_path / "three" / "s.tsv", win) == want
    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    assert score_files(path, "4", cfg, None, tmp_path / "three_host" / "s.tsv", win) == want
    monkeypatch.delenv("SAI_AMD_INGEST")
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES")
    # two ranks on this box's one GPU, gloo for the gather; started by `score` itself as a child job with --vcf
    out = tmp_path / "two" / "s.tsv"
    code = ("import sai_amd.stats; from sai_amd.sai import score; "
            f"score(vcf_file={path!r}, chr_name='4', win_len={win[0]}, win_step={win[1]}, anc_allele_file=None, "
            f"output_file={str(out)!r}, config={cfg!r}, num_workers=2)")  # fmt: skip
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SAI_AMD_DIST_BACKEND="gloo")
    res = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert {p.name[1:]: p.read_bytes() for p in out.parent.glob("s*")} == want
