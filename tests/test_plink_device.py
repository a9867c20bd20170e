"""PLINK 1 filesets on the GPU: ``sai_plink_decode`` against the host decoder byte for byte, the streaming
reader against the host reader, and ``score`` on a fileset against ``score`` on the VCF of the same
genotypes (byte-identical TSV, .U.log and .Q.log), one process and two ranks."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_plink_cpu import FIXTURES, HET, HOM_A1, HOM_A2, MISSING, fileset_from_vcf, random_case, write_fileset, write_vcf

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


def decode_both(eng, rows, row_bytes, rib, flip, n_cols, cols, ploidies, first_col=-1, uniform=0, out_row0=0, tail_rows=0):
    """(host out, host status, device out, device status, the untouched rows around the device call)."""
    import torch

    from sai_amd import _ffi, _ffi_plink

    lib = _ffi_plink.load()
    n_out, n_slots = len(rib), len(cols)
    n_batch = len(rows) // row_bytes if row_bytes else 0
    h_out = np.empty((n_out, n_slots), dtype=np.int8)
    h_st = np.empty(n_out, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _ffi.check(lib.sai_plink_decode_host(p(rows), n_batch, row_bytes, n_out, p(rib), p(flip), n_cols, n_slots, p(cols), p(ploidies),
                                         p(h_out), p(h_st), 3))  # fmt: skip
    dev = lambda a: torch.from_numpy(a).to(eng.device)  # noqa: E731
    d_rows, d_rib, d_flip, d_cols, d_pl = dev(rows), dev(rib), dev(flip), dev(cols), dev(ploidies)
    d_out = torch.full((out_row0 + n_out + tail_rows, n_slots), 77, dtype=torch.int8, device=eng.device)
    d_st = torch.full((n_out,), -5, dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_plink_decode(eng.ctx, eng._ptr(d_rows), n_batch, row_bytes, n_out, eng._ptr(d_rib), eng._ptr(d_flip), n_cols,
                                    n_slots, None if first_col >= 0 else eng._ptr(d_cols), first_col,
                                    None if uniform else eng._ptr(d_pl), uniform, C.c_void_p(d_out.data_ptr()), out_row0,
                                    eng._ptr(d_st), C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    around = np.concatenate([got[:out_row0].ravel(), got[out_row0 + n_out :].ravel()])
    return h_out, h_st, got[out_row0 : out_row0 + n_out], d_st.cpu().numpy(), around


def slot_lists(n_fam, rng):
    """(name, columns) over the paths of the kernel: all columns, one consecutive run, a reversed list, a list
    with repeats, two slots out of many."""
    lists = [("all", np.arange(n_fam))]
    lo = int(rng.integers(0, n_fam))
    hi = int(rng.integers(lo, n_fam)) + 1
    lists.append(("run", np.arange(lo, hi)))
    lists.append(("reversed", np.arange(n_fam)[::-1]))
    lists.append(("repeats", rng.integers(0, n_fam, size=min(n_fam + 3, 300))))
    lists.append(("two", np.array([n_fam - 1, n_fam // 2])))
    return [(name, np.ascontiguousarray(c, dtype=np.int32)) for name, c in lists]


@pytest.mark.parametrize("n_fam", [1, 3, 4, 5, 63, 64, 65, 2002, 10007])
def test_kernel_equals_host_decoder(eng, n_fam):
    from sai_amd import _ffi_plink

    rng = np.random.default_rng(1000 + n_fam)
    row_bytes = (n_fam + 3) // 4
    n_batch = 41 if n_fam > 1000 else 173
    rows = rng.integers(0, 256, size=n_batch * row_bytes, dtype=np.uint8)  # any byte string is a valid row
    no_het = rows.copy()  # every 10 pair turned into 11
    no_het |= (no_het >> 1) & 0x55 & ~(no_het & 0x55)
    assert not ((no_het >> 1) & ~no_het & 0x55).any()
    subsets = [np.arange(n_batch), np.sort(rng.choice(n_batch, size=n_batch // 3, replace=False)), np.array([n_batch - 1])]
    seen_flag = seen_clean = 0
    for name, cols in slot_lists(n_fam, rng):
        for rib in subsets:
            rib = np.ascontiguousarray(rib, dtype=np.int32)
            flip = rng.integers(0, 2, size=len(rib)).astype(np.uint8)  # flipped and unflipped rows mixed
            for kind in ("two", "one", "one-clean", "mixed"):
                data = no_het if kind == "one-clean" else rows
                ploidies = {"two": np.full(len(cols), 2), "one": np.ones(len(cols)), "one-clean": np.ones(len(cols)),
                            "mixed": rng.integers(1, 3, size=len(cols))}[kind].astype(np.int32)  # fmt: skip
                uniform = int(ploidies[0]) if (ploidies == ploidies[0]).all() else 0
                consecutive = bool(np.array_equal(cols, np.arange(cols[0], cols[0] + len(cols))))
                for promise in ([False, True] if (consecutive or uniform) else [False]):
                    first_col = int(cols[0]) if promise and consecutive else -1
                    uni = uniform if promise else 0
                    row0, tail = (int(rng.integers(0, 9)), 2) if promise else (0, 0)
                    h_out, h_st, d_out, d_st, around = decode_both(eng, data, row_bytes, rib, flip, n_fam, cols, ploidies, first_col, uni,
                                                                   row0, tail)  # fmt: skip
                    where = (n_fam, name, len(rib), kind, promise)
                    assert np.array_equal(d_out, h_out), where
                    assert np.array_equal(d_st, h_st), where
                    assert (around == 77).all(), where  # nothing outside the call's rows is written
                    assert not (h_st == _ffi_plink.SAI_PLINK_STATUS_BAD_INDEX).any()
                    if kind in ("two", "one-clean"):
                        assert not h_st.any()
                        seen_clean += 1
                    elif h_st.any():
                        seen_flag += 1
                        r = int(np.flatnonzero(h_st)[0])  # the flag names the lowest heterozygous ploidy-1 slot of the row
                        s = len(cols) - int(h_st[r])
                        code = lambda c: (int(data[int(rib[r]) * row_bytes + c // 4]) >> (2 * (c % 4))) & 3  # noqa: E731
                        assert ploidies[s] == 1 and code(int(cols[s])) == HET
                        assert not any(ploidies[t] == 1 and code(int(cols[t])) == HET for t in range(s))
    assert seen_clean and (seen_flag or n_fam == 1)


def test_kernel_restates_the_table_and_refuses_bad_indices(eng):
    """Independent of the host decoder: the four codes at both ploidies, kept and flipped; an index outside its
    range is flagged, written as 0 and never dereferenced."""
    from sai_amd import _ffi_plink

    table = {(2, 0): [2, -2, 1, 0], (2, 1): [0, 4, 1, 2], (1, 0): [1, -1, 0, 0], (1, 1): [0, 2, 0, 1]}  # by code 00, 01, 10, 11
    rows = np.array([0b11100100], dtype=np.uint8)  # samples 0..3 hold the codes 0, 1, 2, 3
    cols = np.arange(4, dtype=np.int32)
    for (ploidy, flipped), want in table.items():
        pl = np.full(4, ploidy, dtype=np.int32)
        for uniform in (0, ploidy):
            h_out, h_st, d_out, d_st, _ = decode_both(eng, rows, 1, np.zeros(1, np.int32), np.array([flipped], np.uint8), 4, cols, pl,
                                                      0 if uniform else -1, uniform)  # fmt: skip
            assert d_out.tolist() == [want] == h_out.tolist()
            assert d_st.tolist() == h_st.tolist() == [4 - 2 if ploidy == 1 else 0]
    bad = _ffi_plink.SAI_PLINK_STATUS_BAD_INDEX
    rows = np.full(6, 0xFF, dtype=np.uint8)
    h_out, h_st, d_out, d_st, _ = decode_both(eng, rows, 2, np.array([0, 3, -1, 2], np.int32), np.zeros(4, np.uint8), 7,
                                              np.array([0, 7, 6, -2], np.int32), np.array([2, 2, 3, 2], np.int32))  # fmt: skip
    assert h_st.tolist() == d_st.tolist() == [bad] * 4
    assert h_out.tolist() == d_out.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    h_out, h_st, d_out, d_st, _ = decode_both(eng, rows, 2, np.array([2, 5], np.int32), np.zeros(2, np.uint8), 7,
                                              np.arange(7, dtype=np.int32), np.full(7, 2, np.int32), 0, 2)  # fmt: skip
    assert h_st.tolist() == d_st.tolist() == [0, bad] and h_out.tolist() == d_out.tolist() == [[0] * 7, [0] * 7]
    rows = np.full(10, 0xFF, dtype=np.uint8)  # rows wide enough for the fast path
    h_out, h_st, d_out, d_st, _ = decode_both(eng, rows, 5, np.array([1, 2], np.int32), np.ones(2, np.uint8), 20,
                                              np.arange(20, dtype=np.int32), np.full(20, 2, np.int32), 0, 2)  # fmt: skip
    assert h_st.tolist() == d_st.tolist() == [0, bad] and h_out.tolist() == d_out.tolist() == [[2] * 20, [0] * 20]


def test_streaming_reader_equals_host_reader(eng, tmp_path, monkeypatch):
    from sai_amd.utils import plink

    for seed in (3, 4, 11):
        case = random_case(seed, tmp_path)
        names, ploidies = [s for s, _ in case["request"]], [p for _, p in case["request"]]
        here = case["positions"]
        row_bytes = (len(case["samples"]) + 3) // 4
        for anc in (None, case["anc"]):
            for chrom, start, end in [("7", None, None), ("7", here[2], here[-2]), ("absent", None, None), ("7", here[-1] + 1, None)]:
                want = plink.load_dosage(case["prefix"], chrom, names, ploidies, start, end, anc)
                if chrom == "absent":
                    assert want[0].size == 0 and want[2] == 0
                for cap in (3 * row_bytes + 1, 4096, None):  # three rows per batch, a few KiB, one batch
                    if cap == 4096:
                        monkeypatch.setenv("SAI_AMD_INGEST_BUFFER", "4096")
                        got = plink.load_dosage_device(eng, case["prefix"] + ".bed", chrom, names, ploidies, start, end, anc)
                        monkeypatch.delenv("SAI_AMD_INGEST_BUFFER")
                    else:
                        got = plink.load_dosage_device(eng, case["prefix"], chrom, names, ploidies, start, end, anc, buffer_bytes=cap)
                    assert got[0].dtype == np.int32 and got[0].tolist() == want[0].tolist() and got[2:] == want[2:]
                    assert tuple(got[1].shape) == want[1].shape and np.array_equal(got[1].cpu().numpy(), want[1])
    # a wide fileset: many batches of several rows, the consecutive-run fast path and a gather
    rng = np.random.default_rng(8)
    samples = [f"w{i}" for i in range(2002)]
    n = 3000
    codes = rng.integers(0, 4, size=(n, 2002)).astype(np.uint8)
    prefix = str(tmp_path / "wide")
    write_fileset(prefix, ["5"] * n, np.cumsum(rng.integers(1, 30, n)).tolist(), [f"v{k}" for k in range(n)], ["A"] * n, ["C"] * n, codes, samples)
    for pick in (samples[100:1900], [samples[i] for i in rng.permutation(2002)[:300]], samples[7:9]):
        want = plink.load_dosage(prefix, "5", pick, [2] * len(pick))
        for cap in (40000, None):
            got = plink.load_dosage_device(eng, prefix, "5", pick, [2] * len(pick), buffer_bytes=cap)
            assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1].cpu().numpy(), want[1])
    with pytest.raises(ValueError, match=r"heterozygous call of sample w\d at variant v\d+ .*configured with ploidy 1"):
        plink.load_dosage_device(eng, prefix, "5", samples[:10], [1] * 10, buffer_bytes=40000)
    with pytest.raises(ValueError, match=r"SAI_AMD_INGEST_BUFFER of 500 bytes is smaller than one row of .*wide.bed \(501 bytes\)"):
        plink.load_dosage_device(eng, prefix, "5", samples[:10], [2] * 10, buffer_bytes=500)


def score_files(source, chrom, cfgfile, anc, out, win=(20000, 10000), num_workers=1):
    from sai_amd.sai import score

    score(vcf_file=source, chr_name=chrom, win_len=win[0], win_step=win[1], anc_allele_file=anc, output_file=str(out), config=cfgfile,
          num_workers=num_workers)  # fmt: skip
    return {p.name[len(out.stem) :]: p.read_bytes() for p in out.parent.glob(out.stem + "*")}


SCORE_CASES = [("tests/data/example.vcf", "21", "tests/data/test_sai.config.yaml", None), *FIXTURES]


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", SCORE_CASES)
def test_score_on_a_fileset_writes_the_files_of_the_vcf(eng, in_repo_root, tmp_path, monkeypatch, vcf, chrom, cfgfile, anc):
    prefix = str(tmp_path / "fx")
    fileset_from_vcf(vcf, prefix)
    for mode in ("device", "host"):
        monkeypatch.setenv("SAI_AMD_INGEST", mode)
        want = score_files(vcf, chrom, cfgfile, anc, tmp_path / f"vcf_{mode}" / "s.tsv")
        for source in (prefix + ".bed", prefix):
            got = score_files(source, chrom, cfgfile, anc, tmp_path / f"set_{mode}_{len(source)}" / "s.tsv")
            assert got == want and len(want[".tsv"].splitlines()) > 1, (mode, source)


def seeded_block(tmp_path):
    """20 000 sites x (60 + 60 + 2) diploids with 1 % missing calls, as VCF and as fileset, and a U + Q + DD
    configuration over it."""
    rng = np.random.default_rng(20260)
    n, sizes = 20000, (60, 60, 2)
    p = rng.random(n) ** 3
    ref = rng.binomial(2, p[:, None] * 0.2, size=(n, sizes[0]))
    tgt = rng.binomial(2, np.clip(p[:, None] * 2, 0, 1), size=(n, sizes[1]))
    src = np.repeat(np.where(rng.random((n, 1)) < 0.5, 2, 0), sizes[2], axis=1)
    dosage = np.concatenate([ref, tgt, src], axis=1)
    codes = np.array([HOM_A2, HET, HOM_A1], dtype=np.uint8)[dosage]
    codes[rng.random(codes.shape) < 0.01] = MISSING
    samples = [f"r{i}" for i in range(sizes[0])] + [f"t{i}" for i in range(sizes[1])] + [f"n{i}" for i in range(sizes[2])]
    positions = np.cumsum(rng.integers(1, 50, n)).tolist()
    kw = dict(chroms=["4"] * n, positions=positions, ids=[f"v{k}" for k in range(n)], a1=["T"] * n, a2=["G"] * n, codes=codes, samples=samples)
    prefix = str(tmp_path / "block")
    write_fileset(prefix, **kw)
    vcf = write_vcf(tmp_path / "block.vcf", **kw)
    for group, pop, members in (("ref", "R", samples[:60]), ("tgt", "T", samples[60:120]), ("src", "S", samples[120:])):
        (tmp_path / f"{group}.list").write_text("".join(f"{pop}\t{s}\n" for s in members))
    uq = "    ref:\n      R: 0.3\n    tgt:\n      T: {x}\n    src:\n      S: \"=1\"\n"
    cfg = tmp_path / "block.yaml"
    cfg.write_text("statistics:\n  U:\n" + uq.format(x=0.2) + "  Q:\n" + uq.format(x=0.95) + "  DD: true\n"
                   "ploidies:\n  ref:\n    R: 2\n  tgt:\n    T: 2\n  src:\n    S: 2\n"
                   f"populations:\n  ref: \"{tmp_path}/ref.list\"\n  tgt: \"{tmp_path}/tgt.list\"\n  src: \"{tmp_path}/src.list\"\n")  # fmt: skip
    return vcf, prefix, str(cfg)


def test_score_on_a_seeded_block_one_chunk_three_chunks_and_two_ranks(eng, in_repo_root, tmp_path, monkeypatch):
    vcf, prefix, cfg = seeded_block(tmp_path)
    win = (5000, 2500)
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES", raising=False)
    want = score_files(vcf, "4", cfg, None, tmp_path / "vcf" / "s.tsv", win)
    assert set(want) == {".tsv", ".U.log", ".Q.log"} and len(want[".tsv"].splitlines()) > 150
    assert len(want[".U.log"].splitlines()) > 1 and len(want[".Q.log"].splitlines()) > 1
    assert score_files(prefix + ".bed", "4", cfg, None, tmp_path / "one" / "s.tsv", win) == want
    from sai_amd import sai as sai_mod

    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "900000")  # the .bed is 620 003 bytes: 2.48 MB resident, three chunks
    assert sai_mod.chunks_for_memory(prefix + ".bed") == 3
    assert score_files(prefix + ".bed", "4", cfg, None, tmp_path / "three" / "s.tsv", win) == want
    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    assert score_files(prefix, "4", cfg, None, tmp_path / "three_host" / "s.tsv", win) == want
    monkeypatch.delenv("SAI_AMD_INGEST")
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES")
    # two ranks on this box's one GPU, gloo for the gather; started by `score` itself as a child job
    out = tmp_path / "two" / "s.tsv"
    code = ("import sai_amd.stats; from sai_amd.sai import score; "
            f"score(vcf_file={prefix + '.bed'!r}, chr_name='4', win_len={win[0]}, win_step={win[1]}, anc_allele_file=None, "
            f"output_file={str(out)!r}, config={cfg!r}, num_workers=2)")  # fmt: skip
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SAI_AMD_DIST_BACKEND="gloo")
    res = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert {p.name[1:]: p.read_bytes() for p in out.parent.glob("s*")} == want
