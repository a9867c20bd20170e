"""A VCF's calls written as a PLINK 1 fileset, on the GPU: the kernel ``sai_bed_encode`` against its host twin byte
for byte, ``convert`` on the GPU route against the host route, and ``score`` on the converted fileset against
``score`` on the VCF (byte-identical files, from both layouts).

The kernel's grid is not capped -- a lane takes one 32-bit word of the rows and a call of 4 GiB is refused -- so
there is no grid-stride loop to run past; the refusal is tested instead."""

import ctypes as C

import numpy as np
import pytest

from test_bed_export_cpu import UNFIT, WIDTHS, fileset_bytes, mixed_case, numpy_encode, ploidy_cases, random_block
from test_plink_cpu import FIXTURES, HOM_A1, HOM_A2, MISSING, write_vcf

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes behind the rows that must stay as they were


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


def encode_device(eng, dosage, ploidies):
    """One ``sai_bed_encode`` call -> (rows, status); the bytes behind the rows are checked here."""
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import bed_writer

    lib = bed_writer.load()
    n_rows, n_slots = dosage.shape
    row_bytes = (n_slots + 3) // 4
    uniform, per_slot = bed_writer._ploidy_arguments(ploidies)
    d_in = torch.from_numpy(np.ascontiguousarray(dosage)).to(eng.device)
    d_pl = None if per_slot is None else torch.from_numpy(per_slot).to(eng.device)
    d_out = torch.full((n_rows * row_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_st = torch.full((n_rows + 2,), -5, dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_bed_encode(eng.ctx, eng._ptr(d_in), n_rows, n_slots, eng._ptr(d_pl), uniform, eng._ptr(d_out), eng._ptr(d_st),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
    torch.cuda.synchronize()
    out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
    assert (out[n_rows * row_bytes :] == 0xA5).all() and (st[n_rows:] == -5).all()
    return out[: n_rows * row_bytes].reshape(n_rows, row_bytes), st[:n_rows]


def plant_unfit(rng, dosage, ploidies):
    """Values outside the table in about one row of three: at the first, a middle and the last slot."""
    n_rows, n_slots = dosage.shape
    pl = np.broadcast_to(np.asarray(ploidies), (n_slots,))
    for r in range(0, n_rows, 3):
        for where in {0, n_slots // 2, n_slots - 1} if r % 2 else {int(rng.integers(n_slots))}:
            choices = [v for v, p in UNFIT if p == pl[where]]
            dosage[r, where] = choices[int(rng.integers(len(choices)))]
    return dosage


@pytest.mark.parametrize("n_slots", WIDTHS + [2002])
def test_kernel_equals_host_twin(eng, n_slots):
    from sai_amd.utils.bed_writer import encode_host

    rng = np.random.default_rng(4000 + n_slots)
    for n_rows in (1, 7, 65):
        for name, ploidies in ploidy_cases(rng, n_slots):
            for flagged in (False, True):
                dosage = random_block(rng, n_rows, n_slots, ploidies)
                if flagged:
                    plant_unfit(rng, dosage, ploidies)
                want_rows, want_status = encode_host(dosage, ploidies)
                rows, status = encode_device(eng, dosage, ploidies)
                assert np.array_equal(rows, want_rows) and status.tolist() == want_status.tolist(), (n_rows, name, flagged)
                assert bool(want_status.any()) == flagged
                if n_rows == 7:  # the twin is pinned to the numpy statement on the host; once more here
                    assert np.array_equal(rows, numpy_encode(dosage, ploidies)[0])


@pytest.mark.parametrize("n_slots", [83, 2003])
def test_rows_that_start_at_every_residue(eng, n_slots):
    """An odd width: row r starts at byte r * n_slots of the block, every residue mod 16 within 16 rows, and the words
    of the rows start at every residue mod 4 of them."""
    from sai_amd.utils.bed_writer import encode_host

    rng = np.random.default_rng(n_slots)
    n_rows = 35
    assert {r * n_slots % 16 for r in range(n_rows)} == set(range(16)) and {r * ((n_slots + 3) // 4) % 4 for r in range(n_rows)} == set(range(4))
    for ploidies in (2, 1):
        dosage = plant_unfit(rng, random_block(rng, n_rows, n_slots, ploidies), ploidies)
        want_rows, want_status = encode_host(dosage, ploidies)
        rows, status = encode_device(eng, dosage, ploidies)
        assert np.array_equal(rows, want_rows) and status.tolist() == want_status.tolist() and want_status.any()


def test_a_ploidy_outside_its_range_on_the_word_path(eng):
    """Rows of nine bytes, per-slot ploidies, one of them 7: the field is 01 and every row says so, as the twin does."""
    from sai_amd.utils.bed_writer import encode_host

    rng = np.random.default_rng(33)
    ploidies = rng.integers(1, 3, 33).astype(np.int32)
    for where in (0, 17, 32):
        pl = ploidies.copy()
        pl[where] = 7
        dosage = plant_unfit(rng, random_block(rng, 9, 33, ploidies), ploidies)
        want_rows, want_status = encode_host(dosage, pl)
        rows, status = encode_device(eng, dosage, pl)
        assert np.array_equal(rows, want_rows) and status.tolist() == want_status.tolist() == [0x7FFFFFFF] * 9
        assert ((rows[:, where // 4] >> (2 * (where % 4))) & 3 == 0b01).all()


def test_every_byte_value_at_every_lane_position(eng):
    """All 256 values of a byte at both ploidies, at each of the 16 positions of a lane's load."""
    from sai_amd.utils.bed_writer import encode_host

    values = np.arange(256, dtype=np.uint8).view(np.int8)
    for ploidy in (2, 1):
        dosage = np.zeros((256 * 16, 32), dtype=np.int8)
        for k in range(16):
            dosage[k * 256 : (k + 1) * 256, k] = values
            dosage[k * 256 : (k + 1) * 256, 16 + (k * 7) % 16] = values[::-1]
        want_rows, want_status = encode_host(dosage, ploidy)
        rows, status = encode_device(eng, dosage, ploidy)
        assert np.array_equal(rows, want_rows) and status.tolist() == want_status.tolist()
        assert np.array_equal(rows, numpy_encode(dosage, ploidy)[0])


@pytest.mark.parametrize("n_slots", [5, 64, 2002])
def test_round_trip_through_the_device_decoder(eng, n_slots):
    import torch

    from sai_amd import _ffi, _ffi_plink

    lib = _ffi_plink.load()
    rng = np.random.default_rng(n_slots)
    n_rows, row_bytes = 65, (n_slots + 3) // 4
    for name, ploidies in ploidy_cases(rng, n_slots):
        pl = np.broadcast_to(np.asarray(ploidies, dtype=np.int32), (n_slots,)).copy()
        codes = rng.integers(0, 4, size=(n_rows, n_slots)).astype(np.uint8)
        codes[:, pl == 1] = rng.choice(np.array([HOM_A1, MISSING, HOM_A2], dtype=np.uint8), size=(n_rows, int((pl == 1).sum())))
        padded = np.zeros((n_rows, row_bytes * 4), dtype=np.uint8)
        padded[:, :n_slots] = codes
        quads = padded.reshape(n_rows, -1, 4)
        bed = np.ascontiguousarray(quads[:, :, 0] | quads[:, :, 1] << 2 | quads[:, :, 2] << 4 | quads[:, :, 3] << 6, dtype=np.uint8)
        dev = lambda a: torch.from_numpy(a).to(eng.device)  # noqa: E731
        d_bed, d_rib, d_flip, d_pl = dev(bed), dev(np.arange(n_rows, dtype=np.int32)), dev(np.zeros(n_rows, dtype=np.uint8)), dev(pl)
        d_out = torch.empty((n_rows, n_slots), dtype=torch.int8, device=eng.device)
        d_st = torch.empty((n_rows,), dtype=torch.int32, device=eng.device)
        _ffi.check(lib.sai_plink_decode(eng.ctx, eng._ptr(d_bed), n_rows, row_bytes, n_rows, eng._ptr(d_rib), eng._ptr(d_flip), n_slots, n_slots,
                                        None, 0, eng._ptr(d_pl), 0, C.c_void_p(d_out.data_ptr()), 0, eng._ptr(d_st),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
        torch.cuda.synchronize()
        assert not d_st.any()
        back, status = encode_device(eng, d_out.cpu().numpy(), ploidies)
        assert not status.any() and np.array_equal(back, bed), name


def test_argument_errors(eng):
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import bed_writer

    lib = bed_writer.load()
    d_in = torch.zeros((64,), dtype=torch.int8, device=eng.device)
    d_out = torch.full((64,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_st = torch.full((4,), -5, dtype=torch.int32, device=eng.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    refused = [
        ((None, ptr(d_in), 2, 5, None, 2, ptr(d_out), ptr(d_st)), b"ctx is NULL"),
        ((eng.ctx, None, 2, 5, None, 2, ptr(d_out), ptr(d_st)), b"NULL buffer"),
        ((eng.ctx, ptr(d_in), 2, 5, None, 2, None, ptr(d_st)), b"NULL buffer"),
        ((eng.ctx, ptr(d_in), 2, 5, None, 2, ptr(d_out), None), b"NULL buffer"),
        ((eng.ctx, ptr(d_in), 2, 5, None, 0, ptr(d_out), ptr(d_st)), b"NULL buffer"),
        ((eng.ctx, ptr(d_in), -1, 5, None, 2, ptr(d_out), ptr(d_st)), b"size out of range"),
        ((eng.ctx, ptr(d_in), 2, 0, None, 2, ptr(d_out), ptr(d_st)), b"size out of range"),
        ((eng.ctx, ptr(d_in), 2, 5, None, 3, ptr(d_out), ptr(d_st)), b"uniform_ploidy must be 0, 1 or 2"),
        ((eng.ctx, ptr(d_in, 1), 2, 5, None, 2, ptr(d_out), ptr(d_st)), b"dosage must be 16-byte aligned"),
        ((eng.ctx, ptr(d_in), 2, 5, None, 2, ptr(d_out, 4), ptr(d_st)), b"out must be 16-byte aligned"),
        # 4 GiB of rows in one call: refused before anything is touched (the grid is not capped, a word per lane)
        ((eng.ctx, ptr(d_in), (1 << 32) // 501 + 1, 2002, None, 2, ptr(d_out), ptr(d_st)), b"a call writes less than 4 GiB of rows"),
    ]
    for args, message in refused:
        assert lib.sai_bed_encode(*args, stream) == _ffi.SAI_ERR_ARG and message in lib.sai_last_error(), message
    assert lib.sai_bed_encode(eng.ctx, None, 0, 5, None, 2, None, None, stream) == 0  # no row: fine, nothing touched
    torch.cuda.synchronize()
    assert (d_out == 0xA5).all() and (d_st == -5).all()
    d_pl = torch.tensor([2, 2, 2, 7, 2], dtype=torch.int32, device=eng.device)  # a ploidy outside 1 .. 2: the rows' status
    _ffi.check(lib.sai_bed_encode(eng.ctx, ptr(d_in), 2, 5, ptr(d_pl), 0, ptr(d_out), ptr(d_st), stream))
    torch.cuda.synchronize()
    assert d_st.tolist() == [0x7FFFFFFF, 0x7FFFFFFF, -5, -5] and d_out[:5].tolist() == [0b01111111, 0b11, 0b01111111, 0b11, 0xA5]


# ---- convert on the GPU route ----


def convert_both(monkeypatch, tmp_path, vcf, chrom, **kw):
    """The fileset written on the GPU route and on the host route -> (prefix, prefix)."""
    from sai_amd.sai import convert

    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    host = convert(vcf, chrom, str(tmp_path / "host"), **kw)
    monkeypatch.delenv("SAI_AMD_INGEST")
    device = convert(vcf, chrom, str(tmp_path / "device"), **kw)
    assert {k: v for k, v in host.items() if k != "ms"} == {k: v for k, v in device.items() if k != "ms"}
    assert device["ms"]["encode"] > 0 and device["ms"]["d2h"] > 0 and host["ms"]["d2h"] == 0
    return str(tmp_path / "device"), str(tmp_path / "host")


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", FIXTURES)
def test_convert_on_the_gpu_writes_the_files_of_the_host_route(eng, in_repo_root, tmp_path, monkeypatch, vcf, chrom, cfgfile, anc):
    device, host = convert_both(monkeypatch, tmp_path, vcf, chrom)
    assert fileset_bytes(device) == fileset_bytes(host)


def test_convert_on_the_gpu_in_many_batches_at_mixed_ploidies(eng, in_repo_root, tmp_path, monkeypatch):
    """13 samples, 100 rows, 16 rows per batch: both pinned buffers go round several times; then a refusal, which
    leaves nothing behind, and an append."""
    from sai_amd.sai import convert

    case = mixed_case(tmp_path)
    monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", "64")
    device, host = convert_both(monkeypatch, tmp_path, case["vcf"], "7", haploid_samples=case["haploid"])
    assert fileset_bytes(device) == fileset_bytes(host)
    before = sorted(p.name for p in tmp_path.iterdir())
    with pytest.raises(ValueError, match=r"mixed.vcf: the call of sample s\d+ at position \d+ has dosage -1 at ploidy 2"):
        convert(case["vcf"], "7", str(tmp_path / "refused"))
    kept = fileset_bytes(device)
    with pytest.raises(ValueError, match=r"has dosage -1 at ploidy 2"):
        convert(case["vcf"], "8", device, append=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == before and fileset_bytes(device) == kept
    cut = case["positions"][37]
    convert(case["vcf"], "7", str(tmp_path / "parts"), haploid_samples=case["haploid"], end=cut)
    convert(case["vcf"], "7", str(tmp_path / "parts"), haploid_samples=case["haploid"], start=cut + 1, append=True)
    assert fileset_bytes(str(tmp_path / "parts")) == kept


# ---- score on the converted fileset ----


def score_files(source, chrom, cfgfile, anc, out, layout=None, win=(20000, 10000)):
    from sai_amd.sai import score

    score(vcf_file=source, chr_name=chrom, win_len=win[0], win_step=win[1], anc_allele_file=anc, output_file=str(out), config=cfgfile,
          num_workers=1, layout=layout)  # fmt: skip
    return {p.name[len(out.stem) :]: p.read_bytes() for p in out.parent.glob(out.stem + "*")}


SCORE_CASES = [("tests/data/example.vcf", "21", "tests/data/test_sai.config.yaml", None), *FIXTURES]


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", SCORE_CASES)
def test_score_on_the_converted_fileset_writes_the_files_of_the_vcf(eng, in_repo_root, tmp_path, monkeypatch, vcf, chrom, cfgfile, anc):
    from sai_amd.sai import convert

    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    prefix = str(tmp_path / "fx")
    convert(vcf, chrom, prefix)
    want = score_files(vcf, chrom, cfgfile, anc, tmp_path / "vcf" / "s.tsv")
    assert score_files(prefix + ".bed", chrom, cfgfile, anc, tmp_path / "set" / "s.tsv") == want and len(want[".tsv"].splitlines()) > 1
    # the 2-bit layout, which no VCF is admitted to: example.vcf, and the outgroup fixture, which the existing packed2 tests score
    if vcf.endswith(("example.vcf", "test.with.outgroup.vcf.gz")):
        assert score_files(prefix, chrom, cfgfile, anc, tmp_path / "packed2" / "s.tsv", layout="packed2") == want
    if vcf.endswith("example.vcf"):
        with pytest.raises(ValueError):
            score_files(vcf, chrom, cfgfile, None, tmp_path / "refused" / "s.tsv", layout="packed2")


def test_score_on_the_converted_outgroup_fileset_in_the_packed_layout(eng, in_repo_root, tmp_path, monkeypatch):
    """The fixture the existing packed2 tests score (tests/test_packed_stats_device.py): flipped rows and an outgroup.
    Converted by ``convert`` and scored in the 2-bit layout with its ancestral alleles, it gives the reference's own
    expected table byte for byte, which is also what the VCF and the int8 layout give at these windows."""
    from sai_amd.sai import convert, score

    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    vcf, chrom, cfgfile, anc = FIXTURES[2]
    assert vcf.endswith("test.with.outgroup.vcf.gz") and anc is not None
    prefix = str(tmp_path / "og")
    assert convert(vcf, chrom, prefix)["rows_written"] == 373
    want = open("tests/data/test.with.outgroup.res.tsv", "rb").read()
    for label, source, layout in (("vcf", vcf, None), ("int8", prefix + ".bed", "int8"), ("packed2", prefix + ".bed", "packed2"), ("bare", prefix, "packed2")):
        out = tmp_path / label / "og.tsv"
        score(vcf_file=source, chr_name=chrom, win_len=40000, win_step=40000, anc_allele_file=anc, output_file=str(out), config=cfgfile,
              num_workers=1, layout=layout)  # fmt: skip
        assert out.read_bytes() == want, label
        assert sorted(p.name for p in out.parent.iterdir()) == ["og.tsv"]  # no U / Q: no logs


def test_score_on_a_converted_fileset_of_mixed_ploidies(eng, in_repo_root, tmp_path, monkeypatch):
    """Diploid ref and tgt, a haploid src: 3 000 sites written with --haploid, scored with the configuration's ploidies
    from the VCF, from the fileset and from the fileset in the 2-bit layout."""
    from sai_amd.sai import convert

    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    rng = np.random.default_rng(77)
    n, sizes = 3000, (21, 19, 2)
    p = rng.random(n) ** 3
    dosage = np.concatenate([rng.binomial(2, p[:, None] * 0.2, size=(n, sizes[0])), rng.binomial(2, np.clip(p[:, None] * 2, 0, 1), size=(n, sizes[1])),
                             np.repeat(np.where(rng.random((n, 1)) < 0.5, 2, 0), sizes[2], axis=1)], axis=1)  # fmt: skip
    codes = np.array([HOM_A2, 2, HOM_A1], dtype=np.uint8)[dosage]
    codes[rng.random(codes.shape) < 0.01] = MISSING
    samples = [f"r{i}" for i in range(sizes[0])] + [f"t{i}" for i in range(sizes[1])] + [f"n{i}" for i in range(sizes[2])]
    src = samples[sizes[0] + sizes[1] :]
    positions = np.cumsum(rng.integers(1, 50, n)).tolist()
    vcf = write_vcf(tmp_path / "block.vcf", ["4"] * n, positions, [f"v{k}" for k in range(n)], ["T"] * n, ["G"] * n, codes, samples, haploid=src)
    for group, pop, members in (("ref", "R", samples[: sizes[0]]), ("tgt", "T", samples[sizes[0] : sizes[0] + sizes[1]]), ("src", "S", src)):
        (tmp_path / f"{group}.list").write_text("".join(f"{pop}\t{s}\n" for s in members))
    uq = "    ref:\n      R: 0.3\n    tgt:\n      T: {x}\n    src:\n      S: \"=1\"\n"
    cfg = tmp_path / "block.yaml"
    cfg.write_text("statistics:\n  U:\n" + uq.format(x=0.2) + "  Q:\n" + uq.format(x=0.95) +
                   "ploidies:\n  ref:\n    R: 2\n  tgt:\n    T: 2\n  src:\n    S: 1\n"
                   f"populations:\n  ref: \"{tmp_path}/ref.list\"\n  tgt: \"{tmp_path}/tgt.list\"\n  src: \"{tmp_path}/src.list\"\n")  # fmt: skip
    prefix = str(tmp_path / "block")
    assert convert(vcf, "4", prefix, haploid_samples=src)["rows_written"] == n
    win = (5000, 2500)
    want = score_files(vcf, "4", str(cfg), None, tmp_path / "vcf" / "s.tsv", win=win)
    assert len(want[".tsv"].splitlines()) > 20
    assert score_files(prefix + ".bed", "4", str(cfg), None, tmp_path / "set" / "s.tsv", win=win) == want
    assert score_files(prefix, "4", str(cfg), None, tmp_path / "packed2" / "s.tsv", layout="packed2", win=win) == want
