"""A VCF's calls written as a PLINK 2 fileset, on the GPU: the kernels of ``sai_pgen_encode`` against their host twin
on every case of ``pgen_export_cases`` (record types, lengths, status values and record bytes identical, nothing
written outside the batch's bytes), past the grid cap, ``convert`` on the GPU route against the host route, the
written records through ``sai_pgen_decode``, and ``score`` on the converted fileset against ``score`` on the VCF."""

import ctypes as C

import numpy as np
import pytest

import pgen_export_cases as PC
from test_bed_export_cpu import mixed_case
from test_pgen_export_cpu import fileset_bytes
from test_plink_cpu import FIXTURES

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes before and behind the records, elements behind every table, that must stay as they were


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


def encode_device(eng, block, ploidies):
    """One ``sai_pgen_encode`` call -> (records, vrtype, length, status); what lies around the outputs is checked here."""
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import bed_writer, pgen_writer

    lib = pgen_writer.load()
    n_rows, n_slots = block.shape
    cap = n_rows * ((n_slots + 3) // 4)
    uniform, per_slot = bed_writer._ploidy_arguments(ploidies)
    d_in = torch.from_numpy(np.ascontiguousarray(block)).to(eng.device)
    d_pl = None if per_slot is None else torch.from_numpy(per_slot).to(eng.device)
    d_out = torch.full((GUARD + cap + GUARD,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_vt = torch.full((n_rows + GUARD,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_len = torch.full((n_rows + GUARD,), -5, dtype=torch.int32, device=eng.device)
    d_off = torch.full((n_rows + 1 + GUARD,), -5, dtype=torch.int32, device=eng.device)
    d_st = torch.full((n_rows + GUARD,), -5, dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_pgen_encode(eng.ctx, eng._ptr(d_in), n_rows, n_slots, eng._ptr(d_pl), uniform, C.c_void_p(d_out.data_ptr() + GUARD), eng._ptr(d_vt),
                                   eng._ptr(d_len), eng._ptr(d_off), eng._ptr(d_st), pgen_writer.ENCODE_ALL, C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
    torch.cuda.synchronize()
    out, vt, ln, off, st = (t.cpu().numpy() for t in (d_out, d_vt, d_len, d_off, d_st))
    ln, off = ln.view(np.uint32), off.view(np.uint32)
    total = int(off[n_rows])
    assert (vt[n_rows:] == 0xA5).all() and (ln[n_rows:] == 0xFFFFFFFB).all() and (off[n_rows + 1 :] == 0xFFFFFFFB).all() and (st[n_rows:] == -5).all()
    assert total == int(ln[:n_rows].sum(dtype=np.uint64)) <= cap and off[:n_rows].tolist() == (np.cumsum(ln[:n_rows], dtype=np.uint64) - ln[:n_rows]).tolist()
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + total :] == 0xA5).all()  # nothing before the records, nothing behind them
    return out[GUARD : GUARD + total], vt[:n_rows], ln[:n_rows], st[:n_rows]


def same_as_host(eng, block, ploidies, name):
    from sai_amd.utils import pgen_writer

    want = pgen_writer.encode_host(block, ploidies)
    got = encode_device(eng, block, ploidies)
    for label, a, b in zip(("vrtype", "length", "status", "records"), (got[1], got[2], got[3], got[0]), (want[1], want[2], want[3], want[0])):
        assert np.array_equal(a, b), (name, label)
    return want


@pytest.mark.parametrize("case", PC.CASES, ids=PC.CASE_IDS)
def test_kernels_equal_host_twin(eng, case):
    out, vrtype, length, status = same_as_host(eng, case.block, case.ploidies, case.name)
    assert not status.any()
    if case.codes.shape[0] <= 17:  # the twin is pinned to the test writer on the host; once more here
        types, records = PC.reference(case)
        assert vrtype.tolist() == types and out.tobytes() == b"".join(records)


def test_kernels_flag_what_the_host_twin_flags(eng):
    seen = 0
    for name, block, ploidies, _, want_status in PC.unfit_cases():
        status = same_as_host(eng, block, ploidies, name)[3]
        assert status.tolist() == want_status, name
        seen += 1
    assert seen > 200


def test_every_byte_value_at_every_lane_position(eng):
    """All 256 values of a byte at both ploidies and with per-slot ploidies, at each of the 16 positions of a lane's
    word, beside neighbours of every fitting value: a recoding that leaks from one byte into the next shows here."""
    values = np.arange(256, dtype=np.uint8).view(np.int8)
    mixed = np.array([1, 2] * 16, dtype=np.int32)
    for ploidies in (2, 1, mixed):
        pl = np.broadcast_to(np.asarray(ploidies), (32,))
        fitting = np.where(pl == 2, 2, 1).astype(np.int8)
        for fill in (0, 1, -1):  # 0, the ALT homozygote, the missing call
            block = np.tile((fitting * fill if fill >= 0 else -fitting)[None, :], (256 * 16, 1)).astype(np.int8)
            for k in range(16):
                block[k * 256 : (k + 1) * 256, k] = values
                block[k * 256 : (k + 1) * 256, 16 + (k * 7) % 16] = values[::-1]
            status = same_as_host(eng, block, ploidies, f"fill {fill}")[3]
            assert status.any() and not status.all()


def test_rows_past_the_grid_cap(eng):
    """2 x cap + 3 rows of 5 samples: every workgroup of the plan and of the write kernel takes a third row."""
    from sai_amd.utils import pgen_writer

    cap = pgen_writer.load().sai_pgen_encode_grid_cap(eng.ctx)
    assert 0 < cap <= 1 << 16
    rng = np.random.default_rng(cap)
    codes = PC.random_rows(rng, 2 * cap + 3, 5)
    out, vrtype, length, status = same_as_host(eng, PC.block_of(codes, 2), 2, "grid cap")
    assert not status.any() and len(set(vrtype[2 * cap :].tolist()) | set(vrtype[:cap].tolist())) > 1


def test_rows_that_start_at_every_residue(eng):
    """An odd width: row r starts at byte r * 83 of the block, every residue mod 16 within 16 rows, and the records at
    every residue mod 4."""
    rng = np.random.default_rng(83)
    codes = PC.random_rows(rng, 67, 83)
    out, vrtype, length, _ = same_as_host(eng, PC.block_of(codes, 2), 2, "residues")
    starts = np.cumsum(length) - length
    assert {int(s) % 4 for s in starts} == {0, 1, 2, 3} and {int(s) % 4 for s, t in zip(starts, vrtype) if t == 0} == {0, 1, 2, 3}


@pytest.mark.parametrize("case", [c for c in PC.CASES if c.codes.shape[0] != 130], ids=[c.name for c in PC.CASES if c.codes.shape[0] != 130])
def test_round_trip_through_the_device_decoder(eng, case):
    import torch

    from sai_amd import _ffi, _ffi_pgen

    lib = _ffi_pgen.load()
    out, vrtype, length, _ = encode_device(eng, case.block, case.ploidies)
    n_rows, n = case.block.shape
    ends = np.cumsum(length, dtype=np.int64)
    rec = np.ascontiguousarray(np.stack([ends - length, length.astype(np.int64), vrtype.astype(np.int64)], axis=1))
    dev = lambda a: torch.from_numpy(a).to(eng.device)  # noqa: E731
    d_bytes, d_rec, d_base, d_flip = dev(np.ascontiguousarray(out)), dev(rec), dev(np.full((n_rows, 3), -1, dtype=np.int64)), dev(np.zeros(n_rows, dtype=np.uint8))
    d_pl = dev(np.array(np.broadcast_to(np.asarray(case.ploidies, dtype=np.int32), (n,))))
    d_out = torch.empty((n_rows, n), dtype=torch.int8, device=eng.device)
    d_st = torch.empty((n_rows,), dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_pgen_decode(eng.ctx, eng._ptr(d_bytes), out.size, n_rows, eng._ptr(d_rec), eng._ptr(d_base), eng._ptr(d_flip), n, n, None, 0,
                                   eng._ptr(d_pl), 0, C.c_void_p(d_out.data_ptr()), 0, eng._ptr(d_st), C.c_void_p(torch.cuda.current_stream().cuda_stream)))  # fmt: skip
    torch.cuda.synchronize()
    assert not d_st.any() and np.array_equal(d_out.cpu().numpy(), case.block)


def test_argument_errors(eng):
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import pgen_writer

    lib = pgen_writer.load()
    d_in = torch.zeros((64,), dtype=torch.int8, device=eng.device)
    d_out = torch.full((64,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_vt = torch.full((8,), 0xA5, dtype=torch.uint8, device=eng.device)
    d_len, d_off, d_st = (torch.full((8,), -5, dtype=torch.int32, device=eng.device) for _ in range(3))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    good = (eng.ctx, ptr(d_in), 2, 5, None, 2, ptr(d_out), ptr(d_vt), ptr(d_len), ptr(d_off), ptr(d_st), pgen_writer.ENCODE_ALL)
    refused = [
        ({0: None}, b"ctx is NULL"), ({1: None}, b"NULL buffer"), ({6: None}, b"NULL buffer"), ({7: None}, b"NULL buffer"), ({8: None}, b"NULL buffer"),
        ({9: None}, b"NULL buffer"), ({10: None}, b"NULL buffer"), ({5: 0}, b"NULL buffer"),
        ({2: -1}, b"size out of range"), ({3: 0}, b"size out of range: a .pgen record holds 1 to 2^31 - 1 samples"),
        ({5: 3}, b"uniform_ploidy must be 0, 1 or 2"), ({11: 0}, b"stages must be 1 .. 7"), ({11: 8}, b"stages must be 1 .. 7"), ({1: ptr(d_in, 1)}, b"dosage must be 16-byte aligned"),
        # 4 GiB of records in one call: refused before anything is touched
        ({2: (1 << 32) // 501 + 1, 3: 2002}, b"a call writes less than 4 GiB of records"),
    ]  # fmt: skip
    for change, message in refused:
        args = [change.get(k, v) for k, v in enumerate(good)]
        assert lib.sai_pgen_encode(*args, stream) == _ffi.SAI_ERR_ARG and message in lib.sai_last_error(), (change, message)
    torch.cuda.synchronize()
    assert (d_out == 0xA5).all() and (d_vt == 0xA5).all() and (d_len == -5).all() and (d_off == -5).all() and (d_st == -5).all()
    assert lib.sai_pgen_encode(eng.ctx, None, 0, 5, None, 2, None, None, None, ptr(d_off), None, 7, stream) == 0  # no row: the total is 0
    torch.cuda.synchronize()
    assert d_off.tolist() == [0] + [-5] * 7 and (d_out == 0xA5).all()
    d_pl = torch.tensor([2, 2, 2, 7, 2], dtype=torch.int32, device=eng.device)  # a ploidy outside 1 .. 2: the rows' status, the code 3
    args = [{4: ptr(d_pl), 5: 0}.get(k, v) for k, v in enumerate(good)]
    _ffi.check(lib.sai_pgen_encode(*args, stream))
    torch.cuda.synchronize()
    assert d_st.tolist()[:3] == [0x7FFFFFFF, 0x7FFFFFFF, -5] and d_out[:5].tolist() == [0b11000000, 0, 0b11000000, 0, 0xA5] and d_off.tolist()[:3] == [0, 2, 4]


# ---- convert on the GPU route ----


def convert_both(monkeypatch, tmp_path, vcf, chrom, tag="", **kw):
    """The fileset written on the GPU route and on the host route -> (prefix, prefix)."""
    from sai_amd.sai import convert

    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    host = convert(vcf, chrom, out_pfile=str(tmp_path / f"host{tag}"), **kw)
    monkeypatch.delenv("SAI_AMD_INGEST")
    device = convert(vcf, chrom, out_pfile=str(tmp_path / f"device{tag}"), **kw)
    assert {k: v for k, v in host.items() if k != "ms"} == {k: v for k, v in device.items() if k != "ms"}
    assert device["ms"]["encode"] > 0 and device["ms"]["d2h"] > 0 and host["ms"]["d2h"] == 0
    return str(tmp_path / f"device{tag}"), str(tmp_path / f"host{tag}")


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", FIXTURES)
def test_convert_on_the_gpu_writes_the_files_of_the_host_route(eng, in_repo_root, tmp_path, monkeypatch, vcf, chrom, cfgfile, anc):
    device, host = convert_both(monkeypatch, tmp_path, vcf, chrom)
    assert fileset_bytes(device) == fileset_bytes(host)
    monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", "64")  # 16 rows per batch: both pinned buffers go round many times
    small, _ = convert_both(monkeypatch, tmp_path, vcf, chrom, tag="_small")
    assert fileset_bytes(small) == fileset_bytes(host)


def test_convert_on_the_gpu_in_many_batches_at_mixed_ploidies(eng, in_repo_root, tmp_path, monkeypatch):
    from sai_amd.sai import convert

    case = mixed_case(tmp_path)
    monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", "64")
    device, host = convert_both(monkeypatch, tmp_path, case["vcf"], "7", haploid_samples=case["haploid"])
    assert fileset_bytes(device) == fileset_bytes(host)
    before = sorted(p.name for p in tmp_path.iterdir())
    with pytest.raises(ValueError, match=r"mixed.vcf: the call of sample s\d+ at position \d+ has dosage -1 at ploidy 2: a .pgen record holds"):
        convert(case["vcf"], "7", out_pfile=str(tmp_path / "refused"))
    assert sorted(p.name for p in tmp_path.iterdir()) == before


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
    convert(vcf, chrom, out_pfile=prefix)
    want = score_files(vcf, chrom, cfgfile, anc, tmp_path / "vcf" / "s.tsv")
    assert score_files(prefix + ".pgen", chrom, cfgfile, anc, tmp_path / "set" / "s.tsv") == want and len(want[".tsv"].splitlines()) > 1
    if vcf.endswith("example.vcf"):  # the 2-bit layout, without ancestral alleles
        assert anc is None and score_files(prefix, chrom, cfgfile, anc, tmp_path / "packed2" / "s.tsv", layout="packed2") == want


def test_score_on_the_converted_outgroup_fileset_in_the_packed_layout(eng, in_repo_root, tmp_path, monkeypatch):
    """The fixture the existing packed2 tests score: flipped rows and an outgroup.  Converted to a ``.pgen`` and scored
    in the 2-bit layout with its ancestral alleles, it gives the reference's own expected table byte for byte."""
    from sai_amd.sai import convert, score

    for name in ("SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "SAI_AMD_INGEST"):
        monkeypatch.delenv(name, raising=False)
    vcf, chrom, cfgfile, anc = FIXTURES[2]
    assert vcf.endswith("test.with.outgroup.vcf.gz") and anc is not None
    prefix = str(tmp_path / "og")
    assert convert(vcf, chrom, out_pfile=prefix)["rows_written"] == 373
    want = open("tests/data/test.with.outgroup.res.tsv", "rb").read()
    for label, source, layout in (("vcf", vcf, None), ("int8", prefix + ".pgen", "int8"), ("packed2", prefix + ".pgen", "packed2"), ("bare", prefix, "packed2")):
        out = tmp_path / label / "og.tsv"
        score(vcf_file=source, chr_name=chrom, win_len=40000, win_step=40000, anc_allele_file=anc, output_file=str(out), config=cfgfile,
              num_workers=1, layout=layout)  # fmt: skip
        assert out.read_bytes() == want, label
