"""A VCF's calls written as a PLINK 2 fileset, on the host: every case of ``pgen_export_cases`` proved to reach what it
is named for, the encoder ``sai_pgen_encode_host`` and the assembled file against the test writer ``pgen_builder`` byte
for byte, the encoder as a stand-alone program under the sanitizers, and ``convert(..., out_pfile=)`` under
``SAI_AMD_INGEST=host`` against the VCF reader on the same calls."""

import ctypes as C
import json

import numpy as np
import pytest

import native_build
import pgen_builder
import pgen_export_cases as PC
from test_bed_export_cpu import _write, listing, mixed_case
from test_plink_cpu import FIXTURES, regions_of, sai_cli


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def listed(row, kind):
    """The samples a record of ``kind`` lists."""
    if kind == 0:
        return np.array([], dtype=np.int64)
    if kind == 1:
        lo, hi = pgen_builder.onebit_pair(row)
        return np.flatnonzero((row != lo) & (row != hi))
    return np.flatnonzero(row != {4: 0, 6: 2, 7: 3}[kind])


def test_the_argmin_rule_is_the_builders_own_choice():
    """``types=None`` of the test writer picks among 0 .. 7; on a first row (no base: types 2 and 3 are out) it is the
    rule of ``reference``."""
    for case in PC.CASES[::9]:
        row = case.codes[:1]
        assert pgen_builder.build_pgen(row)[1][0][2] == PC.reference_of(("first", case.name), row)[0][0]


@pytest.mark.parametrize("case", PC.CASES, ids=PC.CASE_IDS)
def test_case_reaches_what_it_is_named_for(case):
    types, records = PC.reference(case)
    n, want = case.codes.shape[1], case.want
    assert all(len(r) <= -(-n // 4) for r in records)  # no record is longer than its dense form: LB is known beforehand
    if "types" in want:
        assert types == want["types"]
    if "w" in want:
        assert pgen_builder.index_width(n) == want["w"]
    entries = [listed(row, kind) for row, kind in zip(case.codes, types)]
    if "L" in want:
        assert [len(e) for e in entries] == [want["L"]] * len(types)
        if "G" in want:
            assert -(-want["L"] // 64) == want["G"] and (want["G"] <= 64) == (want["L"] <= 4096)
    if "varint_L" in want:
        assert all(len(pgen_builder.varint(len(e))) == want["varint_L"] for e in entries)
    if "delta_bytes" in want:
        widest = [max((len(pgen_builder.varint(int(d))) for d in np.diff(e)), default=0) for e in entries]
        # varint(3), one 3-byte index, one code byte, two 3-byte deltas
        assert widest[:2] == [want["delta_bytes"]] * 2 and records[0][0] == 3 and len(records[0]) == 1 + 3 + 1 + 2 * 3
    if "pairs" in want:
        assert [r[0] for r in records] == [4 * lo + (hi - lo) for lo, hi in want["pairs"]]
    if "tie_pair" in want:
        counts = sorted(np.bincount(case.codes[0], minlength=4).tolist(), reverse=True)
        assert pgen_builder.onebit_pair(case.codes[0]) == want["tie_pair"] and (counts[0] == counts[1] or counts[1] == counts[2])
    if case.family == "ploidies":
        pl = np.broadcast_to(np.asarray(case.ploidies), (n,))
        assert (pl == 1).any() and not (case.codes[:, pl == 1] == 1).any() and (case.block[:, pl == 1] == -1).any()


def test_the_families_together_reach_every_type_and_width():
    by_family = {}
    for case in PC.CASES:
        by_family.setdefault(case.family, set()).update(PC.reference(case)[0])
    assert by_family["widths"] == by_family["ploidies"] | {1} == set(PC.KINDS)
    widths = {c.codes.shape[1] for c in PC.CASES if c.family == "widths"}
    assert widths == set(PC.WIDTHS) and {c.codes.shape[0] for c in PC.CASES if c.family == "widths"} == set(PC.ROW_COUNTS)
    assert {pgen_builder.index_width(n) for n in (255, 256, 65535, 65536, 70000)} == {1, 2, 3}
    edge = [c for c in PC.CASES if c.name.startswith("the LDS tile edge")]
    assert [c.codes.shape[1] for c in edge] == [16383, 16384, 16385]


@pytest.mark.parametrize("case", PC.CASES, ids=PC.CASE_IDS)
def test_host_twin_and_assembled_file_equal_the_test_writer(case):
    from sai_amd.utils import pgen_writer

    types, records = PC.reference(case)
    out, vrtype, length, status = pgen_writer.encode_host(case.block, case.ploidies, n_threads=3)
    assert vrtype.tolist() == types and length.tolist() == [len(r) for r in records] and not status.any()
    assert out.tobytes() == b"".join(records)
    n = case.codes.shape[1]
    lb = pgen_writer.length_bytes(n)
    assert lb == max(1, -(-(-(-n // 4)).bit_length() // 8))
    data, table = pgen_builder.build_pgen(case.codes, types=types, len_bytes=lb)
    head = pgen_writer.assemble_header(n, vrtype, length)
    assert len(head) == pgen_writer.header_len(len(types), n) == table[0][0] and head + out.tobytes() == data
    assert data[2] == 0x10 and data[11] == lb - 1


def test_header_of_more_than_one_block():
    """65 536 + 3 variants of one sample: two blocks, the second offset behind the first block's records."""
    from sai_amd.utils import pgen_writer

    codes = (np.arange(65539) % 4).astype(np.uint8)[:, None]
    out, vrtype, length, status = pgen_writer.encode_host(PC.block_of(codes, 2), 2)
    assert vrtype.tolist() == [0] * 65539 and length.tolist() == [1] * 65539
    data, _ = pgen_builder.build_pgen(codes, types=[0] * 65539, len_bytes=1)
    assert pgen_writer.assemble_header(1, vrtype, length) + out.tobytes() == data


def test_status_of_values_that_do_not_fit_and_of_bad_ploidies():
    from sai_amd.utils import pgen_writer

    seen = 0
    for name, block, ploidies, codes, want_status in PC.unfit_cases():
        out, vrtype, length, status = pgen_writer.encode_host(block, ploidies, n_threads=2)
        types, records = PC.reference_of(name, codes)
        assert status.tolist() == want_status, name
        assert vrtype.tolist() == types and out.tobytes() == b"".join(records), name  # the value's code is 3
        seen += 1
    assert seen > 200


def test_host_encoder_argument_errors():
    from sai_amd import _ffi
    from sai_amd.utils import pgen_writer

    lib = pgen_writer.load_host()
    assert lib.sai_pgen_export_abi_version() == pgen_writer.SAI_PGEN_EXPORT_ABI_VERSION == 1
    dosage = np.zeros((2, 5), dtype=np.int8)
    dosage[:, 1] = 1
    out, vt, ln, st = np.full(4, 0xA5, dtype=np.uint8), np.full(2, 0xA5, dtype=np.uint8), np.full(2, 77, dtype=np.uint32), np.full(2, -7, dtype=np.int32)
    total = C.c_int64(-9)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda *a: lib.sai_pgen_encode_host(*a, 1)  # noqa: E731
    good = (p(dosage), 2, 5, None, 2, p(out), 4, p(vt), p(ln), p(st), C.byref(total))
    refused = [
        ({0: None}, b"NULL buffer"), ({5: None}, b"NULL buffer"), ({7: None}, b"NULL buffer"), ({8: None}, b"NULL buffer"), ({9: None}, b"NULL buffer"),
        ({10: None}, b"NULL buffer"), ({4: 0}, b"NULL buffer"),  # no uniform ploidy and no array
        ({1: -1}, b"size out of range"), ({2: 0}, b"size out of range"), ({1: 2**62}, b"size out of range"), ({6: -1}, b"size out of range"),
        ({4: 3}, b"uniform_ploidy must be 0, 1 or 2"), ({4: -1}, b"uniform_ploidy must be 0, 1 or 2"),
    ]  # fmt: skip
    for change, message in refused:
        args = [change.get(k, v) for k, v in enumerate(good)]
        assert call(*args) == _ffi.SAI_ERR_ARG and message in lib.sai_last_error(), (change, message)
        assert (out == 0xA5).all() and (vt == 0xA5).all() and (ln == 77).all() and (st == -7).all()
    # records that do not fit in out: the tables and the total are written, no byte of out is
    args = [{6: 3}.get(k, v) for k, v in enumerate(good)]
    assert call(*args) == _ffi.SAI_ERR_ARG and b"the records take 4 bytes and out holds 3" in lib.sai_last_error()
    assert (out == 0xA5).all() and vt.tolist() == [0, 0] and ln.tolist() == [2, 2] and total.value == 4
    assert call(*good) == 0 and out.tolist() == [0b00000100, 0] * 2
    total.value = -9
    assert call(None, 0, 5, None, 2, None, 0, None, None, None, C.byref(total)) == 0 and total.value == 0  # no row: fine


@pytest.mark.parametrize("case", [c for c in PC.CASES if c.codes.shape[0] != 130], ids=[c.name for c in PC.CASES if c.codes.shape[0] != 130])
def test_round_trip_through_the_host_decoder(case):
    """The written records through ``sai_pgen_decode_host`` at the ploidies they were written with: the block."""
    from sai_amd import _ffi, _ffi_pgen
    from sai_amd.utils import pgen_writer

    lib = _ffi_pgen.load_host()
    out, vrtype, length, _ = pgen_writer.encode_host(case.block, case.ploidies)
    assert np.array_equal(decode_host(lib, _ffi, out, vrtype, length, case.ploidies, case.block.shape), case.block)


def decode_host(lib, _ffi, out, vrtype, length, ploidies, shape):
    n_rows, n = shape
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ends = np.cumsum(length, dtype=np.int64)
    rec = np.ascontiguousarray(np.stack([ends - length, length.astype(np.int64), vrtype.astype(np.int64)], axis=1))
    base, flip = np.full((n_rows, 3), -1, dtype=np.int64), np.zeros(n_rows, dtype=np.uint8)
    cols, pl = np.arange(n, dtype=np.int32), np.ascontiguousarray(np.broadcast_to(np.asarray(ploidies, dtype=np.int32), (n,)))
    back, status = np.empty((n_rows, n), dtype=np.int8), np.empty(n_rows, dtype=np.int32)
    buf = np.ascontiguousarray(out) if out.size else np.zeros(1, dtype=np.uint8)
    _ffi.check(lib.sai_pgen_decode_host(p(buf), out.size, n_rows, p(rec), p(base), p(flip), n, n, p(cols), p(pl), p(back), p(status), 2))
    assert not status.any()
    return back


# ---- the stand-alone program under the sanitizers ----


def fnv1a(data: bytes) -> int:
    digest = 0xCBF29CE484222325
    for b in data:
        digest = ((digest ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return digest


def test_host_encoder_is_clean_under_asan_ubsan(tmp_path, tmp_path_factory):
    from sai_amd.utils import pgen_writer

    exe = native_build.dump_program("pgen_export_dump", tmp_path_factory)["san"]
    picked = [c for c in PC.CASES if c.codes.shape[0] == 17 and c.codes.shape[1] in (1, 5, 17, 257, 2002)] + [c for c in PC.CASES if c.family in ("types", "wide")]
    unfit = [(name, block, pl) for name, block, pl, _, _ in PC.unfit_cases()[::37]]
    assert len(picked) > 20 and len(unfit) > 5
    for name, block, ploidies in [(c.name, c.block, c.ploidies) for c in picked] + unfit:
        path = tmp_path / "block.bin"
        block.tofile(path)
        uniform, per_slot = pgen_writer.bed_writer._ploidy_arguments(ploidies)
        extra = [] if uniform else [",".join(map(str, per_slot))]
        res = native_build.run_native(exe, [path, *block.shape, uniform, 3, *extra])
        assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, (name, res.stderr[-3000:])
        out, vrtype, length, status = pgen_writer.encode_host(block, ploidies)
        lines = res.stdout.splitlines()
        assert [[int(v) for v in line.split()] for line in lines[:3]] == [status.tolist(), vrtype.tolist(), length.tolist()], name
        assert lines[3] == f"{out.size} {fnv1a(out.tobytes()):016x}", name
    res = native_build.run_native(exe, [path, *block.shape, 3, 1])
    assert res.returncode == 3 and "uniform_ploidy must be 0, 1 or 2" in res.stderr and "Sanitizer" not in res.stderr


# ---- convert, on the host route ----


@pytest.fixture
def host_route(monkeypatch, in_repo_root):
    monkeypatch.setenv("SAI_AMD_INGEST", "host")


def fileset_bytes(prefix):
    return {ext: open(prefix + ext, "rb").read() for ext in (".pgen", ".pvar", ".psam")}


def check_text_files(prefix, vcf, chrom, names, start=None, end=None, skip_multi=False):
    from sai_amd.utils.bed_writer import SiteColumns

    with SiteColumns(vcf, chrom, start, end) as sites:
        ids, ref, alt = sites.columns()
        rows = [f"{chrom}\t{sites.pos[k]}\t{ids[k]}\t{ref[k]}\t{alt[k]}" for k in range(sites.n_rows) if not (skip_multi and sites.multi[k])]
    assert open(prefix + ".pvar").read() == "#CHROM\tPOS\tID\tREF\tALT\n" + "".join(r + "\n" for r in rows)
    assert open(prefix + ".psam").read() == "#IID\tSEX\n" + "".join(f"{s}\tNA\n" for s in names)
    return len(rows)


def same_block(got, want):
    return got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1]) and got[2:] == want[2:]


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", FIXTURES)
def test_convert_writes_the_fileset_of_the_fixture(host_route, tmp_path, vcf, chrom, cfgfile, anc):
    from sai_amd.sai import convert
    from sai_amd.utils import native_vcf, pgen, pgen_writer
    from sai_amd.utils.bed_writer import header_samples

    prefix = str(tmp_path / "out")
    summary = convert(vcf, chrom, out_pfile=prefix)
    names = header_samples(vcf)
    n_rows = check_text_files(prefix, vcf, chrom, names)
    positions = native_vcf.load_dosage(vcf, chrom, names, [2] * len(names))[0]
    assert summary["rows_written"] == n_rows == len(positions) and summary["rows_skipped"] == 0 and summary["samples"] == len(names)
    data = open(prefix + ".pgen", "rb").read()
    assert summary["bytes"] == len(data) and set(summary["ms"]) == {"read", "site_scan", "encode", "d2h", "write", "total"}
    assert pgen.header_counts(prefix) == (n_rows, len(names)) and data[:3] == pgen_writer.MAGIC and pgen.is_fileset(prefix)
    # the file is the test writer's for the codes the VCF reader's block stands for
    block = native_vcf.load_dosage(vcf, chrom, names, [2] * len(names))[1]
    codes = np.select([block == 0, block == 1, block == 2], [0, 1, 2], 3).astype(np.uint8)
    assert np.array_equal(PC.block_of(codes, 2), block)
    types = PC.reference_of(("fixture", vcf), codes)[0]
    assert data == pgen_builder.build_pgen(codes, types=types, len_bytes=pgen_writer.length_bytes(len(names)))[0]
    # read back at the ploidy it was written with: the VCF reader's block, with and without ancestral alleles
    compared = 0
    for anc_file in [None, anc] if anc else [None]:
        for start, end in regions_of(positions):
            try:
                want_block = native_vcf.load_dosage(vcf, chrom, names, [2] * len(names), start, end, anc_file)
            except ValueError as exc:
                with pytest.raises(ValueError) as mine_exc:
                    pgen.load_dosage(prefix, chrom, names, [2] * len(names), start, end, anc_file)
                assert str(mine_exc.value) == str(exc)
                continue
            assert same_block(pgen.load_dosage(prefix, chrom, names, [2] * len(names), start, end, anc_file), want_block)
            compared += 1
    assert compared >= 4
    # --start / --end, and a subset of the samples in another order
    lo, hi = regions_of(positions)[1]
    part = str(tmp_path / "part")
    pick = names[::-1][: max(1, len(names) // 2)]
    assert convert(vcf, chrom, out_pfile=part + ".pgen", samples=pick, start=lo, end=hi)["rows_written"] == int(((positions >= lo) & (positions <= hi)).sum())
    assert check_text_files(part, vcf, chrom, pick, lo, hi) == int(((positions >= lo) & (positions <= hi)).sum())
    assert same_block(pgen.load_dosage(part, chrom, pick, [2] * len(pick))[:2], native_vcf.load_dosage(vcf, chrom, pick, [2] * len(pick), lo, hi)[:2])


def test_convert_at_mixed_ploidies_and_in_many_batches(host_route, tmp_path, monkeypatch):
    from sai_amd.sai import convert
    from sai_amd.utils import native_vcf, pgen

    case = mixed_case(tmp_path)
    vcf, names, ploidies = case["vcf"], case["samples"], case["ploidies"]
    whole = str(tmp_path / "whole")
    assert convert(vcf, "7", out_pfile=whole, haploid_samples=case["haploid"])["rows_written"] == 100
    assert check_text_files(whole, vcf, "7", names) == 100 and open(whole + ".pvar").read().splitlines()[1].split("\t")[2] == "."  # ID as the VCF has it
    for anc in (None, case["anc"]):
        for start, end in regions_of(np.array(case["positions"])):
            want = native_vcf.load_dosage(vcf, "7", names, ploidies, start, end, anc)
            assert same_block(pgen.load_dosage(whole, "7", names, ploidies, start, end, anc), want)
    assert (pgen.load_dosage(whole, "7", names, ploidies)[1][:, np.array(ploidies) == 1] == -1).any()  # a missing haploid call
    # several batches (16 rows each) write the same bytes
    monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", "64")
    convert(vcf, "7", out_pfile=str(tmp_path / "small"), haploid_samples=case["haploid"])
    assert fileset_bytes(str(tmp_path / "small")) == fileset_bytes(whole)


def test_convert_skips_multiallelic_records(host_route, tmp_path):
    from sai_amd.sai import convert
    from sai_amd.utils import native_vcf, pgen

    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\tc\n"
    rows = [("5", 10, "A", "C", "0|0\t0|1\t1|1"), ("5", 20, "A", "C,G", "0|2\t1|1\t2|2"), ("5", 30, "G", "T", ".|.\t1|0\t0|0"), ("5", 40, "G", "T,A", "0|0\t0|0\t0|0")]
    vcf = _write(tmp_path / "multi.vcf", head + "".join(f"{c}\t{p}\t.\t{r}\t{a}\t.\t.\t.\tGT\t{g}\n" for c, p, r, a, g in rows))
    before = listing(tmp_path)
    with pytest.raises(ValueError, match=r"multi.vcf: the record at position 20 of chromosome 5 has more than one ALT allele, and a .pgen record holds two alleles "
                                         r".2 such records: --skip-multiallelic"):  # fmt: skip
        convert(vcf, "5", out_pfile=str(tmp_path / "m"))
    assert listing(tmp_path) == before
    summary = convert(vcf, "5", out_pfile=str(tmp_path / "m"), skip_multiallelic=True)
    assert (summary["rows_written"], summary["rows_skipped"]) == (2, 2)
    pos, dos, _, _ = pgen.load_dosage(str(tmp_path / "m"), "5", ["a", "b", "c"], [2, 2, 2])
    want = native_vcf.load_dosage(vcf, "5", ["a", "b", "c"], [2, 2, 2])
    assert pos.tolist() == [10, 30] and np.array_equal(dos, want[1][[0, 2]]) and dos.tolist() == [[0, 1, 2], [-2, 1, 0]]
    assert open(str(tmp_path / "m") + ".pvar").read() == "#CHROM\tPOS\tID\tREF\tALT\n5\t10\t.\tA\tC\n5\t30\t.\tG\tT\n"
    assert check_text_files(str(tmp_path / "m"), vcf, "5", ["a", "b", "c"], skip_multi=True) == 2
    for call, dosage in (("./0", -1), ("2|2", 4), ("1|2", 3)):
        bad = _write(tmp_path / "bad.vcf", head + f"5\t10\t.\tA\tC\t.\t.\t.\tGT\t0|0\t{call}\t1|1\n")
        before = listing(tmp_path)
        with pytest.raises(ValueError, match=f"bad.vcf: the call of sample b at position 10 has dosage {dosage} at ploidy 2: a .pgen record holds"):
            convert(bad, "5", out_pfile=str(tmp_path / "b"))
        assert listing(tmp_path) == before


def test_convert_refusals_leave_nothing_behind(host_route, tmp_path, monkeypatch):
    from sai_amd.sai import convert
    from sai_amd.utils import pgen_writer

    case = mixed_case(tmp_path)
    vcf, hap = case["vcf"], case["haploid"]
    out = str(tmp_path / "out")
    done = str(tmp_path / "done")
    convert(vcf, "7", out_pfile=done, haploid_samples=hap)
    import bcf_builder

    bcf = bcf_builder.write_bcf(tmp_path / "example.bcf", bcf_builder.read_vcf_text("tests/data/example.vcf"))
    before = listing(tmp_path)

    def refused(match, *args, exc=ValueError, **kw):
        with pytest.raises(exc, match=match):
            convert(*args, **kw)
        assert listing(tmp_path) == before

    refused("done.pgen is a PLINK 2 fileset, already a binary format", done + ".pgen", "7", out_pfile=out)
    refused("example.bcf is a BCF file, already a binary format", str(bcf), "21", out_pfile=out)
    refused("ploidy 3: a PLINK 2 fileset holds haploid and diploid calls only", vcf, "7", out_pfile=out, ploidy=3)
    refused("ploidy 0", vcf, "7", out_pfile=out, ploidy=0)
    refused(f"^samples not found in {vcf}: zz$", vcf, "7", out_pfile=out, samples=["s0", "zz", "yy"])
    refused(f"^samples not found in {vcf}: nobody$", vcf, "7", out_pfile=out, haploid_samples=["nobody"])
    refused("sample s1 is asked for twice: a .psam names a sample once", vcf, "7", out_pfile=out, samples=["s1", "s2", "s1"])
    refused("absent.vcf is not found", str(tmp_path / "absent.vcf"), "7", out_pfile=out)
    refused(r"mixed.vcf: the call of sample s\d+ at position \d+ has dosage -1 at ploidy 2: a .pgen record holds", vcf, "7", out_pfile=out)
    refused("mixed.vcf: no record of chromosome 9$", vcf, "9", out_pfile=out)
    refused("mixed.vcf: no record of chromosome 7 in the region 1000000-1000010", vcf, "7", out_pfile=out, start=1000000, end=1000010)
    refused("done.pgen exists: name another prefix", vcf, "7", out_pfile=done, haploid_samples=hap)
    refused("done.pgen exists: name another prefix", vcf, "7", out_pfile=done + ".pgen", haploid_samples=hap)
    refused(r"out.pgen: --append does not go with --out-pfile, because the record table of a .pgen sits at the front of the file", vcf, "7", out_pfile=out,
            haploid_samples=hap, append=True)  # fmt: skip
    refused("name either out_prefix .PLINK 1. or out_pfile .PLINK 2.", vcf, "7", out, out_pfile=out)
    refused("name either out_prefix", vcf, "7")
    # a failure after the first batch has been written: the temporary files go
    monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", "64")
    real, calls = pgen_writer.check_io, []

    def failing(lib, rc):
        calls.append(rc)
        if len(calls) == 2:
            raise OSError("injected")
        return real(lib, rc)

    monkeypatch.setattr(pgen_writer, "check_io", failing)
    refused("injected", vcf, "7", out_pfile=out, haploid_samples=hap, exc=OSError)
    assert len(calls) == 2


def test_pvar_lines_are_the_bim_lines_in_another_order():
    from sai_amd.utils import pgen_writer

    bim = b"".join(b"%d\t%s\t0\t%d\t%s\t%s\n" % (k % 23, b"." if k % 3 else b"rs%d" % k, 100 + k * 37, b"ACGT"[k % 4 : k % 4 + 1] * (1 + k % 3), b"TG"[k % 2 : k % 2 + 1])
                   for k in range(300))  # fmt: skip
    want = b"".join(b"\t".join([f[0], f[3], f[1], f[5], f[4]]) + b"\n" for f in (line.split(b"\t") for line in bim.splitlines()))
    assert pgen_writer.pvar_text(bim) == want and pgen_writer.pvar_text(b"") == b"" and pgen_writer.pvar_text(b"1\t\t0\t5\tC\t\n") == b"1\t5\t\t\tC\n"
    for bad in (b"1\ta\t0\t5\tC\n", b"1\ta\t0\t5\tC\tA\tx\n", b"1\ta\t0\t5\tC\tA", b"1\ta\t0\t5\tC\tA\n\n"):
        with pytest.raises(ValueError, match="not six tab-separated columns ended by a newline"):
            pgen_writer.pvar_text(bad)


# ---- the build and the command line ----


def test_units_header_and_binding():
    from sai_amd import _build
    from sai_amd.utils import bed_writer, pgen_writer

    assert "pgen/pgen_encode.hip" in _build.UNITS and "pgen/pgen_encode.hip" not in _build.HOST_UNITS and "pgen/pgen_encode_host.cpp" in _build.HOST_UNITS
    header = _build.CSRC / "pgen" / "pgen_export.hpp"
    assert header in _build.staleness_inputs() and not (_build.INCLUDE / "pgen_export.hpp").exists()
    text = header.read_text()
    assert "#define SAI_PGEN_EXPORT_ABI_VERSION 1\n" in text
    for name in pgen_writer.SIGNATURES:
        assert f" {name}(" in text, name
    lib = pgen_writer.load()
    assert lib.sai_pgen_export_abi_version() == 1 and all(hasattr(lib, name) for name in pgen_writer.SIGNATURES)
    assert set(pgen_writer.HOST_SYMBOLS) == {"sai_pgen_export_abi_version", "sai_pgen_encode_host", "sai_pgen_pvar_lines"} and pgen_writer.load_host() is not None
    assert bed_writer.load().sai_bed_export_abi_version() == 1  # the .bed export's version stays


def test_command_line(tmp_path, monkeypatch):
    from sai_amd.parsers.convert_parser import PGEN_NOTE, PROMISE

    res = sai_cli("convert", "--help")
    flat = " ".join(res.stdout.split())
    assert res.returncode == 0 and PROMISE in flat and PGEN_NOTE in flat and "has not been opened with plink2" in PGEN_NOTE
    for flag in ("--vcf FILE", "--chr-name C", "--out-bfile PREFIX", "--out-pfile PREFIX", "--ploidy {1,2}", "--haploid FILE", "--samples FILE", "--start N",
                 "--end N", "--append", "--skip-multiallelic"):  # fmt: skip
        assert flag in flat, flag
    case = mixed_case(tmp_path)
    hap = tmp_path / "hap.txt"
    hap.write_text("".join(f"{s}\tpop\n" for s in case["haploid"]))
    prefix = str(tmp_path / "cli")
    monkeypatch.setenv("SAI_AMD_INGEST", "host")  # the child processes inherit it
    common = ("convert", "--vcf", case["vcf"], "--chr-name", "7", "--haploid", str(hap), "--end", str(case["positions"][49]))
    res = sai_cli(*common, "--out-pfile", prefix, "--out-bfile", prefix)
    assert res.returncode == 2 and "not allowed with argument" in res.stderr
    res = sai_cli(*common)
    assert res.returncode == 2 and "one of the arguments --out-bfile --out-pfile is required" in res.stderr
    res = sai_cli(*common, "--out-pfile", prefix, "--append")
    assert res.returncode == 2 and "--append does not go with --out-pfile" in res.stderr and listing(tmp_path) == sorted(["hap.txt", "mixed.vcf", "mixed.anc.bed"])
    res = sai_cli(*common, "--out-pfile", prefix)
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads(res.stdout.splitlines()[-1])["rows_written"] == 50
    from sai_amd.sai import convert

    convert(case["vcf"], "7", out_pfile=str(tmp_path / "api"), haploid_samples=case["haploid"], end=case["positions"][49])
    assert fileset_bytes(prefix) == fileset_bytes(str(tmp_path / "api"))
