"""A VCF's calls written as an EIGENSOFT fileset, on the host: the encoder ``sai_geno_encode_host`` in its two forms
against the numpy statement of ``geno_export_cases`` and against the test writer of ``test_eigenstrat_cpu``, the hash of
the header record against its worked values, the encoder as a stand-alone program under the sanitizers, and
``convert(..., out_eigenstrat=)`` under ``SAI_AMD_INGEST=host`` against the VCF reader on the same calls."""

import ctypes as C
import json

import numpy as np
import pytest

import geno_export_cases as GC
import native_build
from test_bed_export_cpu import _write, listing, mixed_case
from test_eigenstrat_cpu import geno_bytes
from test_pgen_export_cpu import fnv1a
from test_plink_cpu import regions_of, sai_cli

FORMATS = ("packed", "transposed")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


# ---- the encoder ----


def test_numpy_statement_restates_the_issues_table():
    block, pl = GC.table_block()
    codes, status = GC.codes_of(block, pl)
    assert not status.any()
    for r in range(block.shape[0]):
        for s in range(block.shape[1]):
            want = {(2, 0): 2, (2, 1): 1, (2, 2): 0, (2, -2): 3, (1, 0): 2, (1, 1): 0, (1, -1): 3}[(int(pl[s]), int(block[r, s]))]
            assert codes[r, s] == want
    assert {(int(pl[s]), int(v)) for s in range(7) for v in block[:, s]} == {(2, 0), (2, 1), (2, 2), (2, -2), (1, 0), (1, 1), (1, -1)}  # every cell
    packed = GC.pack_records(np.array([[2, 1, 0, 3, 1]], dtype=np.uint8), 48)
    assert packed[0, :2].tolist() == [0b10010011, 0b01000000] and not packed[0, 2:].any()  # the first field in the two top bits


@pytest.mark.parametrize("shape", GC.shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_equals_the_numpy_statement(shape):
    from sai_amd.utils.geno_writer import encode_host, record_bytes

    n_rows, n_slots = shape
    rng = np.random.default_rng(1000 * n_rows + n_slots)
    for name, ploidies in GC.ploidy_cases(rng, n_slots):
        for flagged in (False, True):
            block = GC.random_block(rng, n_rows, n_slots, ploidies)
            if flagged:
                GC.plant_unfit(rng, block, ploidies)
            want, want_status = GC.numpy_encode(block, ploidies)
            records, status = encode_host(block, ploidies, n_threads=3)
            assert records.shape == (n_rows, record_bytes(n_slots)) == (n_rows, GC.record_bytes(n_slots)) and np.array_equal(records, want), (name, flagged)
            assert status.tolist() == want_status.tolist() and bool(status.any()) == flagged
            want_t, _ = GC.numpy_encode(block, ploidies, transposed=True)
            assert want_t.shape == (n_slots, GC.record_bytes(n_rows))
            combined = np.zeros(n_rows, dtype=np.int32)
            for slot0, n_out in GC.slot_groups(n_slots):
                records, status = encode_host(block, ploidies, transposed=True, slot0=slot0, n_out=n_out, n_threads=3)
                assert np.array_equal(records, want_t[slot0 : slot0 + n_out]), (name, flagged, slot0, n_out)
                want_part = GC.codes_of(block[:, slot0 : slot0 + n_out], np.broadcast_to(np.asarray(ploidies), (n_slots,))[slot0 : slot0 + n_out])[1]
                want_part = np.where((want_part > 0) & (want_part != GC.BAD_INDEX), want_part + n_slots - slot0 - n_out, want_part)  # counted from the block's end
                assert status.tolist() == want_part.tolist()
            # the calls over the slot groups of a block share the status: it is raised, never zeroed
            half = n_slots // 2
            for slot0, n_out in ((half, n_slots - half), (0, half)):
                encode_host(block, ploidies, transposed=True, slot0=slot0, n_out=n_out, status=combined, n_threads=2)
            assert combined.tolist() == want_status.tolist()


def test_every_table_cell_and_every_unfit_value():
    from sai_amd.utils.geno_writer import encode_host

    block, pl = GC.table_block()
    for transposed in (False, True):
        records, status = encode_host(block, pl, transposed=transposed)
        assert np.array_equal(records, GC.numpy_encode(block, pl, transposed)[0]) and not status.any()
    seen = 0
    for n_slots in (1, 5, 13, 193):
        rng = np.random.default_rng(900 + n_slots)
        for value, ploidy in GC.UNFIT:
            for where in sorted({0, n_slots // 2, n_slots - 1}):
                mixed = np.where(np.arange(n_slots) == where, ploidy, rng.integers(1, 3, n_slots)).astype(np.int32)
                for ploidies in (ploidy, mixed):
                    block = GC.random_block(rng, 3, n_slots, ploidies)
                    block[1, where] = value
                    if where + 2 < n_slots and np.broadcast_to(np.asarray(ploidies), (n_slots,))[n_slots - 1] == ploidy:
                        block[1, n_slots - 1] = value  # a second one behind it: the lowest slot is reported
                    for transposed in (False, True):
                        records, status = encode_host(block, ploidies, transposed=transposed, n_threads=2)
                        assert status.tolist() == [0, n_slots - where, 0], (value, ploidy, where, transposed)
                        assert np.array_equal(records, GC.numpy_encode(block, ploidies, transposed)[0])
                    assert (encode_host(block, ploidies)[0][1, where // 4] >> (6 - 2 * (where % 4))) & 3 == 3  # its field is 3
                    seen += 1
    assert seen > 100
    # a ploidy outside 1 .. 2: its field is 3 in every row, and every row says so
    for bad in (0, 3, -1):
        pl = np.array([2, 1, bad, 2, 1], dtype=np.int32)
        block = np.array([[0, 0, 0, 1, 1], [2, 1, 1, 5, -1]], dtype=np.int8)
        for transposed in (False, True):
            records, status = encode_host(block, pl, transposed=transposed)
            assert status.tolist() == [GC.BAD_INDEX] * 2 and np.array_equal(records, GC.numpy_encode(block, pl, transposed)[0])
        assert encode_host(block, pl)[0][:, 0].tolist() == [0b10101101, 0b00001111]


def test_data_records_are_the_test_writers():
    """``geno_bytes`` of tests/test_eigenstrat_cpu.py builds the files the reader's tests read: its records are ours."""
    from sai_amd.utils.geno_writer import encode_host

    for n_rows, n_slots in ((5, 13), (193, 193), (257, 65), (17, 2002)):
        rng = np.random.default_rng(n_rows + n_slots)
        for name, ploidies in GC.ploidy_cases(rng, n_slots):
            block = GC.random_block(rng, n_rows, n_slots, ploidies)
            g = GC.codes_of(block, ploidies)[0]
            for fmt in FORMATS:
                records = encode_host(block, ploidies, transposed=fmt == "transposed")[0]
                theirs = geno_bytes(fmt, g)
                assert theirs[records.shape[1] :] == records.tobytes(), (n_rows, n_slots, name, fmt)


def test_host_encoder_argument_errors():
    from sai_amd import _ffi
    from sai_amd.utils import geno_writer

    lib = geno_writer.load_host()
    assert lib.sai_geno_export_abi_version() == geno_writer.SAI_GENO_EXPORT_ABI_VERSION == 1
    dosage = np.zeros((2, 5), dtype=np.int8)
    out, status = np.full((5, 48), 0xA5, dtype=np.uint8), np.full(2, -7, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = (p(dosage), 2, 5, None, 2, 0, 0, 5, p(out), p(status), 1)
    refused = [
        ({0: None}, b"NULL buffer"), ({8: None}, b"NULL buffer"), ({9: None}, b"NULL buffer"), ({4: 0}, b"NULL buffer"),
        ({1: -1}, b"size out of range"), ({2: 0}, b"size out of range"), ({1: 2**62}, b"size out of range"),
        ({4: 3}, b"uniform_ploidy must be 0, 1 or 2"), ({4: -1}, b"uniform_ploidy must be 0, 1 or 2"),
        ({6: 1}, b"slot0 + n_out exceeds n_slots"), ({7: 6}, b"slot0 + n_out exceeds n_slots"), ({6: -1}, b"slot0 + n_out exceeds n_slots"),
        ({7: 4}, b"the packed form takes every slot"), ({5: 1, 6: 3, 7: 3}, b"slot0 + n_out exceeds n_slots"),
    ]  # fmt: skip
    for change, message in refused:
        args = [change.get(k, v) for k, v in enumerate(good)]
        assert lib.sai_geno_encode_host(*args) == _ffi.SAI_ERR_ARG and message in lib.sai_last_error(), (change, message)
        assert (out == 0xA5).all() and (status == -7).all()
    assert lib.sai_geno_encode_host(None, 0, 5, None, 2, 0, 0, 5, None, None, 1) == 0  # no row: fine, nothing touched
    assert lib.sai_geno_encode_host(p(dosage), 2, 5, None, 2, 1, 2, 0, None, None, 1) == 0  # no slot: the same
    assert (out == 0xA5).all() and (status == -7).all()
    assert lib.sai_geno_encode_host(*good) == 0 and status.tolist() == [0, 0] and out[0, :3].tolist() == [0b10101010, 0b10000000, 0] and (out[2:] == 0xA5).all()


# ---- the hash and the text ----


def test_hash_worked_values_and_mirror():
    """The rule as the issue states it: hashit("ab") = 97 * 23 + 98, hasharr(["ab", "c"]) = (2329 * 17) ^ 99."""
    from sai_amd.utils import geno_writer

    assert GC.hashit(b"ab") == 2329 and GC.hasharr(["ab", "c"]) == 0x9ACA
    assert geno_writer.hash_lines(b"ab\n") == 2329 and geno_writer.hash_lines(b"ab U pop\nc\tU\tpop\n") == 0x9ACA and geno_writer.hash_lines(b"") == 0
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"abcXYZ019_:.-\xc3\xa9", dtype=np.uint8)
    names = [bytes(rng.choice(alphabet, size=int(rng.integers(1, 40)))) for _ in range(500)]
    text = b"".join(n + (b" " if k % 2 else b"\t") + b"U label%d\n" % k for k, n in enumerate(names))
    assert geno_writer.hash_lines(text) == GC.hasharr(names) and geno_writer.hash_lines(text) > 0xFFFF  # 32 bits, wrapped many times
    assert geno_writer.hash_lines(text[:-1]) == GC.hasharr(names)  # a last line without its newline


def test_snp_lines_are_the_bim_lines_in_another_order():
    from sai_amd.utils import geno_writer

    bim = b"".join(b"%d\t%s\t0\t%d\t%s\t%s\n" % (k % 23, b"." if k % 3 else b"rs%d" % k, 100 + k * 37, b"ACGT"[k % 4 : k % 4 + 1] * (1 + k % 3), b"TG"[k % 2 : k % 2 + 1])
                   for k in range(300))  # fmt: skip
    want = b"".join(b"\t".join([f[0] + b":" + f[3] if f[1] == b"." else f[1], f[0], b"0.0", f[3], f[5], f[4]]) + b"\n" for f in (line.split(b"\t") for line in bim.splitlines()))
    assert geno_writer.snp_text(bim) == want and geno_writer.snp_text(b"") == b"" and geno_writer.snp_text(b"1\t..\t0\t5\tC\t\n") == b"..\t1\t0.0\t5\t\tC\n"
    for bad in (b"1\ta\t0\t5\tC\n", b"1\ta\t0\t5\tC\tA\tx\n", b"1\ta\t0\t5\tC\tA", b"1\ta\t0\t5\tC\tA\n\n"):
        with pytest.raises(ValueError, match="not six tab-separated columns ended by a newline"):
            geno_writer.snp_text(bad)


# ---- the stand-alone program under the sanitizers ----


def test_host_encoder_is_clean_under_asan_ubsan(tmp_path, tmp_path_factory):
    from sai_amd.utils import bed_writer, geno_writer

    exe = native_build.dump_program("geno_export_dump", tmp_path_factory)["san"]
    runs = 0
    for n_rows, n_slots in [(1, 1), (5, 13), (17, 193), (193, 5), (257, 65), (16, 2002), (1000, 12)]:
        rng = np.random.default_rng(n_rows * 7 + n_slots)
        for name, ploidies in GC.ploidy_cases(rng, n_slots):
            block = GC.plant_unfit(rng, GC.random_block(rng, n_rows, n_slots, ploidies), ploidies)
            path = tmp_path / "block.bin"
            block.tofile(path)
            uniform, per_slot = bed_writer._ploidy_arguments(ploidies)
            extra = [] if uniform else [",".join(map(str, per_slot))]
            for transposed, slot0, n_out in [(0, 0, n_slots), (1, 0, n_slots), (1, n_slots // 3, n_slots - n_slots // 3)]:
                res = native_build.run_native(exe, ["encode", path, n_rows, n_slots, uniform, 3, transposed, slot0, n_out, *extra])
                assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, (name, res.stderr[-3000:])
                records, status = geno_writer.encode_host(block, ploidies, transposed=bool(transposed), slot0=slot0, n_out=n_out)
                lines = res.stdout.splitlines()
                assert [int(v) for v in lines[0].split()] == status.tolist() and status.any(), name
                assert lines[1] == f"{records.size} {fnv1a(records.tobytes()):016x}", name
                runs += 1
    assert runs >= 60
    res = native_build.run_native(exe, ["encode", path, n_rows, n_slots, 3, 1, 0, 0, n_slots])
    assert res.returncode == 3 and "uniform_ploidy must be 0, 1 or 2" in res.stderr and "Sanitizer" not in res.stderr
    bim = b"".join(b"7\t%s\t0\t%d\t%s\tA\n" % (b"." if k % 3 else b"rs%d" % k, 5 + 11 * k, b"C" * (1 + k % 4)) for k in range(200))
    (tmp_path / "sites.bim").write_bytes(bim)
    res = native_build.run_native(exe, ["text", tmp_path / "sites.bim"])
    assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
    snp = geno_writer.snp_text(bim)
    assert res.stdout.split() == ["%x" % geno_writer.hash_lines(bim), str(len(snp)), f"{fnv1a(snp):016x}", "%x" % geno_writer.hash_lines(snp)]


# ---- convert, on the host route ----


@pytest.fixture
def host_route(monkeypatch, in_repo_root):
    monkeypatch.setenv("SAI_AMD_INGEST", "host")


def fileset_bytes(prefix):
    return {ext: open(prefix + ext, "rb").read() for ext in (".geno", ".snp", ".ind")}


def check_fileset(prefix, fmt, vcf, chrom, names, labels=None, start=None, end=None, skip_multi=False):
    """The three files against the site columns, the format rules and the Python mirror of the hash.  -> rows"""
    from sai_amd.utils.bed_writer import SiteColumns

    with SiteColumns(vcf, chrom, start, end) as sites:
        ids, ref, alt = sites.columns()
        rows = [(ids[k] if ids[k] != "." else f"{chrom}:{sites.pos[k]}", sites.pos[k], ref[k], alt[k]) for k in range(sites.n_rows) if not (skip_multi and sites.multi[k])]
    snp = open(prefix + ".snp").read()
    assert snp == "".join(f"{i}\t{chrom}\t0.0\t{p}\t{r}\t{a}\n" for i, p, r, a in rows)
    labels = labels or {}
    assert open(prefix + ".ind").read() == "".join(f"{s} U {labels.get(s, s)}\n" for s in names)
    data = open(prefix + ".geno", "rb").read()
    transposed = fmt == "transposed"
    rlen = GC.record_bytes(len(rows) if transposed else len(names))
    assert len(data) == rlen * (1 + (len(names) if transposed else len(rows)))
    text = "%s %7d %7d %x %x" % ("TGENO" if transposed else "GENO", len(names), len(rows), GC.hasharr(names), GC.hasharr([r[0] for r in rows]))
    assert len(text) <= 48 and data[:rlen] == text.encode() + b"\0" * (rlen - len(text))
    return len(rows)


def same_block(got, want):
    return got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1]) and got[2:] == want[2:]


@pytest.mark.parametrize("fmt", FORMATS)
def test_convert_at_mixed_ploidies_reads_back_as_the_vcf(host_route, tmp_path, monkeypatch, fmt):
    from sai_amd.sai import convert
    from sai_amd.utils import eigenstrat, native_vcf

    case = mixed_case(tmp_path)
    vcf, names, ploidies = case["vcf"], case["samples"], case["ploidies"]
    whole = str(tmp_path / "whole")
    summary = convert(vcf, "7", out_eigenstrat=whole, geno_format=fmt, haploid_samples=case["haploid"])
    assert (summary["rows_written"], summary["rows_skipped"], summary["samples"]) == (100, 0, 13)
    assert set(summary) == {"rows_written", "rows_skipped", "samples", "bytes", "ms"} and set(summary["ms"]) == {"read", "site_scan", "encode", "d2h", "write", "total"}
    assert check_fileset(whole, fmt, vcf, "7", names) == 100 and summary["bytes"] == len(fileset_bytes(whole)[".geno"])
    assert open(whole + ".snp").read().split("\n")[0].split("\t")[0] == f"7:{case['positions'][0]}"  # the "." of the VCF
    assert eigenstrat.is_fileset(whole)
    # the data records are the test writer's for the codes the VCF reader's block stands for
    block = native_vcf.load_dosage(vcf, "7", names, ploidies)[1]
    g, status = GC.codes_of(block, ploidies)
    rlen = GC.record_bytes(100 if fmt == "transposed" else 13)
    assert not status.any() and fileset_bytes(whole)[".geno"][rlen:] == geno_bytes(fmt, g)[rlen:]
    for anc in (None, case["anc"]):
        for start, end in regions_of(np.array(case["positions"])):
            want = native_vcf.load_dosage(vcf, "7", names, ploidies, start, end, anc)
            assert same_block(eigenstrat.load_dosage(whole, "7", names, ploidies, start, end, anc), want)
    assert (eigenstrat.load_dosage(whole, "7", names, ploidies)[1][:, np.array(ploidies) == 1] == -1).any()  # a missing haploid call
    # a subset of the samples in another order, with labels, inside a region
    lo, hi = regions_of(np.array(case["positions"]))[1]
    pick = names[::-1][:7]
    labels = {s: f"Pop{k % 2}" for k, s in enumerate(pick[:5])}
    part = str(tmp_path / "part")
    hap = [s for s in case["haploid"] if s in pick]
    n_part = int(((np.array(case["positions"]) >= lo) & (np.array(case["positions"]) <= hi)).sum())
    assert convert(vcf, "7", out_eigenstrat=part + ".geno", geno_format=fmt, samples=pick, haploid_samples=hap, start=lo, end=hi, labels=labels)["rows_written"] == n_part
    assert check_fileset(part, fmt, vcf, "7", pick, labels, lo, hi) == n_part
    pl = [1 if s in hap else 2 for s in pick]
    assert same_block(eigenstrat.load_dosage(part, "7", pick, pl)[:2], native_vcf.load_dosage(vcf, "7", pick, pl, lo, hi)[:2])
    # several batches write the same bytes: 64 bytes are 16 rows of the packed form (the least), one individual of the transposed one
    monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", "64")
    convert(vcf, "7", out_eigenstrat=str(tmp_path / "small"), geno_format=fmt, haploid_samples=case["haploid"])
    assert fileset_bytes(str(tmp_path / "small")) == fileset_bytes(whole)


def test_convert_skips_multiallelic_records(host_route, tmp_path):
    from sai_amd.sai import convert
    from sai_amd.utils import eigenstrat, native_vcf

    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\tc\n"
    rows = [("5", 10, "A", "C", "0|0\t0|1\t1|1"), ("5", 20, "A", "C,G", "0|2\t1|1\t2|2"), ("5", 30, "G", "TT", ".|.\t1|0\t0|0"), ("5", 40, "G", "T,A", "0|0\t0|0\t0|0")]
    vcf = _write(tmp_path / "multi.vcf", head + "".join(f"{c}\t{p}\t.\t{r}\t{a}\t.\t.\t.\tGT\t{g}\n" for c, p, r, a, g in rows))
    before = listing(tmp_path)
    with pytest.raises(ValueError, match=r"multi.vcf: the record at position 20 of chromosome 5 has more than one ALT allele, and a .geno record holds two alleles "
                                         r".2 such records: --skip-multiallelic"):  # fmt: skip
        convert(vcf, "5", out_eigenstrat=str(tmp_path / "m"))
    assert listing(tmp_path) == before
    for fmt in FORMATS:
        prefix = str(tmp_path / fmt)
        summary = convert(vcf, "5", out_eigenstrat=prefix, geno_format=fmt, skip_multiallelic=True)
        assert (summary["rows_written"], summary["rows_skipped"]) == (2, 2)
        pos, dos, _, _ = eigenstrat.load_dosage(prefix, "5", ["a", "b", "c"], [2, 2, 2])
        want = native_vcf.load_dosage(vcf, "5", ["a", "b", "c"], [2, 2, 2])
        assert pos.tolist() == [10, 30] and np.array_equal(dos, want[1][[0, 2]]) and dos.tolist() == [[0, 1, 2], [-2, 1, 0]]
        assert open(prefix + ".snp").read() == "5:10\t5\t0.0\t10\tA\tC\n5:30\t5\t0.0\t30\tG\tTT\n"  # a multi-character allele as the VCF spells it
        assert check_fileset(prefix, fmt, vcf, "5", ["a", "b", "c"], skip_multi=True) == 2
    for call, dosage in (("./0", -1), ("2|2", 4), ("1|2", 3)):
        bad = _write(tmp_path / "bad.vcf", head + f"5\t10\t.\tA\tC\t.\t.\t.\tGT\t0|0\t{call}\t1|1\n")
        before = listing(tmp_path)
        for fmt in FORMATS:
            with pytest.raises(ValueError, match=f"bad.vcf: the call of sample b at position 10 has dosage {dosage} at ploidy 2: a .geno record holds"):
                convert(bad, "5", out_eigenstrat=str(tmp_path / "b"), geno_format=fmt)
            assert listing(tmp_path) == before


def test_convert_refusals_leave_nothing_behind(host_route, tmp_path, monkeypatch):
    from sai_amd.sai import convert
    from sai_amd.utils import geno_writer

    case = mixed_case(tmp_path)
    vcf, hap = case["vcf"], case["haploid"]
    out = str(tmp_path / "out")
    done = str(tmp_path / "done")
    convert(vcf, "7", out_eigenstrat=done, haploid_samples=hap)
    import bcf_builder

    bcf = bcf_builder.write_bcf(tmp_path / "example.bcf", bcf_builder.read_vcf_text("tests/data/example.vcf"))
    before = listing(tmp_path)

    def refused(match, *args, exc=ValueError, **kw):
        with pytest.raises(exc, match=match):
            convert(*args, **kw)
        assert listing(tmp_path) == before

    refused("done.geno is an EIGENSTRAT fileset, already a binary format", done + ".geno", "7", out_eigenstrat=out)
    refused("example.bcf is a BCF file, already a binary format", str(bcf), "21", out_eigenstrat=out)
    refused("ploidy 3: an EIGENSOFT fileset holds haploid and diploid calls only", vcf, "7", out_eigenstrat=out, ploidy=3)
    refused(f"^samples not found in {vcf}: zz$", vcf, "7", out_eigenstrat=out, samples=["s0", "zz", "yy"])
    refused("sample s1 is asked for twice: a .ind names a sample once", vcf, "7", out_eigenstrat=out, samples=["s1", "s2", "s1"])
    for fmt in FORMATS:  # a half-missing call: a haploid call read at ploidy 2
        refused(r"mixed.vcf: the call of sample s\d+ at position \d+ has dosage -1 at ploidy 2: a .geno record holds", vcf, "7", out_eigenstrat=out, geno_format=fmt)
    refused("mixed.vcf: no record of chromosome 7 in the region 1000000-1000010", vcf, "7", out_eigenstrat=out, start=1000000, end=1000010)
    refused("done.geno exists: name another prefix", vcf, "7", out_eigenstrat=done, haploid_samples=hap)
    refused("done.geno exists: name another prefix", vcf, "7", out_eigenstrat=done + ".geno", haploid_samples=hap)
    refused(r"out.geno: --append does not go with --out-eigenstrat, because the counts of a .geno sit in its header record", vcf, "7", out_eigenstrat=out,
            haploid_samples=hap, append=True)  # fmt: skip
    refused("geno_format 'text': a .geno is written packed or transposed", vcf, "7", out_eigenstrat=out, geno_format="text")
    # the three-way rule; the sentence the two older writers' tests pin is still in it
    refused(r"name either out_prefix .PLINK 1. or out_pfile .PLINK 2. or out_eigenstrat .EIGENSOFT., not out_prefix and out_pfile$", vcf, "7", out, out_pfile=out)
    refused("not out_prefix and out_eigenstrat", vcf, "7", out, out_eigenstrat=out)
    refused("not out_pfile and out_eigenstrat", vcf, "7", out_pfile=out, out_eigenstrat=out)
    refused("not out_prefix and out_pfile and out_eigenstrat", vcf, "7", out, out_pfile=out, out_eigenstrat=out)
    refused(r"or out_eigenstrat .EIGENSOFT.$", vcf, "7")
    refused("geno_format and labels go with out_eigenstrat", vcf, "7", out, geno_format="transposed")
    # a failure after the first batch has been written: the temporary files go
    monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", "64")
    real = geno_writer.check_io
    for fmt in FORMATS:
        calls = []

        def failing(lib, rc):
            calls.append(rc)
            if len(calls) == 6:  # the two passes of the .snp lines, the two hashes, one batch; then this one
                raise OSError("injected")
            return real(lib, rc)

        monkeypatch.setattr(geno_writer, "check_io", failing)
        refused("injected", vcf, "7", out_eigenstrat=out, haploid_samples=hap, geno_format=fmt, exc=OSError)
        assert len(calls) == 6
        monkeypatch.setattr(geno_writer, "check_io", real)


# ---- the build and the command line ----


def test_units_header_and_binding():
    from sai_amd import _build
    from sai_amd.utils import bed_writer, geno_writer, pgen_writer

    device = [u for u in _build.UNITS if u not in _build.HOST_UNITS]
    assert device[device.index("eigenstrat/geno_transpose.hip") + 1] == "eigenstrat/geno_encode.hip" and device[-2:] == ["join/tile_parts.hip", "join/tile_rows.hip"]
    host = _build.HOST_UNITS
    assert host[host.index("eigenstrat/eigenstrat_index.cpp") + 1] == "eigenstrat/geno_encode_host.cpp" and host[-2:] == ["join/site_join_host.cpp", "join/site_join_many_host.cpp"]
    assert _build.UNITS[-len(host) :] == host
    header = _build.CSRC / "eigenstrat" / "geno_export.hpp"
    assert header in _build.staleness_inputs() and not (_build.INCLUDE / "geno_export.hpp").exists()
    text = header.read_text()
    assert "#define SAI_GENO_EXPORT_ABI_VERSION 1\n" in text and "geno_code_of(int32_t v, int32_t ploidy, bool* fits)" in text
    for name in geno_writer.SIGNATURES:
        assert f" {name}(" in text, name
    declared = {line.split("(")[0].split()[-1] for line in text.splitlines() if line.startswith("int sai_")}
    assert declared == set(geno_writer.SIGNATURES)  # names declared = names bound
    lib = geno_writer.load()
    assert lib.sai_geno_export_abi_version() == 1 and all(hasattr(lib, name) for name in geno_writer.SIGNATURES)
    assert set(geno_writer.HOST_SYMBOLS) == set(geno_writer.SIGNATURES) - {"sai_geno_encode", "sai_geno_encode_transposed"} and geno_writer.load_host() is not None
    assert bed_writer.load().sai_bed_export_abi_version() == 1 and pgen_writer.load().sai_pgen_export_abi_version() == 1  # the other two stay


def test_command_line(tmp_path, monkeypatch):
    from sai_amd.parsers.convert_parser import GENO_NOTE, PGEN_NOTE, PROMISE

    res = sai_cli("convert", "--help")
    flat = " ".join(res.stdout.split())
    assert res.returncode == 0 and PROMISE in flat and PGEN_NOTE in flat and GENO_NOTE in flat
    assert "unverified" in GENO_NOTE and "hashcheck: NO" in GENO_NOTE and "single-letter alleles" in GENO_NOTE
    for flag in ("--out-bfile PREFIX", "--out-pfile PREFIX", "--out-eigenstrat PREFIX", "--geno-format {packed,transposed}", "--samples FILE", "--append"):
        assert flag in flat, flag
    case = mixed_case(tmp_path)
    hap = tmp_path / "hap.txt"
    hap.write_text("".join(f"{s}\tpop\n" for s in case["haploid"]))
    keep = tmp_path / "keep.txt"
    keep.write_text("".join(f"{s}\tPop{k % 3}\n" if k % 4 else f"{s}\n" for k, s in enumerate(case["samples"][::-1])))
    ours = sorted(["hap.txt", "keep.txt", "mixed.vcf", "mixed.anc.bed"])
    prefix = str(tmp_path / "cli")
    monkeypatch.setenv("SAI_AMD_INGEST", "host")  # the child processes inherit it
    common = ("convert", "--vcf", case["vcf"], "--chr-name", "7", "--haploid", str(hap), "--samples", str(keep), "--end", str(case["positions"][49]))
    # the three messages the older writers' tests pin
    res = sai_cli(*common, "--out-pfile", prefix, "--out-bfile", prefix)
    assert res.returncode == 2 and "not allowed with argument" in res.stderr
    res = sai_cli(*common)
    assert res.returncode == 2 and "one of the arguments --out-bfile --out-pfile is required" in res.stderr and "--out-eigenstrat" in res.stderr
    res = sai_cli(*common, "--out-pfile", prefix, "--append")
    assert res.returncode == 2 and "--append does not go with --out-pfile" in res.stderr
    # the new usage errors
    for extra, message in (
        (("--out-eigenstrat", prefix, "--out-bfile", prefix), "argument --out-eigenstrat: not allowed with argument --out-bfile"),
        (("--out-eigenstrat", prefix, "--out-pfile", prefix), "argument --out-eigenstrat: not allowed with argument --out-pfile"),
        (("--out-eigenstrat", prefix, "--append"), "--append does not go with --out-eigenstrat"),
        (("--out-bfile", prefix, "--geno-format", "packed"), "--geno-format goes with --out-eigenstrat"),
        (("--out-pfile", prefix, "--geno-format", "transposed"), "--geno-format goes with --out-eigenstrat"),
        (("--out-eigenstrat", prefix, "--geno-format", "text"), "invalid choice: 'text'"),
    ):
        res = sai_cli(*common, *extra)
        assert res.returncode == 2 and message in res.stderr and listing(tmp_path) == ours, (extra, res.stderr[-500:])
    from sai_amd.sai import convert
    from sai_amd.utils.geno_writer import labels_of

    labels = labels_of(keep)
    assert len(labels) == 9 and labels["s11"] == "Pop1"
    for fmt in FORMATS:
        res = sai_cli(*common, "--out-eigenstrat", f"{prefix}_{fmt}", *(("--geno-format", fmt) if fmt != "packed" else ()))
        assert res.returncode == 0, res.stderr[-2000:]
        assert json.loads(res.stdout.splitlines()[-1])["rows_written"] == 50
        convert(case["vcf"], "7", out_eigenstrat=str(tmp_path / f"api_{fmt}"), geno_format=fmt, haploid_samples=case["haploid"], samples=case["samples"][::-1],
                end=case["positions"][49], labels=labels)  # fmt: skip
        assert fileset_bytes(f"{prefix}_{fmt}") == fileset_bytes(str(tmp_path / f"api_{fmt}"))
        assert check_fileset(f"{prefix}_{fmt}", fmt, case["vcf"], "7", case["samples"][::-1], labels, end=case["positions"][49]) == 50
    res = sai_cli(*common, "--out-eigenstrat", f"{prefix}_packed")
    assert res.returncode == 2 and "cli_packed.geno exists" in res.stderr
