"""A VCF's calls written as a PLINK 1 fileset, on the host: the encoder ``sai_bed_encode_host`` against a numpy
statement of its table, the site scanner against ``vcf.read_site_columns``, both as stand-alone programs under the
sanitizers, and ``convert`` under ``SAI_AMD_INGEST=host`` against the filesets ``test_plink_cpu`` writes and against
the VCF reader on the same calls."""

import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import native_build
from test_ingest_native import write_bgzf
from test_plink_cpu import FIXTURES, HET, HOM_A1, HOM_A2, MISSING, fileset_from_vcf, regions_of, sai_cli, write_vcf

WIDTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65]
BAD_INDEX = 0x7FFFFFFF
# dosage -> code, per ploidy: the unflipped column of include/saihip_plink.h, read backwards
TABLE = {2: {2: 0b00, 1: 0b10, 0: 0b11, -2: 0b01}, 1: {1: 0b00, 0: 0b11, -1: 0b01}}
# every value that does not fit, with the ploidy it is planted at
UNFIT = [(-128, 2), (-3, 2), (-1, 2), (-2, 1), (2, 1), (3, 2), (4, 2), (127, 2), (3, 1), (4, 1), (127, 1), (-128, 1)]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def numpy_encode(dosage, ploidies):
    """The table as numpy states it: (rows uint8 [n][ceil(slots / 4)], status int32 [n])."""
    dosage = np.asarray(dosage, dtype=np.int8)
    n_rows, n_slots = dosage.shape
    pl = np.broadcast_to(np.asarray(ploidies, dtype=np.int64), (n_slots,))
    codes = np.full(dosage.shape, 0b01, dtype=np.uint8)
    fits = np.zeros(dosage.shape, dtype=bool)
    for ploidy, table in TABLE.items():
        for value, code in table.items():
            hit = (dosage == value) & (pl == ploidy)[None, :]
            codes[hit] = code
            fits |= hit
    padded = np.zeros((n_rows, -(-n_slots // 4) * 4), dtype=np.uint8)
    padded[:, :n_slots] = codes
    quads = padded.reshape(n_rows, -1, 4)
    rows = (quads[:, :, 0] | quads[:, :, 1] << 2 | quads[:, :, 2] << 4 | quads[:, :, 3] << 6).astype(np.uint8)
    status = np.zeros(n_rows, dtype=np.int32)
    for r in range(n_rows):
        bad = np.flatnonzero(~fits[r])
        if bad.size:
            status[r] = n_slots - int(bad[0])
    status[:] = np.where(np.isin(pl, (1, 2)).all(), status, BAD_INDEX)
    return rows, status


def random_block(rng, n_rows, n_slots, ploidies):
    """Values of the table only, every one of them likely."""
    pl = np.broadcast_to(np.asarray(ploidies), (n_slots,))
    dip = rng.choice(np.array([2, 1, 0, -2], dtype=np.int8), size=(n_rows, n_slots))
    hap = rng.choice(np.array([1, 0, -1], dtype=np.int8), size=(n_rows, n_slots))
    return np.where((pl == 2)[None, :], dip, hap).astype(np.int8)


def ploidy_cases(rng, n_slots):
    return [("uniform 2", 2), ("uniform 1", 1), ("mixed", rng.integers(1, 3, n_slots).astype(np.int32))]


@pytest.mark.parametrize("n_slots", WIDTHS)
def test_host_encoder_restates_the_table(n_slots):
    from sai_amd.utils.bed_writer import encode_host

    rng = np.random.default_rng(500 + n_slots)
    for n_rows in (1, 2, 7):
        for name, ploidies in ploidy_cases(rng, n_slots):
            dosage = random_block(rng, n_rows, n_slots, ploidies)
            rows, status = encode_host(dosage, ploidies, n_threads=3)
            want_rows, want_status = numpy_encode(dosage, ploidies)
            assert rows.shape == (n_rows, (n_slots + 3) // 4) and np.array_equal(rows, want_rows), (n_rows, name)
            assert not status.any() and not want_status.any()
            if n_slots % 4:  # the unused bits of a row's last byte
                assert not (rows[:, -1] >> (2 * (n_slots % 4))).any()


@pytest.mark.parametrize("n_slots", WIDTHS)
def test_host_encoder_flags_every_value_that_does_not_fit(n_slots):
    from sai_amd.utils.bed_writer import encode_host

    rng = np.random.default_rng(900 + n_slots)
    for value, ploidy in UNFIT:
        for where in sorted({0, n_slots // 2, n_slots - 1}):
            for name, ploidies in (("uniform", ploidy), ("mixed", np.where(np.arange(n_slots) == where, ploidy, rng.integers(1, 3, n_slots)).astype(np.int32))):
                dosage = random_block(rng, 3, n_slots, ploidies)
                dosage[1, where] = value
                if where + 2 < n_slots:  # a second one behind it: the lowest slot is reported
                    dosage[1, n_slots - 1] = value if np.ndim(ploidies) == 0 or ploidies[n_slots - 1] == ploidy else 77
                rows, status = encode_host(dosage, ploidies, n_threads=2)
                want_rows, want_status = numpy_encode(dosage, ploidies)
                assert status.tolist() == want_status.tolist() == [0, n_slots - where, 0], (value, ploidy, where, name)
                assert np.array_equal(rows, want_rows) and (rows[1, where // 4] >> (2 * (where % 4))) & 3 == 0b01


def test_host_encoder_argument_errors_and_bad_ploidies():
    from sai_amd import _ffi
    from sai_amd.utils import bed_writer

    lib = bed_writer.load_host()
    assert lib.sai_bed_export_abi_version() == bed_writer.SAI_BED_EXPORT_ABI_VERSION == 1
    dosage = np.zeros((2, 5), dtype=np.int8)
    rows, status, pl = np.full((2, 2), 0xA5, dtype=np.uint8), np.full(2, -7, dtype=np.int32), np.full(5, 2, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda *a: lib.sai_bed_encode_host(*a, 1)  # noqa: E731
    refused = [
        ((None, 2, 5, None, 2, p(rows), p(status)), b"NULL buffer"),
        ((p(dosage), 2, 5, None, 2, None, p(status)), b"NULL buffer"),
        ((p(dosage), 2, 5, None, 2, p(rows), None), b"NULL buffer"),
        ((p(dosage), 2, 5, None, 0, p(rows), p(status)), b"NULL buffer"),  # no uniform ploidy and no array
        ((p(dosage), -1, 5, None, 2, p(rows), p(status)), b"size out of range"),
        ((p(dosage), 2, 0, None, 2, p(rows), p(status)), b"size out of range"),
        ((p(dosage), 2**62, 5, None, 2, p(rows), p(status)), b"size out of range"),
        ((p(dosage), 2, 5, None, 3, p(rows), p(status)), b"uniform_ploidy must be 0, 1 or 2"),
        ((p(dosage), 2, 5, None, -1, p(rows), p(status)), b"uniform_ploidy must be 0, 1 or 2"),
    ]
    for args, message in refused:
        assert call(*args) == _ffi.SAI_ERR_ARG and message in lib.sai_last_error(), message
        assert (rows == 0xA5).all() and (status == -7).all()
    assert call(None, 0, 5, None, 2, None, None) == 0 and (rows == 0xA5).all()  # no row: fine, nothing touched
    # a ploidy outside 1 .. 2 in the array: the row's status says so, the field is 01
    for bad in (0, 3, -1):
        pl[3] = bad
        assert call(p(dosage), 2, 5, p(pl), 0, p(rows), p(status)) == 0
        assert status.tolist() == [BAD_INDEX, BAD_INDEX] and rows.tolist() == [[0b01111111, 0b11]] * 2
        assert np.array_equal(rows, numpy_encode(dosage, pl)[0])


@pytest.mark.parametrize("n_slots", WIDTHS + [2002])
def test_round_trip_through_the_host_decoder(n_slots):
    """Random codes -> sai_plink_decode_host -> sai_bed_encode_host: the same bytes (no het at ploidy 1)."""
    from sai_amd import _ffi, _ffi_plink
    from sai_amd.utils.bed_writer import encode_host

    lib = _ffi_plink.load_host()
    rng = np.random.default_rng(70 + n_slots)
    n_rows, row_bytes = 7, (n_slots + 3) // 4
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for name, ploidies in ploidy_cases(rng, n_slots):
        pl = np.broadcast_to(np.asarray(ploidies, dtype=np.int32), (n_slots,)).copy()
        codes = rng.integers(0, 4, size=(n_rows, n_slots)).astype(np.uint8)
        codes[:, pl == 1] = rng.choice(np.array([HOM_A1, MISSING, HOM_A2], dtype=np.uint8), size=(n_rows, int((pl == 1).sum())))
        padded = np.zeros((n_rows, row_bytes * 4), dtype=np.uint8)
        padded[:, :n_slots] = codes
        quads = padded.reshape(n_rows, -1, 4)
        bed = np.ascontiguousarray(quads[:, :, 0] | quads[:, :, 1] << 2 | quads[:, :, 2] << 4 | quads[:, :, 3] << 6, dtype=np.uint8)
        dosage, status = np.empty((n_rows, n_slots), dtype=np.int8), np.empty(n_rows, dtype=np.int32)
        rib, flip, cols = np.arange(n_rows, dtype=np.int32), np.zeros(n_rows, dtype=np.uint8), np.arange(n_slots, dtype=np.int32)
        _ffi.check(lib.sai_plink_decode_host(p(bed), n_rows, row_bytes, n_rows, p(rib), p(flip), n_slots, n_slots, p(cols), p(pl), p(dosage), p(status), 2))
        assert not status.any()
        back, st = encode_host(dosage, ploidies, n_threads=2)
        assert not st.any() and np.array_equal(back, bed), name


# ---- the site scanner ----


def as_three(tmp_path, vcf):
    """The VCF as plain text, gzip and bgzip (small ragged members: lines straddle them)."""
    opener = gzip.open if str(vcf).endswith(".gz") else open
    with opener(vcf, "rb") as f:
        text = f.read()
    stem = os.path.basename(str(vcf)).replace(".gz", "")
    plain, gz, bgz = tmp_path / stem, tmp_path / (stem + ".gz"), tmp_path / (stem + ".bgz")
    plain.write_bytes(text)
    with gzip.open(gz, "wb") as f:
        f.write(text)
    write_bgzf(bgz, text, np.random.default_rng(5))
    return [str(plain), str(gz), str(bgz)]


def chromosomes_of(vcf):
    from sai_amd.utils.vcf import _open_text

    with _open_text(vcf) as f:
        return list(dict.fromkeys(line.split("\t", 1)[0] for line in f if not line.startswith("#")))


def check_scanner(path, chrom, start, end, n_threads=3):
    from sai_amd.utils.bed_writer import SiteColumns, header_samples
    from sai_amd.utils.vcf import _open_text, read_site_columns

    pos, ref, alt = read_site_columns(path, chrom, start, end)
    with _open_text(path) as f:
        wanted = [line.split("\t", 5) for line in f if not line.startswith("#")]
    wanted = [w for w in wanted if w[0] == chrom and (start is None or int(w[1]) >= start) and (end is None or int(w[1]) <= end)]
    with SiteColumns(path, chrom, start, end, n_threads) as sites:
        ids, got_ref, got_alt = sites.columns()
        assert sites.pos.dtype == np.int32 and sites.pos.tolist() == pos.tolist() and got_ref == ref and got_alt == alt
        assert ids == [w[2] for w in wanted] and sites.multi.tolist() == [int("," in w[4]) for w in wanted]
        assert sites.samples == header_samples(path)
        lines = sites.bim_text(sites.multi).decode().splitlines()
        assert lines == [f"{chrom}\t{w[2]}\t0\t{int(w[1])}\t{w[4].strip()}\t{w[3]}" for w in wanted if "," not in w[4]]
    return len(pos)


@pytest.mark.parametrize("vcf", sorted(str(p) for p in (native_build.ROOT / "tests" / "data").glob("*.vcf*") if not str(p).endswith((".tbi", ".csi"))))
def test_site_scanner_equals_read_site_columns(tmp_path, vcf):
    from sai_amd.utils.vcf import read_site_columns

    seen = 0
    for path in as_three(tmp_path, vcf):
        for chrom in chromosomes_of(path)[:3] + ["nope"]:
            here = read_site_columns(path, chrom)[0]
            regions = regions_of(here) if len(np.unique(here)) > 3 else [(None, None)]
            for start, end in regions:
                seen += check_scanner(path, chrom, start, end)
    assert seen > 0


def test_site_scanner_on_hand_built_text(tmp_path):
    """A chromosome in two runs, long lines -- one of them longer than the buffer the gzip pass starts with -- a last
    line without a newline, ALT with commas, ALT as the line's last column, and text large enough for several threads."""
    from sai_amd.utils.bed_writer import SiteColumns

    samples = [f"s{i}" for i in range(3)]
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n"
    long_info = "X" * 300000
    records = [("7", 10, "a", "A", "C"), ("8", 11, ".", "G", "T"), ("7", 12, "b", "AT", "A,ATT"), ("77", 13, "c", "A", "C"), ("7", 14, ".", "C", "G,T,A")]
    body = "".join(f"{c}\t{p}\t{i}\t{r}\t{a}\t.\tPASS\t{long_info * (17 if k == 6 else 1)}\tGT\t0|0\t0|1\t1|1\n" for k, (c, p, i, r, a) in enumerate(records * 3))
    text = head + body + "7\t99\tlast\tA\tG"  # five columns, no newline
    for path in as_three(tmp_path, _write(tmp_path / "hand.vcf", text)):
        for n_threads in (1, 3, 16):
            assert check_scanner(path, "7", None, None, n_threads) == 10
            assert check_scanner(path, "7", 12, 14, n_threads) == 6
            assert check_scanner(path, "77", None, None, n_threads) == 3
        with SiteColumns(path, "7") as sites:
            assert sites.samples == samples and sites.pos.tolist() == [10, 12, 14] * 3 + [99] and sites.multi.tolist() == [0, 1, 1] * 3 + [0]
            assert sites.columns() == (["a", "b", "."] * 3 + ["last"], ["A", "AT", "C"] * 3 + ["A"], ["C", "A", "G"] * 3 + ["G"])
    # refusals: no header, a record cut short, a position that is no number, a file that is not there
    for name, bad, message in (("nohead", body, "not a VCF .no #CHROM header"), ("short", head + "7\t5\tx\tA\n", "fewer than 5 columns"),
                               ("pos", head + "7\tfive\tx\tA\tC\n", "has the position 'five'")):  # fmt: skip
        with pytest.raises(ValueError, match=message):
            SiteColumns(_write(tmp_path / f"{name}.vcf", bad), "7")
    with pytest.raises(ValueError, match="cannot open .*absent.vcf"):
        SiteColumns(str(tmp_path / "absent.vcf"), "7")
    # a gzip file cut off in the middle of its stream is refused, not scanned as if it were whole
    whole = open(tmp_path / "hand.vcf.gz", "rb").read()
    cut = tmp_path / "cut.vcf.gz"
    cut.write_bytes(whole[: len(whole) // 2])
    with pytest.raises(ValueError, match="cut.vcf.gz: the gzip stream ends before its end mark"):
        SiteColumns(str(cut), "7")


def _write(path, text):
    with open(path, "w", newline="") as f:
        f.write(text)
    return str(path)


# ---- the stand-alone programs under the sanitizers ----


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return {name: native_build.dump_program(name, tmp_path_factory)["san"] for name in ("bed_encode_dump", "vcf_sites_dump")}


def clean(res):
    return res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr


def test_host_encoder_is_clean_under_asan_ubsan(tmp_path, programs):
    from sai_amd.utils.bed_writer import encode_host

    rng = np.random.default_rng(11)
    for n_rows, n_slots in ((1, 1), (7, 5), (2, 16), (7, 65), (3, 2002)):
        for name, ploidies in ploidy_cases(rng, n_slots):
            dosage = random_block(rng, n_rows, n_slots, ploidies)
            dosage[n_rows - 1, n_slots - 1] = 99  # also the flagged path
            block = tmp_path / "block.bin"
            dosage.tofile(block)
            uniform = int(ploidies) if np.ndim(ploidies) == 0 else 0
            extra = [] if uniform else [",".join(map(str, ploidies))]
            res = native_build.run_native(programs["bed_encode_dump"], [block, n_rows, n_slots, uniform, 3, *extra])
            assert clean(res), res.stderr[-3000:]
            status_line, hex_line = res.stdout.splitlines()
            rows, status = encode_host(dosage, ploidies)
            assert [int(v) for v in status_line.split()] == status.tolist() and status[-1] == 1
            assert bytes.fromhex(hex_line) == rows.tobytes() and np.array_equal(rows, numpy_encode(dosage, ploidies)[0])
    res = native_build.run_native(programs["bed_encode_dump"], [block, 3, 2002, 3, 1])
    assert res.returncode == 3 and "uniform_ploidy must be 0, 1 or 2" in res.stderr and "Sanitizer" not in res.stderr


def test_site_scanner_is_clean_under_asan_ubsan(tmp_path, programs):
    from sai_amd.utils.bed_writer import SiteColumns

    for vcf, chrom, _, _ in FIXTURES:
        for path in as_three(tmp_path, vcf):
            for start, end in ((None, None), (1000, 60000)):
                res = native_build.run_native(programs["vcf_sites_dump"], [path, chrom, -1 if start is None else start, -1 if end is None else end, 3])
                assert clean(res), res.stderr[-3000:]
                lines = res.stdout.split("\n")
                with SiteColumns(path, chrom, start, end) as sites:
                    ids, ref, alt = sites.columns()
                    n = sites.n_rows
                    assert lines[0] == f"sites {n} {len(sites.samples)}" and lines[1].split("\t") == sites.samples
                    assert lines[2 : 2 + n] == [f"{sites.pos[k]} {sites.multi[k]} {ids[k]} {ref[k]} {alt[k]}" for k in range(n)]
                    assert "\n".join(lines[2 + n :]).encode() == sites.bim_text(sites.multi)
    res = native_build.run_native(programs["vcf_sites_dump"], [tmp_path / "absent.vcf", "1", -1, -1, 2])
    assert res.returncode == 3 and "cannot open" in res.stderr and "Sanitizer" not in res.stderr


# ---- convert, on the host route ----


@pytest.fixture
def host_route(monkeypatch, in_repo_root):
    monkeypatch.setenv("SAI_AMD_INGEST", "host")


def fileset_bytes(prefix):
    return {ext: open(prefix + ext, "rb").read() for ext in (".bed", ".bim", ".fam")}


def bim_columns(prefix):
    rows = [line.split("\t") for line in open(prefix + ".bim").read().splitlines()]
    return [[r[k] for r in rows] for k in range(6)]


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", FIXTURES)
def test_convert_writes_the_fileset_of_the_fixture(host_route, tmp_path, vcf, chrom, cfgfile, anc):
    from sai_amd.sai import convert
    from sai_amd.utils import native_vcf, plink
    from sai_amd.utils.bed_writer import header_samples

    prefix, ref_prefix = str(tmp_path / "out"), str(tmp_path / "ref")
    summary = convert(vcf, chrom, prefix)
    positions, chroms = fileset_from_vcf(vcf, ref_prefix)
    here = np.array(chroms) == chrom
    names = header_samples(vcf)
    row_bytes = (len(names) + 3) // 4
    # the .bed test_plink_cpu's converter writes: its rows of this chromosome (it writes every chromosome of the file)
    ref_bed = np.fromfile(ref_prefix + ".bed", dtype=np.uint8)
    want = bytes(ref_bed[:3]) + ref_bed[3:].reshape(-1, row_bytes)[here].tobytes()
    assert open(prefix + ".bed", "rb").read() == want
    assert summary["rows_written"] == int(here.sum()) and summary["rows_skipped"] == 0 and summary["samples"] == len(names)
    assert summary["bytes"] == len(want) and set(summary["ms"]) == {"read", "site_scan", "encode", "d2h", "write", "total"}
    mine, ref = bim_columns(prefix), bim_columns_any(ref_prefix)
    keep = [k for k, c in enumerate(ref[0]) if c == chrom]
    assert mine[0] == [chrom] * len(keep) and mine[2] == ["0"] * len(keep)
    for col in (3, 4, 5):  # positions and alleles
        assert mine[col] == [ref[col][k] for k in keep]
    assert open(prefix + ".fam").read() == "".join(f"{s} {s} 0 0 0 -9\n" for s in names)
    # read back at the ploidy it was written with: the VCF reader's block, with and without ancestral alleles
    compared = 0
    for anc_file in [None, anc] if anc else [None]:
        for start, end in regions_of(positions[here]):
            try:
                want_block = native_vcf.load_dosage(vcf, chrom, names, [2] * len(names), start, end, anc_file)
            except ValueError as exc:
                with pytest.raises(ValueError) as mine_exc:
                    plink.load_dosage(prefix, chrom, names, [2] * len(names), start, end, anc_file)
                assert str(mine_exc.value) == str(exc)
                continue
            got = plink.load_dosage(prefix, chrom, names, [2] * len(names), start, end, anc_file)
            assert got[0].tolist() == want_block[0].tolist() and np.array_equal(got[1], want_block[1]) and got[2:] == want_block[2:]
            compared += 1
    assert compared >= 4
    # a region of the file, and a subset of the samples in another order
    lo, hi = regions_of(positions[here])[1]
    part = str(tmp_path / "part")
    pick = names[::-1][: max(1, len(names) // 2)]
    assert convert(vcf, chrom, part, samples=pick, start=lo, end=hi)["rows_written"] == int(((positions[here] >= lo) & (positions[here] <= hi)).sum())
    got = plink.load_dosage(part, chrom, pick, [2] * len(pick))
    want_block = native_vcf.load_dosage(vcf, chrom, pick, [2] * len(pick), lo, hi)
    assert got[0].tolist() == want_block[0].tolist() and np.array_equal(got[1], want_block[1])


def bim_columns_any(prefix):
    rows = [line.split() for line in open(prefix + ".bim").read().splitlines()]
    return [[r[k] for r in rows] for k in range(6)]


def mixed_case(tmp_path, n=120, seed=3):
    """A VCF with haploid and diploid samples (test_plink_cpu.write_vcf) on two chromosomes."""
    rng = np.random.default_rng(seed)
    samples = [f"s{i}" for i in range(13)]
    haploid = [s for i, s in enumerate(samples) if i % 3 == 1]
    codes = rng.choice([HOM_A1, HET, HOM_A2, MISSING], size=(n, len(samples)), p=[0.3, 0.3, 0.3, 0.1]).astype(np.uint8)
    for s in haploid:
        col = samples.index(s)
        het = codes[:, col] == HET
        codes[het, col] = rng.choice([HOM_A1, HOM_A2], size=int(het.sum()))
    chroms = ["7"] * (n - 20) + ["8"] * 20
    positions = np.concatenate([np.cumsum(rng.integers(1, 90, n - 20)), np.cumsum(rng.integers(1, 90, 20))]).tolist()
    a1, a2 = rng.choice(list("AC"), n).tolist(), rng.choice(list("GT"), n).tolist()
    vcf = write_vcf(tmp_path / "mixed.vcf", chroms, positions, [f"rs{k}" if k % 4 else "." for k in range(n)], a1, a2, codes, samples, haploid)
    anc = tmp_path / "mixed.anc.bed"
    anc.write_text("".join(f"{chroms[k]}\t{positions[k] - 1}\t{positions[k]}\t{(a1[k], a2[k], 'N')[k % 3]}\n" for k in range(n) if k % 5))
    return dict(vcf=vcf, anc=str(anc), samples=samples, haploid=haploid, positions=positions[: n - 20], ploidies=[1 if s in haploid else 2 for s in samples])


def test_convert_at_mixed_ploidies_and_append(host_route, tmp_path, monkeypatch):
    from sai_amd.sai import convert
    from sai_amd.utils import native_vcf, plink

    case = mixed_case(tmp_path)
    vcf, names, ploidies = case["vcf"], case["samples"], case["ploidies"]
    whole = str(tmp_path / "whole")
    assert convert(vcf, "7", whole, haploid_samples=case["haploid"])["rows_written"] == 100
    assert bim_columns(whole)[1][:5] == [".", "rs1", "rs2", "rs3", "."]  # ID as the VCF has it
    for anc in (None, case["anc"]):
        for start, end in regions_of(np.array(case["positions"])):
            want = native_vcf.load_dosage(vcf, "7", names, ploidies, start, end, anc)
            got = plink.load_dosage(whole, "7", names, ploidies, start, end, anc)
            assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    assert (plink.load_dosage(whole, "7", names, ploidies)[1][:, np.array(ploidies) == 1] == -1).any()  # a missing haploid call
    # two ranges appended equal one conversion; a further chromosome goes behind them
    cut = case["positions"][40]
    parts = str(tmp_path / "parts")
    first = convert(vcf, "7", parts, haploid_samples=case["haploid"], end=cut, append=True)  # nothing there yet: a new fileset
    second = convert(vcf, "7", parts, haploid_samples=case["haploid"], start=cut + 1, append=True)
    assert first["rows_written"] + second["rows_written"] == 100 and fileset_bytes(parts) == fileset_bytes(whole)
    assert second["bytes"] == second["rows_written"] * 4 and first["bytes"] == 3 + first["rows_written"] * 4
    convert(vcf, "8", parts, haploid_samples=case["haploid"], append=True)
    convert(vcf, "8", str(tmp_path / "eight"), haploid_samples=case["haploid"])
    both = fileset_bytes(parts)
    assert both[".bed"] == fileset_bytes(whole)[".bed"] + fileset_bytes(str(tmp_path / "eight"))[".bed"][3:]
    want = native_vcf.load_dosage(vcf, "8", names, ploidies)
    got = plink.load_dosage(parts, "8", names, ploidies)
    assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1])
    # several batches (16 rows each) write the same bytes
    monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", "64")
    convert(vcf, "7", str(tmp_path / "small"), haploid_samples=case["haploid"])
    assert fileset_bytes(str(tmp_path / "small")) == fileset_bytes(whole)


def listing(tmp_path):
    return sorted(p.name for p in tmp_path.iterdir())


def test_convert_refusals_leave_nothing_behind(host_route, tmp_path):
    from sai_amd.sai import convert
    from sai_amd.utils import native_vcf

    case = mixed_case(tmp_path)
    vcf, hap = case["vcf"], case["haploid"]
    out = str(tmp_path / "out")
    before = listing(tmp_path)

    def refused(match, *args, exc=ValueError, **kw):
        with pytest.raises(exc, match=match):
            convert(*args, **kw)
        assert listing(tmp_path) == before

    # a fileset or a BCF as input
    done = str(tmp_path / "done")
    convert(vcf, "7", done, haploid_samples=hap)
    before = listing(tmp_path)
    refused("done.bed is a PLINK fileset, already a binary format", done + ".bed", "7", out)
    refused("done is a PLINK fileset, already a binary format", done, "7", out)
    import bcf_builder

    bcf = bcf_builder.write_bcf(tmp_path / "example.bcf", bcf_builder.read_vcf_text("tests/data/example.vcf"))
    before = listing(tmp_path)
    refused("example.bcf is a BCF file, already a binary format", str(bcf), "21", out)
    # ploidy, samples
    refused("ploidy 3: a PLINK 1 fileset holds haploid and diploid calls only", vcf, "7", out, ploidy=3)
    refused("ploidy 0", vcf, "7", out, ploidy=0)
    with pytest.raises(ValueError) as from_reader:
        native_vcf.load_dosage(vcf, "7", ["s0", "zz", "yy"], [2, 2, 2])
    assert str(from_reader.value) == f"samples not found in {vcf}: zz"
    refused(f"^samples not found in {vcf}: zz$", vcf, "7", out, samples=["s0", "zz", "yy"])
    refused(f"^samples not found in {vcf}: nobody$", vcf, "7", out, haploid_samples=["nobody"])
    # a call that does not fit: a haploid call read at ploidy 2 is padded with a missing allele, so "0" has dosage -1
    refused(r"mixed.vcf: the call of sample s\d+ at position \d+ has dosage -1 at ploidy 2", vcf, "7", out)
    # no record
    refused("mixed.vcf: no record of chromosome 9$", vcf, "9", out)
    refused("mixed.vcf: no record of chromosome 7 in the region 1000000-1000010", vcf, "7", out, start=1000000, end=1000010)
    # an existing .bed without --append
    refused("done.bed exists: name another prefix, or add its rows to it with --append", vcf, "7", done, haploid_samples=hap)
    # the three --append mismatches, and an error in the middle of an append: the files are what they were
    kept = fileset_bytes(done)
    refused("done.fam names 13 samples and the conversion 12, the first difference at line 1", vcf, "8", done, samples=case["samples"][1:], append=True)
    refused(r"the call of sample s\d+ at position \d+ has dosage -1 at ploidy 2", vcf, "8", done, append=True)  # same samples, fails while encoding
    assert fileset_bytes(done) == kept
    with open(done + ".bim", "a") as f:
        f.write("7\tx\t0\t1\tA\tC\n")
    before = listing(tmp_path)
    refused(r"done.bed: 403 bytes, but 3 \+ 101 variants of the .bim x 4 bytes for 13 samples is 407", vcf, "8", done, haploid_samples=hap, append=True)
    with open(done + ".bed", "r+b") as f:
        f.write(b"\x6c\x1b\x00")
    refused("done.bed: not a variant-major PLINK 1 .bed file .it starts with 6c1b00.", vcf, "8", done, haploid_samples=hap, append=True)
    os.remove(done + ".fam")
    before = listing(tmp_path)
    refused("done.fam is not found: --append needs the three files", vcf, "8", done, haploid_samples=hap, append=True)


def test_convert_multiallelic_records_and_what_does_not_fit(host_route, tmp_path):
    from sai_amd.sai import convert
    from sai_amd.utils import native_vcf, plink

    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\tc\n"
    rows = [("5", 10, "A", "C", "0|0\t0|1\t1|1"), ("5", 20, "A", "C,G", "0|2\t1|1\t2|2"), ("5", 30, "G", "T", ".|.\t1|0\t0|0"), ("5", 40, "G", "T,A", "0|0\t0|0\t0|0")]
    vcf = _write(tmp_path / "multi.vcf", head + "".join(f"{c}\t{p}\t.\t{r}\t{a}\t.\t.\t.\tGT\t{g}\n" for c, p, r, a, g in rows))
    before = listing(tmp_path)
    with pytest.raises(ValueError, match=r"multi.vcf: the record at position 20 of chromosome 5 has more than one ALT allele.*2 such records: --skip-multiallelic"):
        convert(vcf, "5", str(tmp_path / "m"))
    assert listing(tmp_path) == before
    summary = convert(vcf, "5", str(tmp_path / "m"), skip_multiallelic=True)
    assert (summary["rows_written"], summary["rows_skipped"]) == (2, 2)
    pos, dos, _, _ = plink.load_dosage(str(tmp_path / "m"), "5", ["a", "b", "c"], [2, 2, 2])
    want = native_vcf.load_dosage(vcf, "5", ["a", "b", "c"], [2, 2, 2])
    assert pos.tolist() == [10, 30] and np.array_equal(dos, want[1][[0, 2]]) and dos.tolist() == [[0, 1, 2], [-2, 1, 0]]
    assert open(str(tmp_path / "m") + ".bim").read() == "5\t.\t0\t10\tC\tA\n5\t.\t0\t30\tT\tG\n"
    # ./0 at ploidy 2 and allele index 2 without a second ALT: named by position, sample, dosage and ploidy
    for call, dosage in (("./0", -1), ("2|2", 4), ("1|2", 3)):
        bad = _write(tmp_path / "bad.vcf", head + f"5\t10\t.\tA\tC\t.\t.\t.\tGT\t0|0\t{call}\t1|1\n")
        before = listing(tmp_path)
        with pytest.raises(ValueError, match=f"bad.vcf: the call of sample b at position 10 has dosage {dosage} at ploidy 2: a .bed row holds"):
            convert(bad, "5", str(tmp_path / "b"))
        assert listing(tmp_path) == before
    bad = _write(tmp_path / "bad.vcf", head + "5\t10\t.\tA\tC\t.\t.\t.\tGT\t0|0\t2\t1|1\n")
    with pytest.raises(ValueError, match="bad.vcf: the call of sample b at position 10 has dosage 2 at ploidy 1: a .bed row holds"):
        convert(bad, "5", str(tmp_path / "b"), haploid_samples=["b"])
    assert listing(tmp_path) == before


def test_a_scan_that_disagrees_with_the_reader_writes_nothing(host_route, tmp_path, monkeypatch):
    from sai_amd.sai import convert
    from sai_amd.utils import bed_writer

    case = mixed_case(tmp_path)
    real = bed_writer.SiteColumns

    class OneShort(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.n_rows, self.pos = self.n_rows - 1, self.pos[:-1]

    monkeypatch.setattr(bed_writer, "SiteColumns", OneShort)
    before = listing(tmp_path)
    with pytest.raises(RuntimeError, match="the site scan found 99 records of chromosome 7 and the genotype reader 100"):
        convert(case["vcf"], "7", str(tmp_path / "out"), haploid_samples=case["haploid"])
    assert listing(tmp_path) == before

    class OtherNames(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.samples = self.samples[:-1]

    monkeypatch.setattr(bed_writer, "SiteColumns", OtherNames)
    with pytest.raises(RuntimeError, match="the site scan found 12 sample names on the #CHROM line and the header pass 13"):
        convert(case["vcf"], "7", str(tmp_path / "out"), haploid_samples=case["haploid"])
    assert listing(tmp_path) == before


# ---- the build and the command line ----


def test_units_header_and_binding():
    from sai_amd import _build
    from sai_amd.utils import bed_writer

    assert "plink/bed_encode.hip" in _build.UNITS and "plink/bed_encode.hip" not in _build.HOST_UNITS
    assert {"plink/bed_encode_host.cpp", "plink/vcf_sites.cpp"} <= set(_build.HOST_UNITS) and _build.UNITS[-len(_build.HOST_UNITS):] == _build.HOST_UNITS
    header = _build.CSRC / "plink" / "bed_export.hpp"
    assert header in _build.staleness_inputs() and not (_build.INCLUDE / "bed_export.hpp").exists()
    text = header.read_text()
    for name in bed_writer.SIGNATURES:
        assert f" {name}(" in text, name
    lib = bed_writer.load()
    assert lib.sai_bed_export_abi_version() == 1 and all(hasattr(lib, name) for name in bed_writer.SIGNATURES)
    assert set(bed_writer.HOST_SYMBOLS) == set(bed_writer.SIGNATURES) - {"sai_bed_encode"}


def test_command_line(tmp_path, monkeypatch):
    from sai_amd.parsers.convert_parser import PROMISE

    res = sai_cli("convert", "--help")
    flat = " ".join(res.stdout.split())
    assert res.returncode == 0 and PROMISE in flat and "byte for byte" in PROMISE
    for flag in ("--vcf FILE", "--chr-name C", "--out-bfile PREFIX", "--ploidy {1,2}", "--haploid FILE", "--samples FILE", "--start N", "--end N",
                 "--append", "--skip-multiallelic"):  # fmt: skip
        assert flag in flat, flag
    case = mixed_case(tmp_path)
    hap = tmp_path / "hap.txt"
    hap.write_text("".join(f"{s}\tpop\n" for s in case["haploid"]))
    env_prefix = str(tmp_path / "cli")
    monkeypatch.setenv("SAI_AMD_INGEST", "host")  # the child processes inherit it
    res = sai_cli("convert", "--vcf", case["vcf"], "--chr-name", "7", "--out-bfile", env_prefix, "--haploid", str(hap), "--end", str(case["positions"][49]))
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads(res.stdout.splitlines()[-1])["rows_written"] == 50
    res = sai_cli("convert", "--vcf", case["vcf"], "--chr-name", "7", "--out-bfile", env_prefix)
    assert res.returncode == 2 and "cli.bed exists" in res.stderr
    from sai_amd.sai import convert

    convert(case["vcf"], "7", str(tmp_path / "api"), haploid_samples=case["haploid"], end=case["positions"][49])
    assert fileset_bytes(env_prefix) == fileset_bytes(str(tmp_path / "api"))
