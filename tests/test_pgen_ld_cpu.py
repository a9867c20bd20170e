"""LD-compressed ``.pgen`` records on the host (``sai convert --out-pfile --ld-compress``): every case of
``pgen_ld_cases`` proved to reach what it is named for, the encoder ``sai_pgen_encode_ld_host`` and the assembled file
against the test writer ``pgen_builder`` byte for byte, its sizes against the plain encoder's, the encoder as a
stand-alone program under the sanitizers, and ``convert(..., out_pfile=, ld_compress=True)`` under
``SAI_AMD_INGEST=host``: one batch against many, read back against the VCF reader, the refusals and the command line."""

import ctypes as C
import json

import numpy as np
import pytest

import native_build
import pgen_builder
import pgen_ld_cases as LC
from test_bed_export_cpu import listing
from test_pgen_export_cpu import decode_host, fileset_bytes, fnv1a, same_block
from test_plink_cpu import regions_of, sai_cli


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def base_rows(vrtype):
    """Per row the row a type 2 / 3 record lists against -- the last row before it of another type -- or -1."""
    out, last = [], -1
    for r, t in enumerate(vrtype):
        out.append(last if t in (2, 3) else -1)
        if t not in (2, 3):
            last = r
    return out


def entries_against_base(codes, types):
    """Per row of type 2 / 3 the number of samples its record lists; None for the other rows."""
    out = []
    for r, (t, b) in enumerate(zip(types, base_rows(types))):
        start = codes[b] if t == 2 else pgen_builder.swap02(codes[b]) if t == 3 else None
        out.append(None if start is None else int((codes[r] != start).sum()))
    return out


# ---- the cases ----


@pytest.mark.parametrize("case", LC.CASES, ids=LC.CASE_IDS)
def test_case_reaches_what_it_is_named_for(case):
    types, records, _ = LC.reference(case)
    n, want = case.codes.shape[1], case.want
    assert all(len(r) <= -(-n // 4) for r in records)  # no record is longer than its dense form: LB is known beforehand
    assert not {2, 3} & set(types[:: LC.SEGMENT])  # anchors
    bases = base_rows(types)
    assert all(b < 0 or b // LC.SEGMENT == r // LC.SEGMENT for r, b in enumerate(bases))  # a base lies in the row's segment
    if "types" in want:
        assert types == want["types"]
    if "w" in want:
        assert pgen_builder.index_width(n) == want["w"]
    if "L" in want:
        assert entries_against_base(case.codes, types) == want["L"]
        if "G" in want:
            assert -(-max(x for x in want["L"] if x is not None) // 64) == want["G"]
    if "lengths" in want:
        assert [len(r) for r in records] == want["lengths"]
    if "tie" in want:  # the two types take the same bytes for the last row, and the lower one is written
        low, high = want["tie"]
        row, base = case.codes[-1], case.codes[bases[-1] if bases[-1] >= 0 else len(types) - 2]
        sizes = {k: len(pgen_builder.encode(row, k, base)) for k in range(8) if k != 5}
        assert sizes[low] == sizes[high] == min(sizes.values()) and types[-1] == low and min(k for k, v in sizes.items() if v == sizes[low]) == low
    if case.family == "ploidies":
        pl = np.broadcast_to(np.asarray(case.ploidies), (n,))
        assert (pl == 1).any() and not (case.codes[:, pl == 1] == 1).any()


def test_the_families_together_reach_every_count_width_and_type():
    by_family = {}
    for case in LC.CASES:
        by_family.setdefault(case.family, []).append(case)
    assert [c.codes.shape[0] for c in by_family["rows"]] == list(LC.ROW_COUNTS) == [1, 15, 16, 17, 31, 32, 33]
    assert {2, 3} <= {t for c in by_family["rows"] for t in LC.reference(c)[0]}
    # a type 2 / 3 row right behind a segment's edge would be a fault: rows 16 and 32 are anchors, 17 and 33 may chain
    assert [c.codes.shape[1] for c in by_family["widths"]] == list(LC.WIDTHS) and [c.codes.shape[1] for c in by_family["wide"]] == [40000, 65537]
    for c in by_family["widths"] + by_family["wide"]:
        assert c.codes.shape[0] % LC.SEGMENT != 0 and (c.codes.shape[1] < 5 or {2, 3} & set(LC.reference(c)[0])), c.name
    assert {pgen_builder.index_width(n) for n in (255, 256, 65537)} == {1, 2, 3}
    for c in by_family["panel"]:
        assert {2, 3} <= set(LC.reference(c)[0]) and c.codes.shape[0] == 640 and (c.codes == 3).any()
    # a type 2 row behind a type 2 row, and one behind a non-anchor base
    chained = [c for c in LC.CASES if any(t in (2, 3) and r and LC.reference(c)[0][r - 1] in (2, 3) for r, t in enumerate(LC.reference(c)[0]))]
    rebased = [c for c in LC.CASES if any(b % LC.SEGMENT > 0 for b in base_rows(LC.reference(c)[0]) if b >= 0)]
    assert len(chained) > 10 and len(rebased) > 10


@pytest.mark.parametrize("case", LC.CASES, ids=LC.CASE_IDS)
def test_host_twin_and_assembled_file_equal_the_test_writer(case):
    from sai_amd.utils import pgen_writer

    types, records, data = LC.reference(case)
    out, vrtype, length, status = pgen_writer.encode_host(case.block, case.ploidies, n_threads=3, ld_compress=True)
    assert vrtype.tolist() == types and length.tolist() == [len(r) for r in records] and not status.any()
    assert out.tobytes() == b"".join(records)
    n = case.codes.shape[1]
    head = pgen_writer.assemble_header(n, vrtype, length)
    assert len(head) == pgen_writer.header_len(len(types), n) and head + out.tobytes() == data
    assert data[2] == 0x10 and data[11] == pgen_writer.length_bytes(n) - 1
    one = pgen_writer.encode_host(case.block, case.ploidies, n_threads=1, ld_compress=True)  # the split over threads changes nothing
    assert one[0].tobytes() == out.tobytes() and one[1].tolist() == types


@pytest.mark.parametrize("case", LC.CASES, ids=LC.CASE_IDS)
def test_ld_records_are_never_longer_than_the_plain_ones(case):
    """Row by row: the plain type is a candidate of every row.  Equal on rows drawn independently; strictly fewer bytes
    on the LD panel, whose copied rows are one byte each (at 2 002 samples the missing calls leave no exact copy, and
    the near copies make the difference)."""
    from sai_amd.utils import pgen_writer

    _, _, plain, _ = pgen_writer.encode_host(case.block, case.ploidies)
    _, vrtype, length, _ = pgen_writer.encode_host(case.block, case.ploidies, ld_compress=True)
    assert (length <= plain).all() and (length[~np.isin(vrtype, (2, 3))] == plain[~np.isin(vrtype, (2, 3))]).all()
    if case.family == "independent":
        assert (length == plain).all()
    if case.family == "panel":
        copies = [r for r, L in enumerate(entries_against_base(case.codes, vrtype.tolist())) if L == 0 and plain[r] > 1]
        assert int(length.sum()) < int(plain.sum()) and all(length[r] == 1 for r in copies) and (copies or case.codes.shape[1] > 200)
        print(f"{case.name}: {int(plain.sum())} B plain, {int(length.sum())} B with LD records, ratio {plain.sum() / length.sum():.3f}")


def test_status_of_values_that_do_not_fit():
    from sai_amd.utils import pgen_writer

    seen = set()
    for name, block, ploidies, codes, want_status in LC.unfit_cases():
        out, vrtype, length, status = pgen_writer.encode_host(block, ploidies, n_threads=2, ld_compress=True)
        types, records, _ = LC.reference_of(name, codes)
        assert status.tolist() == want_status, name
        assert vrtype.tolist() == types and out.tobytes() == b"".join(records), name  # the value's code is 3, in a base too
        seen |= {types[r] for r in (1, 5, 17)}
    assert {2, 3} & seen


def test_host_encoder_argument_errors():
    from sai_amd import _ffi
    from sai_amd.utils import pgen_writer

    lib = pgen_writer.load_ld_host()
    assert lib.sai_pgen_export_ld_version() == pgen_writer.SAI_PGEN_EXPORT_LD_VERSION == 1 and lib.sai_pgen_ld_segment() == pgen_writer.LD_SEGMENT == 16
    assert pgen_writer.load_host().sai_pgen_export_abi_version() == 1
    dosage = np.zeros((2, 5), dtype=np.int8)
    dosage[:, 1] = 1
    out, vt, ln, st = np.full(4, 0xA5, dtype=np.uint8), np.full(2, 0xA5, dtype=np.uint8), np.full(2, 77, dtype=np.uint32), np.full(2, -7, dtype=np.int32)
    total = C.c_int64(-9)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda *a: lib.sai_pgen_encode_ld_host(*a, 1)  # noqa: E731
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
    args = [{6: 2}.get(k, v) for k, v in enumerate(good)]
    assert call(*args) == _ffi.SAI_ERR_ARG and b"the records take 3 bytes and out holds 2" in lib.sai_last_error()
    assert (out == 0xA5).all() and vt.tolist() == [0, 2] and ln.tolist() == [2, 1] and total.value == 3
    assert call(*good) == 0 and out.tolist() == [0b00000100, 0, 0, 0xA5]  # the second row: a difflist of no entry
    total.value = -9
    assert call(None, 0, 5, None, 2, None, 0, None, None, None, C.byref(total)) == 0 and total.value == 0  # no row: fine


@pytest.mark.parametrize("case", LC.SMALL, ids=LC.SMALL_IDS)
def test_round_trip_through_the_host_decoder(case):
    """The written records through ``sai_pgen_decode_host`` at the ploidies they were written with: the block."""
    from sai_amd import _ffi, _ffi_pgen
    from sai_amd.utils import pgen_writer

    lib = _ffi_pgen.load_host()
    out, vrtype, length, _ = pgen_writer.encode_host(case.block, case.ploidies, ld_compress=True)
    assert np.array_equal(decode_host_with_bases(lib, _ffi, out, vrtype, length, case.ploidies, case.block.shape), case.block)
    plain = pgen_writer.encode_host(case.block, case.ploidies)
    assert np.array_equal(decode_host(lib, _ffi, *plain[:3], case.ploidies, case.block.shape), case.block)  # ... as the plain records do


def decode_host_with_bases(lib, _ffi, out, vrtype, length, ploidies, shape):
    n_rows, n = shape
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ends = np.cumsum(length, dtype=np.int64)
    rec = np.ascontiguousarray(np.stack([ends - length, length.astype(np.int64), vrtype.astype(np.int64)], axis=1))
    base, flip = np.full((n_rows, 3), -1, dtype=np.int64), np.zeros(n_rows, dtype=np.uint8)
    for r, b in enumerate(base_rows(vrtype.tolist())):
        if b >= 0:
            base[r] = rec[b]
    cols, pl = np.arange(n, dtype=np.int32), np.ascontiguousarray(np.broadcast_to(np.asarray(ploidies, dtype=np.int32), (n,)))
    back, status = np.empty((n_rows, n), dtype=np.int8), np.empty(n_rows, dtype=np.int32)
    _ffi.check(lib.sai_pgen_decode_host(p(np.ascontiguousarray(out)), out.size, n_rows, p(rec), p(base), p(flip), n, n, p(cols), p(pl), p(back), p(status), 2))
    assert not status.any()
    return back


# ---- the stand-alone program under the sanitizers ----


def test_host_encoder_is_clean_under_asan_ubsan(tmp_path, tmp_path_factory):
    from sai_amd.utils import pgen_writer

    exe = native_build.dump_program("pgen_ld_dump", tmp_path_factory)["san"]
    picked = [c for c in LC.SMALL if c.family in ("rows", "chain", "entries", "wide", "ploidies") or c.codes.shape[1] in (1, 5, 17, 257, 1025, 16385)]
    unfit = [(name, block, pl) for name, block, pl, _, _ in LC.unfit_cases()[::4]]
    assert len(picked) > 30 and len(unfit) > 3
    for name, block, ploidies in [(c.name, c.block, c.ploidies) for c in picked] + unfit:
        path = tmp_path / "block.bin"
        block.tofile(path)
        uniform, per_slot = pgen_writer.bed_writer._ploidy_arguments(ploidies)
        extra = [] if uniform else [",".join(map(str, per_slot))]
        res = native_build.run_native(exe, [path, *block.shape, uniform, 3, *extra])
        assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, (name, res.stderr[-3000:])
        out, vrtype, length, status = pgen_writer.encode_host(block, ploidies, ld_compress=True)
        lines = res.stdout.splitlines()
        assert [[int(v) for v in line.split()] for line in lines[:3]] == [status.tolist(), vrtype.tolist(), length.tolist()], name
        assert lines[3] == f"{out.size} {fnv1a(out.tobytes()):016x}", name
    res = native_build.run_native(exe, [path, *block.shape, 3, 1])
    assert res.returncode == 3 and "uniform_ploidy must be 0, 1 or 2" in res.stderr and "Sanitizer" not in res.stderr


# ---- convert, on the host route ----


@pytest.fixture
def host_route(monkeypatch, in_repo_root):
    monkeypatch.setenv("SAI_AMD_INGEST", "host")


def panel_vcf(tmp_path, n_rows=330, n=200, haploid=()):
    """The LD panel as a VCF of chromosome 9 (and a few rows of chromosome 10 behind it) -> (path, codes of chromosome 9)."""
    codes = LC.ld_panel(np.random.default_rng(n_rows), n_rows + 5, n)
    names = [f"s{k}" for k in range(n)]
    hap = {names.index(s) for s in haploid}
    for col in hap:
        codes[codes[:, col] == 1, col] = 2
    dip_call, hap_call = ("0|0", "0|1", "1|1", ".|."), ("0", None, "1", ".")
    positions = np.cumsum(np.random.default_rng(1).integers(50, 500, n_rows + 5))
    path = tmp_path / "panel.vcf"
    if not path.exists():
        with open(path, "w") as f:
            f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
            for k in range(n_rows + 5):
                calls = [(hap_call if c in hap else dip_call)[int(codes[k, c])] for c in range(n)]
                f.write("\t".join(["9" if k < n_rows else "10", str(positions[k]), f"rs{k}" if k % 3 else ".", "AC"[k % 2], "GT"[k % 2], ".", "PASS", ".", "GT", *calls]) + "\n")
    return str(path), codes[:n_rows]


def panel_config(tmp_path, n=200):
    """A configuration of ``score`` over the panel's samples: 90 reference, 90 target and 20 source individuals."""
    names = [f"s{k}" for k in range(n)]
    for label, pop, part in (("ref", "AFR", names[:90]), ("tgt", "CHB", names[90:180]), ("src", "Nean", names[180:])):
        (tmp_path / f"{label}.ind.list").write_text("".join(f"{pop}\t{s}\n" for s in part))
    text = open("tests/data/test_sai.config.yaml").read()
    for label in ("ref", "tgt", "src"):
        text = text.replace(f"tests/data/example.{label}.ind.list", str(tmp_path / f"{label}.ind.list"))
    (tmp_path / "panel.yaml").write_text(text)
    return str(tmp_path / "panel.yaml")


def record_types_of(prefix, n_rows):
    """{record type: count} from the header of PREFIX.pgen (fewer than 65 536 variants: one block)."""
    data = open(prefix + ".pgen", "rb").read()
    assert n_rows <= 65536 and int.from_bytes(data[3:7], "little") == n_rows and data[11] & 4 == 0
    nib = np.frombuffer(data[20 : 20 + (n_rows + 1) // 2], dtype=np.uint8)
    types = np.stack([nib & 15, nib >> 4], axis=1).reshape(-1)[:n_rows]
    return {int(t): int(c) for t, c in zip(*np.unique(types, return_counts=True))}


def test_convert_writes_the_ld_fileset_in_one_batch_and_in_many(host_route, tmp_path, monkeypatch):
    from sai_amd.sai import convert
    from sai_amd.utils import native_vcf, pgen, pgen_writer

    vcf, codes = panel_vcf(tmp_path)
    names = [f"s{k}" for k in range(codes.shape[1])]
    whole, plain = str(tmp_path / "whole"), str(tmp_path / "plain")
    summary = convert(vcf, "9", out_pfile=whole, ld_compress=True)
    without = convert(vcf, "9", out_pfile=plain)
    assert set(summary) == set(without) | {"record_types"} and "record_types" not in without
    assert summary["rows_written"] == len(codes) == 330 and summary["bytes"] < without["bytes"]
    types, _, data = LC.reference_of("panel vcf", codes)
    assert open(whole + ".pgen", "rb").read() == data and pgen.header_counts(whole) == (len(codes), len(names))
    assert summary["record_types"] == record_types_of(whole, len(codes)) == {t: types.count(t) for t in sorted(set(types))}
    assert summary["record_types"][2] > 0 and summary["record_types"][3] > 0 and not {2, 3} & set(record_types_of(plain, len(codes)))
    assert {ext: b for ext, b in fileset_bytes(whole).items() if ext != ".pgen"} == {ext: b for ext, b in fileset_bytes(plain).items() if ext != ".pgen"}
    # several batches (16 rows each, then 48) write the same bytes: a batch is a whole number of segments
    for k, batch in enumerate(("64", str(48 * 50))):
        monkeypatch.setenv("SAI_AMD_CONVERT_BATCH", batch)
        assert pgen_writer.bed_writer._batch_rows(50) in (16, 48)
        convert(vcf, "9", out_pfile=str(tmp_path / f"small{k}"), ld_compress=True)
        assert fileset_bytes(str(tmp_path / f"small{k}")) == fileset_bytes(whole)
    monkeypatch.delenv("SAI_AMD_CONVERT_BATCH")
    # read back: the VCF reader's block, with and without ancestral alleles, whole and by region (a region's first
    # row may be of type 2 or 3, its base before the region)
    positions = native_vcf.load_dosage(vcf, "9", names, [2] * len(names))[0]
    anc = tmp_path / "panel.anc.bed"
    anc.write_text("".join(f"9\t{p - 1}\t{p}\t{'ACGTN'[k % 5]}\n" for k, p in enumerate(positions.tolist()) if k % 7))
    regions = regions_of(positions) + [(int(positions[r]), int(positions[r + 3])) for r in range(1, len(types) - 3) if types[r] in (2, 3)][:6]
    compared = 0
    for anc_file in (None, str(anc)):
        for start, end in regions:
            try:
                want = native_vcf.load_dosage(vcf, "9", names, [2] * len(names), start, end, anc_file)
            except ValueError as exc:  # a region without a record: the same refusal
                with pytest.raises(ValueError) as mine:
                    pgen.load_dosage(whole, "9", names, [2] * len(names), start, end, anc_file)
                assert str(mine.value).replace(whole + ".pgen", vcf) == str(exc)
                continue
            assert same_block(pgen.load_dosage(whole, "9", names, [2] * len(names), start, end, anc_file), want)
            compared += 1
    assert compared >= 12
    pick = names[::-3]
    part = str(tmp_path / "part")
    convert(vcf, "9", out_pfile=part, samples=pick, start=int(positions[5]), end=int(positions[200]), ld_compress=True)
    assert same_block(pgen.load_dosage(part, "9", pick, [2] * len(pick))[:2], native_vcf.load_dosage(vcf, "9", pick, [2] * len(pick), int(positions[5]), int(positions[200]))[:2])


def test_convert_at_mixed_ploidies(host_route, tmp_path):
    from sai_amd.sai import convert
    from sai_amd.utils import native_vcf, pgen

    haploid = [f"s{k}" for k in range(0, 40, 3)]
    vcf, codes = panel_vcf(tmp_path, n_rows=100, n=40, haploid=haploid)
    names = [f"s{k}" for k in range(40)]
    ploidies = [1 if s in haploid else 2 for s in names]
    prefix = str(tmp_path / "mixed")
    summary = convert(vcf, "9", out_pfile=prefix, haploid_samples=haploid, ld_compress=True)
    assert summary["rows_written"] == 100 and {2, 3} & set(summary["record_types"])
    assert open(prefix + ".pgen", "rb").read() == LC.reference_of("mixed vcf", codes)[2]
    assert same_block(pgen.load_dosage(prefix, "9", names, ploidies), native_vcf.load_dosage(vcf, "9", names, ploidies))


def test_convert_refusals_leave_nothing_behind(host_route, tmp_path):
    from sai_amd.sai import convert

    vcf, _ = panel_vcf(tmp_path, n_rows=20, n=8)
    out = str(tmp_path / "out")
    before = listing(tmp_path)
    for kw in (dict(out_prefix=out), dict(out_eigenstrat=out), dict(out_eigenstrat=out, geno_format="transposed")):
        with pytest.raises(ValueError, match="^ld_compress goes with out_pfile: only a .pgen holds records that list their differences from an earlier record$"):
            convert(vcf, "9", ld_compress=True, **kw)
        assert listing(tmp_path) == before
    with pytest.raises(ValueError, match="name either out_prefix"):
        convert(vcf, "9", ld_compress=True)
    with pytest.raises(ValueError, match=r"out.pgen: --append does not go with --out-pfile"):
        convert(vcf, "9", out_pfile=out, ld_compress=True, append=True)
    assert listing(tmp_path) == before
    convert(vcf, "9", out_pfile=out, ld_compress=True)
    with pytest.raises(ValueError, match="out.pgen exists: name another prefix"):
        convert(vcf, "9", out_pfile=out, ld_compress=True)


# ---- the build and the command line ----


def test_units_header_and_binding():
    from sai_amd import _build
    from sai_amd.utils import pgen_writer

    device = [u for u in _build.UNITS if u not in _build.HOST_UNITS]
    assert "pgen/pgen_encode_ld.hip" in device and "pgen/pgen_encode_ld_host.cpp" in _build.HOST_UNITS
    header = _build.CSRC / "pgen" / "pgen_export_ld.hpp"
    assert header in _build.staleness_inputs() and _build.CSRC / "pgen" / "pgen_encode_device.hpp" in _build.staleness_inputs()
    assert not (_build.INCLUDE / "pgen_export_ld.hpp").exists()
    text = header.read_text()
    assert "#define SAI_PGEN_EXPORT_LD_VERSION 1\n" in text and "#define SAI_PGEN_LD_SEGMENT 16\n" in text
    for name in pgen_writer.LD_SIGNATURES:
        assert f" {name}(" in text, name
    plain = (_build.CSRC / "pgen" / "pgen_export.hpp").read_text()
    assert "#define SAI_PGEN_EXPORT_ABI_VERSION 1\n" in plain and not any(f" {name}(" in plain for name in pgen_writer.LD_SIGNATURES)
    assert not set(pgen_writer.LD_SIGNATURES) & set(pgen_writer.SIGNATURES)
    lib = pgen_writer.load_ld()
    assert lib.sai_pgen_export_ld_version() == 1 and lib.sai_pgen_export_abi_version() == 1 and all(hasattr(lib, name) for name in pgen_writer.LD_SIGNATURES)
    assert set(pgen_writer.LD_HOST_SYMBOLS) == {"sai_pgen_export_ld_version", "sai_pgen_ld_segment", "sai_pgen_encode_ld_host"}


def test_command_line(tmp_path, monkeypatch):
    from sai_amd.parsers.convert_parser import LD_NOTE, PGEN_NOTE

    res = sai_cli("convert", "--help")
    flat = " ".join(res.stdout.split())
    assert res.returncode == 0 and "--ld-compress" in flat and LD_NOTE in flat and PGEN_NOTE in LD_NOTE and "has not been opened with plink2" in LD_NOTE
    vcf, _ = panel_vcf(tmp_path, n_rows=60, n=30)
    prefix = str(tmp_path / "cli")
    monkeypatch.setenv("SAI_AMD_INGEST", "host")  # the child processes inherit it
    common = ("convert", "--vcf", vcf, "--chr-name", "9")
    before = listing(tmp_path)
    for other in (("--out-bfile", prefix), ("--out-eigenstrat", prefix), ()):
        res = sai_cli(*common, *other, "--ld-compress")
        assert res.returncode == 2 and "--ld-compress goes with --out-pfile: only a .pgen holds records" in res.stderr and listing(tmp_path) == before
    res = sai_cli(*common, "--out-pfile", prefix, "--ld-compress")
    assert res.returncode == 0, res.stderr[-2000:]
    summary = json.loads(res.stdout.splitlines()[-1])
    assert summary["rows_written"] == 60 and {"2", "3"} & set(summary["record_types"])
    from sai_amd.sai import convert

    api = convert(vcf, "9", out_pfile=str(tmp_path / "api"), ld_compress=True)
    assert fileset_bytes(prefix) == fileset_bytes(str(tmp_path / "api")) and {str(k): v for k, v in api["record_types"].items()} == summary["record_types"]
    res = sai_cli(*common, "--out-pfile", str(tmp_path / "plain"))
    assert res.returncode == 0 and "record_types" not in json.loads(res.stdout.splitlines()[-1])
