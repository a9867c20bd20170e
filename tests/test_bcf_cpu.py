"""BCF files on the host: the header and its dictionaries, the record walk, the row selection and the host decoder
of GT vectors, against the VCF reader on the VCF text the file was written from.  The files are written here by
tests/bcf_builder.py (pure Python, from the format rules alone); the expectation always comes from the VCF readers,
which the existing suites pin to the reference."""

import re
import subprocess

import numpy as np
import pytest

import abi_checks
import bcf_builder as B
import native_build
from conftest import DATA, GOLDEN, ROOT

# (name, chromosome, ancestral-allele file or None = one is written from the records)
FILES = [("example.vcf", "21", None), ("test.data.vcf", "21", "test.anc.allele.bed"),
         ("test.mixed.ploidy.data.vcf.gz", "21", "test.mixed.ploidy.data.anc.alleles"),
         ("test.with.outgroup.vcf.gz", "1", "test.with.outgroup.anc.alleles"), ("seeded", "7", None)]  # fmt: skip
# what the builder varies: bytes of a GT value, IDX= in the header, FORMAT fields around GT, member size, EOF member
SHAPES = [dict(width=1), dict(width=2, idx=True, extra_before=True, member_size=200, eof=False),
          dict(width=4, extra_after=True, member_size=977), dict(width=1, idx=True, extra_before=True, extra_after=True, member_size=200),
          dict(width=2, member_size=65280, eof=False), dict(width=4, idx=True, member_size=200)]  # fmt: skip


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def seeded_vcf(seed=11, n_samples=19, n_records=70) -> str:
    """Haploid, diploid and triploid calls mixed in one record, ``.``, ``./.``, ``.|1``, phased and unphased calls,
    multiallelic sites with allele 2 and 3, repeated positions, FORMAT with and without a field around GT, a
    chromosome before and one behind.  Only calls the VCF reader accepts."""
    rng = np.random.default_rng(seed)
    names = [f"s{k}" for k in range(n_samples)]
    lines = ["##fileformat=VCFv4.2", "##contig=<ID=3>", "##contig=<ID=7>", "##contig=<ID=9>",
             '##FILTER=<ID=q10,Description="Quality below 10, or so">', '##INFO=<ID=DP,Number=1,Type=Integer,Description="x">',
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q">',
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names)]  # fmt: skip
    special = [".", "./.", ".|1", "1|.", "0", "1", "0/1/2", "3|2|1", "2/3", "./././.", "1|1|1|1"]
    pos = 100
    for k in range(n_records):
        chrom = "3" if k < 4 else "9" if k >= n_records - 5 else "7"
        pos += int(rng.choice([0, 0, 1, 7, 300]))
        n_alt = int(rng.choice([1, 1, 2, 3]))
        alleles = list(rng.permutation(["A", "C", "G", "T"]))[: n_alt + 1]
        calls = []
        for _ in names:
            if rng.random() < 0.35:
                call = special[int(rng.integers(len(special)))]
                call = re.sub(r"\d", lambda m: str(min(int(m.group()), n_alt)), call)
            else:
                a = rng.integers(0, n_alt + 1, size=2)
                call = f"{a[0]}{'|' if rng.random() < 0.5 else '/'}{a[1]}"
            calls.append(call)
        fmt = ["GT", "GT:GQ", "GQ:GT"][k % 3]
        cells = [c if fmt == "GT" else f"{c}:{7 + k % 50}" if fmt == "GT:GQ" else f"{7 + k % 50}:{c}" for c in calls]
        alt = ",".join(alleles[1:]) if k % 17 else "."
        if alt == ".":
            cells = [re.sub(r"[1-9]", "0", c) if fmt != "GQ:GT" else c.split(":")[0] + ":" + re.sub(r"[1-9]", "0", c.split(":")[1]) for c in cells]
        lines.append("\t".join([chrom, str(pos), f"v{k}" if k % 3 else ".", alleles[0], alt, "50", ["PASS", ".", "q10"][k % 3], "DP=4", fmt] + cells))
    return "\n".join(lines) + "\n"


_text = {}


def vcf_text(name) -> str:
    if name not in _text:
        _text[name] = seeded_vcf() if name == "seeded" else B.read_vcf_text(DATA / name)
    return _text[name]


def vcf_path(name, tmp) -> str:
    """The source VCF as a file the VCF reader takes."""
    if name != "seeded":
        return str(DATA / name)
    path = tmp / "seeded.vcf"
    if not path.exists():
        path.write_text(vcf_text(name))
    return str(path)


def samples_of(name) -> list:
    return next(ln for ln in vcf_text(name).split("\n") if ln.startswith("#CHROM")).split("\t")[9:]


def records_of(name, chrom) -> list:
    return [ln.split("\t") for ln in vcf_text(name).split("\n") if ln and not ln.startswith("#") and ln.split("\t", 1)[0] == chrom]


def anc_file(name, chrom, given, tmp) -> str:
    """The ancestral alleles of the data directory, or a table that keeps, flips, drops and misses records."""
    if given is not None:
        return str(DATA / given)
    path = tmp / f"{name}.anc.bed"
    if not path.exists():
        rows = []
        for k, col in enumerate(records_of(name, chrom)):
            allele = [col[3], col[4].split(",")[0], col[4].split(",")[-1], "N", None][k % 5]
            if allele is not None:
                rows.append(f"{chrom}\t{int(col[1]) - 1}\t{col[1]}\t{allele}")
        path.write_text("\n".join(rows) + "\n")
    return str(path)


def region_of(name, chrom):
    pos = sorted({int(col[1]) for col in records_of(name, chrom)})
    return pos[1], pos[-2]


def small_buffer(name) -> int:
    """A staging buffer that holds a row or two, so that batches are cut between any two rows: 4 KiB, or 16 KiB for the
    1 513 samples of the outgroup file (a row of 4-byte values is 12 104 bytes)."""
    return 4096 if len(samples_of(name)) * 2 * 4 <= 4096 else 16384


def same(a, b) -> bool:
    return np.array_equal(a[0], b[0]) and a[1].dtype == b[1].dtype and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


@pytest.mark.parametrize("name,chrom,given_anc", FILES, ids=[f[0] for f in FILES])
def test_load_dosage_equals_the_vcf_reader(tmp_path, name, chrom, given_anc):
    """Positions, dosages, n_matched and n_anc for ploidy 1 to 4, with and without a region and ancestral alleles, for
    every shape the builder writes; every case is compared."""
    from sai_amd.utils import bcf, native_vcf

    text, samples, vcf = vcf_text(name), samples_of(name), vcf_path(name, tmp_path)
    anc, region = anc_file(name, chrom, given_anc, tmp_path), region_of(name, chrom)
    order = list(reversed(samples))[: max(1, len(samples) - 1)]  # not the file's order, not every sample
    asks = [(pl, reg, a) for pl in (1, 2, 3, 4) for reg in ((None, None), region) for a in (None, anc)]
    want = {ask: native_vcf.load_dosage(vcf, chrom, order, [ask[0]] * len(order), *ask[1], ask[2]) for ask in asks}
    assert any(len(w[0]) for w in want.values())
    compared = 0
    for k, shape in enumerate(SHAPES):
        path = B.write_bcf(tmp_path / f"{k}.bcf", text, **shape)
        for ask in asks:
            got = bcf.load_dosage(path, chrom, order, [ask[0]] * len(order), *ask[1], ask[2], buffer_bytes=[None, small_buffer(name)][k % 2])
            assert same(got, want[ask]), (name, shape, ask)
            compared += 1
    assert compared == len(SHAPES) * 16
    # mixed ploidies in one pass, a sample at two ploidies: every request is a slot
    mixed = [1 + k % 4 for k in range(len(samples))] + [3]
    got = bcf.load_dosage(path, chrom, samples + samples[:1], mixed, None, None, anc)
    for s, (nme, pl) in enumerate(zip(samples + samples[:1], mixed)):
        one = native_vcf.load_dosage(vcf, chrom, [nme], [pl], None, None, anc)
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1][:, s], one[1][:, 0]) and got[2:] == one[2:]


def test_the_seeded_file_holds_what_it_promises():
    calls = {c.split(":")[0] if ln[8].startswith("GT") else c.split(":")[-1] for ln in records_of("seeded", "7") for c in ln[9:]}
    assert {".", "./.", ".|1", "1|.", "0", "1", "0/1/2", "2/3", "./././."} <= calls and any("3" in c for c in calls)
    pos = [int(ln[1]) for ln in records_of("seeded", "7")]
    assert len(set(pos)) < len(pos) and any("," in ln[4] for ln in records_of("seeded", "7"))
    for ln in records_of("seeded", "7"):  # three calls of different length in one record, somewhere
        if len({len(re.split(r"[/|]", c.split(":")[0 if ln[8].startswith("GT") else -1])) for c in ln[9:]}) >= 3:
            break
    else:
        pytest.fail("no record mixes haploid, diploid and triploid calls")


def test_worked_example(tmp_path):
    """tests/golden/bcf_worked_example.hex: the inflated stream of 3 samples x 4 records, field by field; the builder
    reproduces it, the index and the host decoder read it."""
    from sai_amd.utils import bcf

    stream = bytes.fromhex("".join(ln.split("#")[0] for ln in (GOLDEN / "bcf_worked_example.hex").read_text().split("\n")))
    text = ("##fileformat=VCFv4.2\n##contig=<ID=5>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"g\">\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\tc\n"
            "5\t10\t.\tA\tC\t.\t.\t.\tGT\t0|1\t1/1\t./.\n"
            "5\t11\trs1\tG\tT,A\t.\tPASS\t.\tGT\t2|0\t0\t0/1/2\n"
            "5\t11\t.\tT\t.\t.\t.\t.\tGT\t0/0\t.\t0|0\n"
            "5\t40\t.\tC\tG\t.\t.\t.\tGT\t1|1\t0|1\t.|1\n")  # fmt: skip
    assert B.inflated_stream(text) == stream
    path = tmp_path / "worked.bcf"
    path.write_bytes(b"".join(B.bgzf_members(stream, member_size=64)))
    assert bcf.scan_first_last(path, "5") == (10, 40) and bcf.header_counts(path) == (4, 3)
    pos, dos, n_matched, n_anc = bcf.load_dosage(path, "5", ["a", "b", "c"], [2, 2, 2])
    assert pos.tolist() == [10, 11, 11, 40] and (n_matched, n_anc) == (4, 0)
    assert dos.tolist() == [[1, 2, -2], [2, -1, 1], [0, -2, 0], [2, 1, 0]]
    pos, dos, _, _ = bcf.load_dosage(path, "5", ["c", "a"], [3, 1], 11, 40)
    assert pos.tolist() == [11, 11, 40] and dos.tolist() == [[3, 2], [-1, 0], [-1, 1]]
    anc = tmp_path / "anc.bed"
    anc.write_text("5\t9\t10\tC\n5\t10\t11\tG\n5\t39\t40\tN\n")
    pos, dos, n_matched, n_anc = bcf.load_dosage(path, "5", ["a", "b", "c"], [2, 2, 2], anc_allele_file=str(anc))
    # 10: flipped; 11 (G): kept as it is; 11 (T, no ALT): neither allele; 40: neither allele
    assert pos.tolist() == [10, 11] and dos.tolist() == [[1, 0, 4], [2, -1, 1]] and (n_matched, n_anc) == (4, 3)


def small_bcf(tmp_path, name="small.bcf", **options) -> str:
    return B.write_bcf(tmp_path / name, vcf_text("example.vcf"), **options)


def test_dispatch(tmp_path, in_repo_root, monkeypatch):
    """reader_for and what hangs on it: scan_first_last, ChunkGenerator, chunks_for_memory, the CLI arguments of the ranks,
    read_dosage_data; the name of the file does not matter."""
    from sai_amd import sai as sai_mod
    from sai_amd.generators import ChunkGenerator
    from sai_amd.utils import bcf, filesets, pgen, plink, eigenstrat
    from sai_amd.utils.native_vcf import scan_first_last
    from sai_amd.utils.read_data import read_data, read_dosage_data

    vcf = "tests/data/example.vcf"
    path = small_bcf(tmp_path, "calls.vcf.gz", member_size=200)  # a misleading name
    assert filesets.READERS == (plink, eigenstrat, pgen) and filesets.FILE_READERS == (bcf,)
    assert filesets.reader_for(path) is bcf and filesets.reader_for(vcf) is None and bcf.fileset_prefix(path) == path
    assert filesets.name_of(path) == "a BCF file" and filesets.cli_source(path) == ["--vcf", path] and filesets.is_fileset(path)
    gz = tmp_path / "text.vcf.gz"
    gz.write_bytes(b"".join(B.bgzf_members(vcf_text("example.vcf").encode())))
    assert filesets.reader_for(str(gz)) is None and filesets.reader_for(str(tmp_path / "absent.bcf")) is None
    for chrom in ("21", "nope"):
        assert scan_first_last(path, chrom) == scan_first_last(vcf, chrom)
    a = ChunkGenerator(vcf_file=path, chr_name="21", window_size=3000, step_size=1000, num_chunks=3)
    b = ChunkGenerator(vcf_file=vcf, chr_name="21", window_size=3000, step_size=1000, num_chunks=3)
    assert a.chunks == b.chunks and a.windows == b.windows
    n_records, n_samples = len(records_of("example.vcf", "21")), len(samples_of("example.vcf"))
    assert filesets.resident_bytes(path) == n_records * n_samples
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", str(-(-n_records * n_samples // 3)))
    assert sai_mod.chunks_for_memory(path) == 3 and sai_mod._reads_in_one_pass(path) is False
    argv = sai_mod._score_cli_arguments(path, "21", 10, 5, None, "o.tsv", "c.yaml", 2)
    assert argv[:3] == ["score", "--vcf", path]
    cfg = sai_mod.load_config("tests/data/test_sai.config.yaml")
    lists = dict(ref_ind_file="tests/data/example.ref.ind.list", tgt_ind_file="tests/data/example.tgt.ind.list",
                 src_ind_file="tests/data/example.src.ind.list")  # fmt: skip
    got, want = (read_dosage_data(f, "21", cfg.ploidies, **lists) for f in (path, vcf))
    for group in ("ref", "tgt", "src"):
        assert got[group][1] == want[group][1] and set(got[group][0]) == set(want[group][0])
        for pop, block in want[group][0].items():
            assert got[group][0][pop].POS.tolist() == block.POS.tolist() and np.array_equal(got[group][0][pop].GT, block.GT)
    with pytest.raises(ValueError, match="a BCF file is read as unphased dosages only"):
        read_data(path, "21", cfg.ploidies, **lists)


def test_packed2_still_refuses_with_its_pinned_sentence(tmp_path, in_repo_root, monkeypatch):
    from sai_amd import sai as sai_mod

    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SAI_AMD_INGEST", "SAI_AMD_LAYOUT"):
        monkeypatch.delenv(name, raising=False)
    path = small_bcf(tmp_path, "calls.bcf")
    ask = dict(chr_name="21", win_len=100, win_step=50, anc_allele_file=None, output_file=str(tmp_path / "o" / "s.tsv"))
    with pytest.raises(ValueError, match=rf"^layout 'packed2' reads a PLINK 1 fileset \(.bed \+ .bim \+ .fam\) only, which {re.escape(path)} is not\.$"):
        sai_mod.score(vcf_file=path, config="tests/data/example.u_and_q.config.yaml", num_workers=1, layout="packed2", **ask)


def test_command_line_help_names_bcf():
    import sys

    res = subprocess.run([sys.executable, "-m", "sai_amd", "score", "--help"], cwd=str(ROOT), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "BCF" in res.stdout


def test_header_binding_and_library_agree_and_the_other_headers_are_untouched():
    from sai_amd import _build, _ffi, _ffi_bcf, _ffi_pgen

    names = abi_checks.declared_names("saihip_bcf.h")
    assert names == sorted(_ffi_bcf.SIGNATURES) and len(names) == 10
    lib = _ffi_bcf.load()
    version = abi_checks.header_macro("saihip_bcf.h", "SAI_BCF_ABI_VERSION")
    assert lib.sai_bcf_abi_version() == _ffi_bcf.SAI_BCF_ABI_VERSION == version == 1
    for name in ("SAI_BCF_STATUS_RANGE", "SAI_BCF_STATUS_BAD_VALUE", "SAI_BCF_STATUS_BAD_INDEX", "SAI_BCF_GT_ALIGN"):
        assert abi_checks.header_macro("saihip_bcf.h", name) == getattr(_ffi_bcf, name)
    assert lib.sai_bcf_decode(None, None, 0, 0, None, None, None, None, 1, 1, None, -1, None, 2, None, 0, None, None) == _ffi.SAI_ERR_ARG
    assert b"ctx is NULL" in lib.sai_last_error()
    assert lib.sai_abi_version() == _ffi.SAI_ABI_VERSION == 16 and lib.sai_pgen_abi_version() == _ffi_pgen.SAI_PGEN_ABI_VERSION == 1
    assert "bcf/bcf_decode.hip" in _build.UNITS and "bcf/bcf_index.cpp" in _build.HOST_UNITS
    assert ROOT / "include" / "saihip_bcf.h" in _build.PUBLIC_HEADERS and "csrc/bcf/*.hip" in abi_checks.package_data_patterns()


# ---- what is refused ------------------------------------------------------------------------------------


def _set(rec, **fields):
    rec.update(fields)


def _gt(rec):
    return next(f for f in rec["fmt"] if f["L"] == 2 and f["type"] in (B.INT8, B.INT16, B.INT32) and "payload" not in f)


def _break_crc(members):
    m = bytearray(members[1])
    m[-8] ^= 0x55
    return [members[0], bytes(m)] + members[2:]


def _break_deflate(members):
    m = bytearray(members[1])
    m[18:24] = b"\xff" * 6  # block type 3 and garbage
    return [members[0], bytes(m)] + members[2:]


def _no_gt_in_dictionary(stream):
    return stream.replace(b"##FORMAT=<ID=GT,", b"##FORMAT=<ID=GX,")


# (name, builder options, the sentence)
REFUSED = [
    ("raw", dict(raw=True), r"a raw \(uncompressed\) BCF is not read: compress it with bgzip"),
    ("bcf4", dict(magic=b"BCF\x04\x00"), r"BCF version 4\.0 is not read: only BCF 2\.2"),
    ("bcf21", dict(magic=b"BCF\x02\x01"), r"BCF version 2\.1 is not read: only BCF 2\.2"),
    ("l_text", dict(l_text=1 << 30), r"l_text of 1073741824 bytes lies beyond the end of the stream"),
    ("no_chrom_line", dict(drop_chrom_line=True), r"the BCF header has no #CHROM line"),
    ("no_gt_key", dict(on_stream=_no_gt_in_dictionary), r"the header declares no FORMAT field GT, but the genotypes of record 21:\d+ are asked for"),
    ("no_gt_entry", dict(on_record=lambda i, r: i == 2 and _set(r, fmt=[])), r"record 21:\d+ has no GT field"),
    ("chrom_index", dict(on_record=lambda i, r: i == 1 and _set(r, chrom=5)), r"record 2 has CHROM index 5, which no ##contig line of the header defines"),
    ("l_shared", dict(on_record=lambda i, r: i == 1 and _set(r, l_shared=23)), r"record 2 has l_shared = 23, fewer than the 24 bytes of its fixed fields"),
    ("record_leaves", dict(on_record=lambda i, r: i == 14 and _set(r, l_indiv=5000)), r"record 15 \(\d+ bytes\) leaves the stream"),
    ("typed_value_leaves", dict(on_record=lambda i, r: i == 3 and _set(r, l_indiv=1)), r"a typed value of the individual part leaves the record"),
    ("gt_leaves", dict(on_record=lambda i, r: i == 3 and _set(r, l_indiv=9)), r"the GT array \(22 bytes\) leaves the record"),
    ("gt_float", dict(on_record=lambda i, r: i == 3 and _set(_gt(r), type=B.FLOAT, values=[1.0] * 22)), r"the GT vector has type 5, not an integer type"),
    ("gt_char", dict(on_record=lambda i, r: i == 3 and _set(_gt(r), type=B.CHAR, payload=b"x" * 22)), r"the GT vector has type 7, not an integer type"),
    ("n_sample", dict(on_record=lambda i, r: i == 3 and _set(r, n_sample=10)), r"record 4 holds 10 samples but the header names 11"),
    ("crc", dict(member_size=300, on_members=_break_crc), r"BGZF block fails to inflate or its CRC"),
    ("deflate", dict(member_size=300, on_members=_break_deflate), r"BGZF block fails to inflate or its CRC"),
]  # fmt: skip


def damaged_files(tmp_path) -> list:
    return [(name, small_bcf(tmp_path, name + ".bcf", **options), sentence) for name, options, sentence in REFUSED]


def test_what_is_refused(tmp_path):
    from sai_amd.utils import bcf

    samples = samples_of("example.vcf")
    ask = dict(chr_name="21", samples=samples, ploidies=[2] * len(samples))
    for name, path, sentence in damaged_files(tmp_path):
        with pytest.raises(ValueError, match=re.escape(path) + ".*" + sentence):
            bcf.load_dosage(path, **ask)
    good = small_bcf(tmp_path)
    with pytest.raises(ValueError, match=rf"samples not found in {re.escape(good)}: nobody"):
        bcf.load_dosage(good, "21", ["ind1", "nobody"], [2, 2])
    for ploidy in (0, 65):
        with pytest.raises(ValueError, match=rf"ploidy {ploidy} of sample ind2 is outside 1 \.\. 64"):
            bcf.load_dosage(good, "21", ["ind1", "ind2"], [2, ploidy])
    with pytest.raises(ValueError, match=r"the staging buffer of 21 bytes is smaller than the GT array of record 21:\d+ \(22 bytes\): raise SAI_AMD_INGEST_BUFFER"):
        bcf.load_dosage(good, buffer_bytes=21, **ask)
    assert len(bcf.load_dosage(good, buffer_bytes=22, **ask)[0]) == len(records_of("example.vcf", "21"))
    # the scan refuses what the header and the record chain can tell
    for name, path, sentence in damaged_files(tmp_path):
        if name not in ("no_gt_key", "no_gt_entry", "typed_value_leaves", "gt_leaves", "gt_float", "gt_char"):
            with pytest.raises(ValueError, match=sentence):
                bcf.scan_first_last(path, "21")
    # values: a reserved one and one that leaves int8, by record and sample
    def values(width, v):
        return dict(width=width, on_record=lambda i, r: i == 4 and _gt(r)["values"].__setitem__(2 * 6 + 1, v))

    reserved = small_bcf(tmp_path, "reserved.bcf", **values(1, -126))
    with pytest.raises(ValueError, match=r"record 21:\d+: the GT vector of sample ind7 holds a reserved value: the record is damaged"):
        bcf.load_dosage(reserved, **ask)
    assert bcf.load_dosage(reserved, "21", samples, [1] * len(samples))[1].shape[0] > 4  # position 1 of ind7 is beyond ploidy 1
    wide = small_bcf(tmp_path, "wide.bcf", **values(2, (200 + 1) << 1))
    with pytest.raises(ValueError, match=r"dosage outside the int8 range at 21:\d+ \(sample ind7\)"):
        bcf.load_dosage(wide, **ask)


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------


@pytest.fixture(scope="module")
def dump_programs(tmp_path_factory):
    """tests/native/bcf_dump.cpp + the host units of libsaihip, once under ASan + UBSan with the runtimes linked in
    (as test_plink_cpu.py::dump_program builds its program) and once plain."""
    return native_build.dump_program("bcf_dump", tmp_path_factory, kinds=("san", "plain"))


def run_dump(exe, path, chrom, start, end, anc, request, cap=4096, n_threads=3):
    return native_build.run_native(exe, [path, chrom, -1 if start is None else start, -1 if end is None else end, anc or "-", n_threads, cap,
                                         *[f"{s}:{p}" for s, p in request]])  # fmt: skip


def test_host_code_is_clean_under_asan_ubsan(tmp_path, dump_programs):
    """The walk and the host decoder, run (not only compiled) under the sanitizers on the files above and on every
    damaged one: clean, the same bytes as the plain build, the same rows as the library."""
    from sai_amd.utils import bcf

    runs = 0
    for k, (name, chrom, given_anc) in enumerate(FILES):
        samples = samples_of(name)
        path = B.write_bcf(tmp_path / f"f{k}.bcf", vcf_text(name), **SHAPES[(k + 1) % len(SHAPES)])
        anc, region = anc_file(name, chrom, given_anc, tmp_path), region_of(name, chrom)
        request = [(s, 1 + j % 4) for j, s in enumerate(samples)]
        for a, (start, end) in ((None, (None, None)), (anc, region)):
            got = {kind: run_dump(exe, path, chrom, start, end, a, request, cap=small_buffer(name)) for kind, exe in dump_programs.items()}
            assert got["san"].returncode == 0, got["san"].stderr[-3000:]
            assert got["san"].stdout == got["plain"].stdout and got["plain"].returncode == 0
            lines = got["san"].stdout.split("\n")
            assert lines[0] == "probe 1" and lines[1].split()[:3] == ["scan", *map(str, bcf.scan_first_last(path, chrom))]
            want = bcf.load_dosage(path, chrom, [s for s, _ in request], [p for _, p in request], start, end, a)
            rows = [ln.split() for ln in lines[2:] if ln and not ln.startswith("counts")]
            assert [int(r[0]) for r in rows] == want[0].tolist() and all(r[4] == "0" for r in rows)
            assert np.array_equal(np.array([r[5:] for r in rows], dtype=np.int64).reshape(len(rows), len(request)), want[1])
            assert lines[-2] == f"counts {want[2]} {want[3]}"
            runs += 1
    samples = samples_of("example.vcf")
    for name, path, sentence in damaged_files(tmp_path):
        got = {kind: run_dump(exe, path, "21", None, None, None, [(s, 2) for s in samples]) for kind, exe in dump_programs.items()}
        assert got["san"].returncode == 3 and re.search(sentence, got["san"].stderr), (name, got["san"].returncode, got["san"].stderr[-2000:])
        assert (got["san"].stdout, got["san"].stderr) == (got["plain"].stdout, got["plain"].stderr) and got["plain"].returncode == 3
        runs += 1
    assert runs == 2 * len(FILES) + len(REFUSED)
