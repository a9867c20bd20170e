"""EIGENSOFT filesets on the host: the index of PREFIX.ind / PREFIX.snp, the three encodings of a .geno, the host
decoder and the dispatch of the readers, against the VCF route on the same genotypes.  The expectation always
comes from the VCF readers (pinned to the reference by the existing suites) or from a restatement inside this
file.  No EIGENSOFT program was at hand: the filesets are written here, from the format rules of
DESIGN_INGEST.md ("EIGENSTRAT filesets"), never read from a fixture."""

import os
import shutil

import numpy as np
import pytest

import abi_checks
import native_build
from conftest import ROOT
from test_plink_cpu import random_case, run_dump, sai_cli, vcf_expectation, write_vcf

ENCODINGS = ("text", "packed", "transposed")
MISSING = 3  # a genotype value g is 0, 1 or 2 copies of the first allele of the .snp line; 3 marks a missing call
G_OF_PLINK = np.array([0, 3, 1, 2], dtype=np.uint8)  # PLINK code (A1 A1, missing, het, A2 A2) -> g, with A2 first


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def pack_msb_first(g):
    """uint8 [records][calls] of 2-bit codes -> bytes [records][ceil(calls / 4)], the FIRST call of a byte in its two
    most significant bits; unused bits are 0."""
    g = np.asarray(g, dtype=np.uint8)
    padded = np.zeros((g.shape[0], -(-g.shape[1] // 4) * 4), dtype=np.uint8)
    padded[:, : g.shape[1]] = g
    q = padded.reshape(g.shape[0], -1, 4)
    return (q[:, :, 0] << 6 | q[:, :, 1] << 4 | q[:, :, 2] << 2 | q[:, :, 3]).astype(np.uint8)


def geno_bytes(encoding, g, hashes=True, newline="\n", final_newline=True):
    """The .geno of the matrix g = uint8 [variants][individuals]."""
    g = np.asarray(g, dtype=np.uint8)
    n_snp, n_ind = g.shape
    if encoding == "text":
        lines = ["".join("0129"[v] for v in row) for row in g]
        text = newline.join(lines) + (newline if final_newline and lines else "")
        return text.encode()
    transposed = encoding == "transposed"
    records = pack_msb_first(g.T if transposed else g)
    rlen = max(48, -(-(n_snp if transposed else n_ind) // 4))
    header = ("%s %7d %7d" % ("TGENO" if transposed else "GENO", n_ind, n_snp)) + (" %x %x" % (0x1A2B3C, 0xBEEF) if hashes else "")
    out = bytearray(header.encode().ljust(rlen, b"\0"))
    for rec in records:
        out += rec.tobytes().ljust(rlen, b"\0")
    return bytes(out)


def write_eigenstrat(prefix, encoding, chroms, positions, ids, ref, alt, g, samples, alleles=True, **kw):
    """g = uint8 [variants][samples] -> PREFIX.geno / .snp / .ind, the columns right-aligned as convertf writes
    them, with a comment and a blank line in the two text files."""
    g = np.asarray(g, dtype=np.uint8).reshape(len(positions), len(samples))
    with open(f"{prefix}.geno", "wb") as f:
        f.write(geno_bytes(encoding, g, **kw))
    with open(f"{prefix}.snp", "w") as f:
        f.write("# id chromosome genetic physical first second\n")
        for k in range(len(positions)):
            tail = f" {ref[k]} {alt[k]}" if alleles else ""
            sep = "\t" if k % 3 == 2 else " "
            f.write(f"{ids[k]:>20}{sep}{chroms[k]:>4}{sep}{k * 1e-6:>12.6f}{sep}{positions[k]:>15}{tail}\n")
            if k == 1:
                f.write("\n")
    with open(f"{prefix}.ind", "w") as f:
        for i, s in enumerate(samples):
            if i == 1:
                f.write("   # a comment\n\n")
            f.write(f"{s:>20} {'MFU'[i % 3]} {'Pop' + str(i % 4):>10}\n")
    return f"{prefix}.geno"


def eigenstrat_of_case(case, encoding, **kw):
    """The fileset of a ``random_case`` of test_plink_cpu in one of the three encodings: A2 of the .bim (REF in the
    VCF) is the first allele."""
    bim = [line.split() for line in open(case["prefix"] + ".bim")]
    prefix = f"{case['prefix']}_{encoding}"
    write_eigenstrat(prefix, encoding, [b[0] for b in bim], [int(b[3]) for b in bim], [b[1] for b in bim], [b[5] for b in bim],
                     [b[4] for b in bim], G_OF_PLINK[case["codes"]], case["samples"], **kw)  # fmt: skip
    return prefix


def eigenstrat_from_plink(bed_prefix, prefix, encoding, **kw):
    """A PLINK fileset written by test_plink_cpu, read back and written as an EIGENSOFT one (A2 first)."""
    bim = [line.split() for line in open(bed_prefix + ".bim")]
    fam = [line.split()[1] for line in open(bed_prefix + ".fam")]
    raw = np.frombuffer(open(bed_prefix + ".bed", "rb").read()[3:], dtype=np.uint8).reshape(len(bim), -1)
    codes = np.stack([(raw >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(len(bim), -1)[:, : len(fam)]
    write_eigenstrat(prefix, encoding, [b[0] for b in bim], [int(b[3]) for b in bim], [b[1] for b in bim], [b[5] for b in bim],
                     [b[4] for b in bim], G_OF_PLINK[codes], fam, **kw)  # fmt: skip
    return prefix


@pytest.mark.parametrize("seed", range(12))
def test_host_reader_equals_the_vcf_loader_on_random_matrices(tmp_path, seed):
    from sai_amd.utils import eigenstrat, filesets, plink

    case = random_case(seed, tmp_path)
    names, ploidies = [s for s, _ in case["request"]], [p for _, p in case["request"]]
    here = case["positions"]
    for encoding in ENCODINGS:
        prefix = eigenstrat_of_case(case, encoding, hashes=bool(seed % 2), newline="\r\n" if seed % 3 == 0 else "\n", final_newline=seed % 4 != 1)
        assert eigenstrat.is_fileset(prefix) and eigenstrat.fileset_prefix(prefix + ".geno") == prefix and not plink.is_fileset(prefix)
        assert filesets.reader_for(prefix) is eigenstrat and filesets.reader_for(case["prefix"]) is plink and filesets.reader_for(case["vcf"]) is None
        for anc in (None, case["anc"]):
            for start, end in [(None, None), (here[len(here) // 3], here[-2] + 1), (here[0] + 1, None)]:
                want = vcf_expectation(case, start, end, anc)
                for cap in (None, 160):  # 160 bytes: two or three records, or 16 bytes per individual
                    pos, dos, n_matched, n_anc = eigenstrat.load_dosage(prefix, "7", names, ploidies, start, end, anc, buffer_bytes=cap)
                    assert pos.dtype == np.int32 and dos.dtype == np.int8 and dos.shape == (len(pos), len(names))
                    assert pos.tolist() == want[0].tolist() and (n_matched, n_anc) == want[2:]
                    assert np.array_equal(dos, want[1]), (seed, encoding, start, end, anc, cap)
        assert eigenstrat.scan_first_last(prefix, "7") == plink.scan_first_last(case["prefix"], "7")
        assert eigenstrat.scan_first_last(prefix + ".geno", "nope") == (None, None)


def test_a_transposed_file_is_read_in_batches_that_end_inside_a_byte(tmp_path):
    """Many variants, few individuals, the smallest staging: batches of 61 variants, so the second one starts at code 1
    of its byte; with an ancestral-allele file the selected variants are sparse."""
    from sai_amd.utils import eigenstrat
    from sai_amd.utils.native_vcf import load_dosage

    rng = np.random.default_rng(5)
    n, samples = 700, ["a", "b", "c", "d", "e"]
    g = rng.integers(0, 4, size=(n, 5)).astype(np.uint8)
    positions = np.cumsum(rng.integers(1, 9, n)).tolist()
    kw = dict(chroms=["2"] * n, positions=positions, ids=[f"v{k}" for k in range(n)])
    plink_codes = np.array([0, 2, 3, 1], dtype=np.uint8)[g]  # g -> PLINK code, for the VCF writer of test_plink_cpu
    vcf = write_vcf(tmp_path / "long.vcf", a1=["T"] * n, a2=["G"] * n, codes=plink_codes, samples=samples, **kw)
    anc = tmp_path / "long.anc"
    anc.write_text("".join(f"2\t{p - 1}\t{p}\t{'GTA'[k % 3]}\n" for k, p in enumerate(positions) if k % 5))
    ask = (["e", "a", "c", "a"], [2, 2, 2, 2])
    for encoding in ENCODINGS:
        prefix = str(tmp_path / f"long_{encoding}")
        write_eigenstrat(prefix, encoding, ref=["G"] * n, alt=["T"] * n, g=g, samples=samples, **kw)
        for anc_file in (None, str(anc)):
            for start in (None, positions[333]):
                want = load_dosage(vcf, "2", ["e", "a", "c"], [2, 2, 2], start, None, anc_file)
                got = eigenstrat.load_dosage(prefix, "2", *ask, start, None, anc_file, buffer_bytes=48)
                assert got[0].tolist() == want[0].tolist() and got[2:] == want[2:] and len(got[0]) > 150
                assert np.array_equal(got[1], want[1][:, [0, 1, 2, 1]]), (encoding, anc_file, start)
    idx = eigenstrat._Index(eigenstrat._ffi_eigenstrat.load_host(), prefix, "2", *ask, positions[333], None, None, 2)
    batches = list(idx.batches(48))
    assert len(batches) > 5 and {b.first_code for b in batches} == {0, 1, 2, 3} and batches[0].n_batch == 61
    assert all(len(b.reads) == 3 for b in batches)  # one pread per DISTINCT individual


def small_fileset(tmp_path, encoding="packed", name="small", **kw):
    samples = ["a", "b", "c", "d", "e"]
    g = np.array([[0, 1, 2, MISSING, 0], [2, 2, 1, 0, MISSING], [1, 0, 0, 2, 2]])
    args = dict(chroms=["3", "3", "3"], positions=[100, 200, 300], ids=["v1", "v2", "v3"], ref=["T", "G", "A"], alt=["A", "C", "G"],
                g=g, samples=samples)  # fmt: skip
    args.update(kw)
    prefix = str(tmp_path / name)
    write_eigenstrat(prefix, encoding, **args)
    return prefix, args


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_the_table_row_by_row(tmp_path, encoding):
    """The dosage table of DESIGN_INGEST.md, restated: ploidy 2 and 1, kept and flipped rows, from bytes written by hand."""
    from sai_amd.utils import eigenstrat

    prefix, _ = small_fileset(tmp_path, encoding)
    # the three variants over the individuals a .. e: 0 1 2 - 0 / 2 2 1 0 - / 1 0 0 2 2
    if encoding == "text":
        raw = b"01290\n22109\n10022\n"
    elif encoding == "packed":  # 5 individuals: records of the 48-byte minimum, individual 0 in bits 7:6
        raw = b"GENO       5       3 ab cd".ljust(48, b"\0")
        for first, second in ((0b00011011, 0b00000000), (0b10100100, 0b11000000), (0b01000010, 0b10000000)):
            raw += bytes([first, second]).ljust(48, b"\0")
    else:  # one record per individual over the three variants
        raw = b"TGENO       5       3".ljust(48, b"\0")
        for byte in (0b00100100, 0b01100000, 0b10010000, 0b11001000, 0b00111000):
            raw += bytes([byte]).ljust(48, b"\0")
    with open(prefix + ".geno", "wb") as f:
        f.write(raw)
    pos, dos, n_matched, n_anc = eigenstrat.load_dosage(prefix, "3", ["a", "b", "c", "d"], [2, 2, 2, 2], start=100, end=100)
    assert pos.tolist() == [100] and dos.tolist() == [[2, 1, 0, -2]]  # 0b00011011: g = 0, 1, 2, missing
    pos, dos, n_matched, n_anc = eigenstrat.load_dosage(prefix, "3", ["e", "a", "d", "a"], [2, 2, 2, 2])
    assert pos.tolist() == [100, 200, 300] and (n_matched, n_anc) == (3, 0)
    assert dos.tolist() == [[2, 2, -2, 2], [-2, 0, 2, 0], [0, 1, 0, 1]]
    anc = tmp_path / "anc.bed"
    anc.write_text("3\t99\t100\tA\n3\t199\t200\tG\n3\t299\t300\tC\n9\t1\t2\tA\n")  # flip (second allele), keep, drop (neither)
    pos, dos, n_matched, n_anc = eigenstrat.load_dosage(prefix, "3", ["a", "b", "c", "d", "e"], [2] * 5, anc_allele_file=str(anc))
    assert pos.tolist() == [100, 200] and (n_matched, n_anc) == (3, 3)
    assert dos.tolist() == [[0, 1, 2, 4, 0], [0, 0, 1, 2, -2]]
    pos, dos, _, _ = eigenstrat.load_dosage(prefix, "3", ["d", "e", "a"], [1, 1, 1], start=100, end=100, anc_allele_file=str(anc))
    assert pos.tolist() == [100] and dos.tolist() == [[2, 0, 0]]  # flipped: missing 2, g = 0 counts 0
    pos, dos, _, _ = eigenstrat.load_dosage(prefix, "3", ["d", "e", "a"], [1, 1, 2], start=150, end=250)
    assert pos.tolist() == [200] and dos.tolist() == [[1, -1, 0]]


def test_the_writer_of_this_file_states_the_format(tmp_path):
    """The test-side writer against bytes written by hand: header, 48-byte minimum record, MSB-first order."""
    g = np.array([[0, 1, 2, MISSING, 0], [2, 2, 1, 0, MISSING], [1, 0, 0, 2, 2]])
    packed = geno_bytes("packed", g, hashes=False)
    assert len(packed) == 48 * 4 and packed[:20] == b"GENO       5       3" and packed[48:50] == bytes([0b00011011, 0])
    assert geno_bytes("packed", g)[:27] == b"GENO       5       3 1a2b3c"
    transposed = geno_bytes("transposed", g, hashes=False)
    assert len(transposed) == 48 * 6 and transposed[:6] == b"TGENO " and transposed[48] == 0b00100100 and transposed[48 * 4] == 0b11001000
    wide = geno_bytes("packed", np.zeros((2, 193), dtype=np.uint8))
    assert len(wide) == 49 * 3 and len(geno_bytes("packed", np.zeros((2, 191), dtype=np.uint8))) == 48 * 3
    assert geno_bytes("text", g) == b"01290\n22109\n10022\n" and geno_bytes("text", g, final_newline=False).endswith(b"2")


def test_refusals(tmp_path, in_repo_root):
    from sai_amd.sai import load_config
    from sai_amd.utils import eigenstrat, filesets
    from sai_amd.utils.native_vcf import load_dosage as vcf_load
    from sai_amd.utils.read_data import read_data, read_dosage_data

    prefix, args = small_fileset(tmp_path)
    ask = dict(chr_name="3", samples=["a", "b"], ploidies=[2, 2])
    assert eigenstrat.load_dosage(prefix, **ask)[1].tolist() == [[2, 1], [0, 0], [1, 2]]

    def broken(name, encoding="packed", **kw):
        bad, _ = small_fileset(tmp_path, encoding, name, **kw)
        return bad

    # none of the three encodings: the first bytes are named
    bad = broken("magic")
    with open(bad + ".geno", "r+b") as f:
        f.write(b"XENO")
    assert not eigenstrat.is_fileset(bad) and not filesets.is_fileset(bad)
    with pytest.raises(ValueError, match=r"magic.geno: not a .geno file: it starts with the bytes 58 45 4E 4F 20 "):
        eigenstrat.load_dosage(bad, **ask)
    # header counts against the line counts of .ind / .snp
    for encoding, tag in (("packed", b"GENO"), ("transposed", b"TGENO")):
        bad = broken("counts_" + encoding, encoding)
        with open(bad + ".geno", "r+b") as f:
            f.write(tag + b"       6       3")
        with pytest.raises(ValueError, match=r"the header counts 6 individuals and 3 variants, but the .ind has 5 lines and the .snp has 3"):
            eigenstrat.load_dosage(bad, **ask)
        bad = broken("header_" + encoding, encoding)
        with open(bad + ".geno", "r+b") as f:
            f.write(tag + b"       x       3")
        with pytest.raises(ValueError, match=f"malformed {tag.decode()} header"):
            eigenstrat.load_dosage(bad, **ask)
        # a wrong file size
        bad = broken("short_" + encoding, encoding)
        with open(bad + ".geno", "r+b") as f:
            f.truncate(48 * 3 + 7)
        records = 3 if encoding == "packed" else 5
        with pytest.raises(ValueError, match=rf"short_{encoding}.geno: 151 bytes, expected {48 * (1 + records)} \(a header and {records} records of 48 bytes\)"):
            eigenstrat.load_dosage(bad, **ask)
    bad = broken("short_text", "text")
    with open(bad + ".geno", "ab") as f:
        f.write(b"01290\n")
    with pytest.raises(ValueError, match=r"short_text.geno: 24 bytes, expected 18 \(3 variants of the .snp x lines of 6 bytes\)"):
        eigenstrat.load_dosage(bad, **ask)
    # text lines of unequal length, and a first line that does not fit the .ind
    bad = broken("ragged", "text")
    with open(bad + ".geno", "wb") as f:
        f.write(b"01290\n2210\n100220\n")
    with pytest.raises(ValueError, match=r"ragged.geno: lines of unequal length: line 2 does not end after 5 characters"):
        eigenstrat.load_dosage(bad, **ask)
    bad = broken("narrow", "text")
    with open(bad + ".geno", "wb") as f:
        f.write(b"0129\n2210\n1002\n")
    with pytest.raises(ValueError, match=r"narrow.geno: the first line holds 4 characters, but the .ind has 5 lines"):
        eigenstrat.load_dosage(bad, **ask)
    # an invalid character in a text .geno names the line
    bad = broken("letters", "text")
    with open(bad + ".geno", "wb") as f:
        f.write(b"01290\n2X109\n10022\n")
    with pytest.raises(ValueError, match=r"letters.geno: line 2 holds a character other than 0, 1, 2 and 9"):
        eigenstrat.load_dosage(bad, **ask)
    assert eigenstrat.load_dosage(bad, "3", ["a", "c"], [2, 2])[1].tolist() == [[2, 0], [0, 1], [1, 2]]  # only a requested column is read
    # a missing .snp / .ind
    for ext in (".snp", ".ind"):
        bad = broken("no" + ext[1:])
        os.remove(bad + ext)
        assert not eigenstrat.is_fileset(bad)
        with pytest.raises(ValueError, match=f"cannot open .*no{ext[1:]}\\{ext}"):
            eigenstrat.load_dosage(bad + ".geno", **ask)
    # an unknown sample: the VCF reader's words
    vcf = write_vcf(tmp_path / "small.vcf", a1=args["alt"], a2=args["ref"], codes=np.array([0, 2, 3, 1], dtype=np.uint8)[args["g"]],
                    **{k: args[k] for k in ("chroms", "positions", "ids", "samples")})  # fmt: skip
    with pytest.raises(ValueError) as from_vcf:
        vcf_load(vcf, "3", ["a", "zz"], [2, 2])
    with pytest.raises(ValueError) as from_set:
        eigenstrat.load_dosage(prefix, "3", ["a", "zz"], [2, 2])
    assert str(from_vcf.value) == f"samples not found in {vcf}: zz" and str(from_set.value) == f"samples not found in {prefix}.ind: zz"
    twice = broken("twice", samples=["a", "b", "c", "b", "e"])
    with pytest.raises(ValueError, match="sample b occurs twice in .*twice.ind"):
        eigenstrat.load_dosage(twice, **ask)
    assert eigenstrat.load_dosage(twice, "3", ["a", "c"], [2, 2])[1].tolist() == [[2, 0], [0, 1], [1, 2]]  # only a requested name matters
    # a .snp line with fewer than four columns, and a position that is no integer
    bad = broken("fewcols")
    with open(bad + ".snp", "a") as f:
        f.write("   v4 3 0.5\n")
    with pytest.raises(ValueError, match="fewcols.snp: variant line 4 has fewer than 4 columns"):
        eigenstrat.load_dosage(bad, **ask)
    bad = broken("badpos", positions=[100, "2e2", 300])
    with pytest.raises(ValueError, match="badpos.snp: variant line 2: the position is not an integer"):
        eigenstrat.load_dosage(bad, **ask)
    # --anc-alleles with a .snp that has no allele columns; without the file such a .snp is fine
    bare = broken("bare", alleles=False)
    assert eigenstrat.load_dosage(bare, **ask)[1].tolist() == [[2, 1], [0, 0], [1, 2]]
    anc = tmp_path / "anc.bed"
    anc.write_text("3\t99\t100\tA\n")
    with pytest.raises(ValueError, match="bare.snp: variant line 1 has no allele columns: an ancestral-allele file cannot be applied"):
        eigenstrat.load_dosage(bare, anc_allele_file=str(anc), **ask)
    # multi-character alleles are compared as strings
    multi = broken("multi", ref=["TA", "G", "A"], alt=["T", "C", "G"])
    anc.write_text("3\t99\t100\tT\n3\t199\t200\tGG\n")  # flip; neither -> dropped
    got = eigenstrat.load_dosage(multi, anc_allele_file=str(anc), **ask)
    assert got[0].tolist() == [100] and got[1].tolist() == [[0, 1]]
    # g = 1 at ploidy 1 names the variant and the sample, in all three encodings
    for encoding in ENCODINGS:
        p = broken("het_" + encoding, encoding)
        with pytest.raises(ValueError, match=r"heterozygous call .* of sample b at variant v1 .position 100., but the sample is configured with ploidy 1"):
            eigenstrat.load_dosage(p, "3", ["a", "b"], [1, 1])
        with pytest.raises(ValueError, match="of sample c at variant v2"):
            eigenstrat.load_dosage(p, "3", ["a", "c"], [2, 1], start=150)
    # ploidy above 2: refused before anything is read (the files of this one do not even exist)
    with pytest.raises(ValueError, match="sample b is configured with ploidy 4: an EIGENSTRAT fileset holds haploid and diploid calls only"):
        eigenstrat.load_dosage(str(tmp_path / "absent"), "3", ["a", "b"], [2, 4])
    # ... also through read_dosage_data, with the tetraploid fixture's configuration
    cfg = load_config("tests/data/test_mixed_ploidy.config.yaml")
    names = sorted({s for g in ("ref", "tgt", "src") for line in open(cfg.populations.get_population(g)) for s in line.split()[1:2]})
    tetra = broken("tetra", samples=names, g=np.full((3, len(names)), 2), chroms=["21"] * 3)
    kw = dict(chr_name="21", ploidy_config=cfg.ploidies, ref_ind_file=cfg.populations.get_population("ref"),
              tgt_ind_file=cfg.populations.get_population("tgt"), src_ind_file=cfg.populations.get_population("src"))  # fmt: skip
    with pytest.raises(ValueError, match="Failed to read VCF file .*tetra.geno from 21: sample .* is configured with ploidy 4"):
        read_dosage_data(vcf_file=tetra + ".geno", **kw)
    with pytest.raises(ValueError, match="an EIGENSTRAT fileset is read as unphased dosages only"):
        read_data(vcf_file=tetra + ".geno", **kw)
    # a buffer smaller than a record, or than one byte per requested individual
    with pytest.raises(ValueError, match=r"SAI_AMD_INGEST_BUFFER of 47 bytes is smaller than one row of .*small.geno .48 bytes."):
        eigenstrat.load_dosage(prefix, buffer_bytes=47, **ask)
    turned = broken("turned", "transposed")
    with pytest.raises(ValueError, match=r"SAI_AMD_INGEST_BUFFER of 1 bytes is smaller than one byte for each of the 2 requested individuals of .*turned.geno"):
        eigenstrat.load_dosage(turned, buffer_bytes=1, **ask)


def test_read_dosage_data_serves_such_a_fileset_like_its_vcf(in_repo_root, tmp_path):
    """Through the callers' one question (filesets.reader_for): read_dosage_data, scan_first_last and ChunkGenerator."""
    from test_plink_cpu import fileset_from_vcf

    from sai_amd.generators import ChunkGenerator
    from sai_amd.sai import load_config
    from sai_amd.utils.native_vcf import scan_first_last
    from sai_amd.utils.read_data import read_dosage_data

    vcf, chrom, cfgfile, anc = "tests/data/test.data.vcf", "21", "tests/data/test.uq.config.yaml", "tests/data/test.anc.allele.bed"
    bed = str(tmp_path / "fx")
    positions, chroms = fileset_from_vcf(vcf, bed)
    cfg = load_config(cfgfile)
    groups = dict(ref_ind_file=cfg.populations.get_population("ref"), tgt_ind_file=cfg.populations.get_population("tgt"),
                  src_ind_file=cfg.populations.get_population("src"), out_ind_file=cfg.populations.get_population("outgroup"))  # fmt: skip
    compared = 0
    for encoding in ENCODINGS:
        prefix = eigenstrat_from_plink(bed, str(tmp_path / encoding), encoding)
        for anc_file in (None, anc):
            kw = dict(chr_name=chrom, ploidy_config=cfg.ploidies, anc_allele_file=anc_file, **groups)
            want = read_dosage_data(vcf_file=vcf, **kw)
            for source in (prefix + ".geno", prefix):
                got = read_dosage_data(vcf_file=source, **kw)
                assert set(got) == set(want)
                for group in want:
                    assert got[group][1] == want[group][1] and (got[group][0] is None) == (want[group][0] is None)
                    for pop, block in (want[group][0] or {}).items():
                        mine = got[group][0][pop]
                        assert mine.POS.tolist() == block.POS.tolist() and mine.GT.dtype == np.int8 and np.array_equal(mine.GT, block.GT)
                        compared += 1
        for name in sorted(set(chroms)) + ["nope"]:
            assert scan_first_last(prefix + ".geno", name) == scan_first_last(vcf, name)
        a = ChunkGenerator(vcf_file=prefix + ".geno", chr_name=chrom, window_size=5000, step_size=2500, num_chunks=3)
        b = ChunkGenerator(vcf_file=vcf, chr_name=chrom, window_size=5000, step_size=2500, num_chunks=3)
        assert a.chunks == b.chunks and a.windows == b.windows
    assert compared >= 12
    # a bare prefix that has both kinds of files stays PLINK; with its extension it is what the extension says
    from sai_amd.utils import eigenstrat, filesets, plink

    for ext in (".geno", ".snp", ".ind"):
        shutil.copy(prefix + ext, bed + ext)
    assert filesets.reader_for(bed) is plink and filesets.reader_for(bed + ".bed") is plink and filesets.reader_for(bed + ".geno") is eigenstrat
    assert eigenstrat.fileset_prefix(bed) is None and eigenstrat.fileset_prefix(bed + ".geno") == bed


def test_one_pass_is_false_memory_estimate_and_rank_arguments(tmp_path, monkeypatch):
    from sai_amd import sai as sai_mod

    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "100")
    for encoding, geno_size, chunks in (("packed", 192, 8), ("transposed", 288, 12), ("text", 18, 1)):  # 4 x when packed, 1 x for text
        prefix, _ = small_fileset(tmp_path, encoding, "mem_" + encoding)
        assert os.path.getsize(prefix + ".geno") == geno_size
        assert sai_mod._reads_in_one_pass(prefix + ".geno") is False and sai_mod._reads_in_one_pass(prefix) is False
        assert sai_mod.chunks_for_memory(prefix + ".geno") == sai_mod.chunks_for_memory(prefix) == chunks
        argv = sai_mod._score_cli_arguments(prefix + ".geno", "3", 10, 5, None, "o.tsv", "c.yaml", 2)
        assert argv[:3] == ["score", "--eigenstrat", prefix] and "--vcf" not in argv and "--bfile" not in argv
    assert sai_mod._score_cli_arguments("x.vcf", "3", 10, 5, None, "o.tsv", "c.yaml", 2)[:3] == ["score", "--vcf", "x.vcf"]


def test_command_line(tmp_path):
    from test_plink_cpu import small_fileset as small_plink

    prefix, _ = small_fileset(tmp_path)
    bfile, _ = small_plink(tmp_path, "bed")
    res = sai_cli("score", "--help")
    assert res.returncode == 0 and "--eigenstrat PREFIX" in res.stdout and "--bfile PREFIX" in res.stdout and "--vcf VCF" in res.stdout
    rest = ["--chr-name", "3", "--output", str(tmp_path / "o.tsv"), "--config", "tests/data/test_sai.config.yaml"]
    # without --eigenstrat the usage error keeps its words; with it, all three flags are named
    res = sai_cli("score", *rest)
    assert res.returncode == 2 and "exactly one of the arguments --vcf and --bfile is required" in res.stderr
    res = sai_cli("score", "--vcf", "tests/data/example.vcf", "--bfile", bfile, *rest)
    assert res.returncode == 2 and "exactly one of the arguments --vcf and --bfile is required" in res.stderr
    for other in (["--vcf", "tests/data/example.vcf"], ["--bfile", bfile], ["--vcf", "tests/data/example.vcf", "--bfile", bfile]):
        res = sai_cli("score", "--eigenstrat", prefix, *other, *rest)
        assert res.returncode == 2 and "exactly one of the arguments --vcf, --bfile and --eigenstrat is required" in res.stderr
    os.remove(prefix + ".snp")
    res = sai_cli("score", "--eigenstrat", prefix, *rest)
    assert res.returncode == 2 and f"{prefix}.snp is not found" in res.stderr
    assert not (tmp_path / "o.tsv").exists()


def test_header_and_binding_agree():
    """include/saihip_eigenstrat.h, sai_amd/_ffi_eigenstrat.py and the library name the same entry points; the two
    earlier headers and their versions are as they were."""
    from sai_amd import _ffi, _ffi_eigenstrat, _ffi_plink

    names = abi_checks.declared_names("saihip_eigenstrat.h")
    assert names == sorted(_ffi_eigenstrat.SIGNATURES) and len(names) == 9 and all(n.startswith("sai_eigenstrat_") for n in names)
    lib = _ffi_eigenstrat.load()
    version = abi_checks.header_macro("saihip_eigenstrat.h", "SAI_EIGENSTRAT_ABI_VERSION")
    assert lib.sai_eigenstrat_abi_version() == _ffi_eigenstrat.SAI_EIGENSTRAT_ABI_VERSION == version == 1
    for name, value in (("STATUS_BAD_INDEX", _ffi_eigenstrat.SAI_EIGENSTRAT_STATUS_BAD_INDEX), ("STATUS_BAD_CHAR", _ffi_eigenstrat.SAI_EIGENSTRAT_STATUS_BAD_CHAR),
                        ("TEXT", _ffi_eigenstrat.TEXT), ("PACKED", _ffi_eigenstrat.PACKED), ("TRANSPOSED", _ffi_eigenstrat.TRANSPOSED)):  # fmt: skip
        assert abi_checks.header_macro("saihip_eigenstrat.h", f"SAI_EIGENSTRAT_{name}") == value
    assert lib.sai_abi_version() == _ffi.SAI_ABI_VERSION == 16 and _ffi_plink.load().sai_plink_abi_version() == 1
    assert not any(n.startswith("sai_eigenstrat") for n in list(_ffi.SIGNATURES) + list(_ffi_plink.SIGNATURES))
    assert len(abi_checks.declared_names("saihip_plink.h")) == 8 and "eigenstrat" not in abi_checks.header_text("saihip_plink.h")
    assert "eigenstrat" not in (ROOT / "include" / "saihip.h").read_text().lower()
    assert lib.sai_eigenstrat_decode(None, 2, None, 0, 0, 0, None, None, 0, 1, None, -1, None, 0, None, 0, None, None) == _ffi.SAI_ERR_ARG
    assert b"ctx is NULL" in lib.sai_last_error()
    assert lib.sai_eigenstrat_decode_transposed(None, None, 0, 0, 0, 0, 0, None, None, 1, None, None, None, 0, None, None) == _ffi.SAI_ERR_ARG
    assert b"ctx is NULL" in lib.sai_last_error()


@pytest.fixture(scope="module")
def dump_program(tmp_path_factory):
    """tests/native/eigenstrat_dump.cpp + the host units of libsaihip under ASan + UBSan, the runtimes linked in."""
    return native_build.dump_program("eigenstrat_dump", tmp_path_factory)["san"]


def test_host_code_is_clean_under_asan_ubsan(tmp_path, dump_program):
    """The index and the host decoder of all three encodings, run (not only compiled) under the sanitizers on the
    filesets of the random cases: same positions, rows, flips and dosages as the library."""
    from sai_amd.utils import eigenstrat

    layout = {"text": 1, "packed": 2, "transposed": 3}
    for seed in (1, 2, 5):
        case = random_case(seed, tmp_path)
        here = case["positions"]
        names, ploidies = [s for s, _ in case["request"]], [p for _, p in case["request"]]
        for encoding in ENCODINGS:
            prefix = eigenstrat_of_case(case, encoding, final_newline=seed != 2)
            for anc in (None, case["anc"]):
                for start, end in [(None, None), (here[1], here[-1] - 1)]:
                    res = run_dump(dump_program, prefix, "7", start, end, anc, case["request"])
                    assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
                    lines = res.stdout.splitlines()
                    pos, dos, n_matched, n_anc = eigenstrat.load_dosage(prefix, "7", names, ploidies, start, end, anc)
                    first, last = eigenstrat.scan_first_last(prefix, "7")
                    assert lines[0].split()[:7] == ["info", str(len(pos)), str(n_matched), str(n_anc), str(first), str(last), str(layout[encoding])]
                    table = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], dtype=np.int64).reshape(len(pos), 4 + len(names))
                    assert table[:, 0].tolist() == pos.tolist() and not table[:, 3].any()
                    assert np.array_equal(table[:, 4:], dos)
    # refusals come back as a status and a message, also there
    res = run_dump(dump_program, prefix, "7", None, None, None, [("nobody", 2)])
    assert res.returncode == 3 and "samples not found" in res.stderr and "Sanitizer" not in res.stderr
    res = run_dump(dump_program, str(tmp_path / "absent"), "7", None, None, None, [("s0", 2)])
    assert res.returncode == 3 and "cannot open" in res.stderr and "Sanitizer" not in res.stderr
    with open(prefix + ".geno", "r+b") as f:
        f.truncate(100)
    res = run_dump(dump_program, prefix, "7", None, None, None, [("s0", 2)])
    assert res.returncode == 3 and "100 bytes, expected" in res.stderr and "Sanitizer" not in res.stderr
