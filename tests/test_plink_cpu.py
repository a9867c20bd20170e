"""PLINK 1 filesets on the host: the index of PREFIX.fam / PREFIX.bim, the host decoder of .bed rows and the
dispatch of the readers, against the VCF route on the same genotypes.  The expectation always comes from
the VCF readers (pinned to the reference by the existing suites) or from a restatement inside this file;
the filesets are written here, by a converter of a dozen lines, never read from a fixture."""

import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_checks
import native_build
from conftest import ROOT

# PLINK 1 codes (bits 1:0 of a sample's pair): 0 = A1 A1, 1 = missing, 2 = heterozygous, 3 = A2 A2
HOM_A1, MISSING, HET, HOM_A2 = 0, 1, 2, 3


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


def write_fileset(prefix, chroms, positions, ids, a1, a2, codes, samples, magic=b"\x6c\x1b\x01"):
    """codes = uint8 [variants][samples] of PLINK codes -> PREFIX.bed / .bim / .fam."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(len(positions), len(samples))
    padded = np.zeros((codes.shape[0], -(-codes.shape[1] // 4) * 4), dtype=np.uint8)
    padded[:, : codes.shape[1]] = codes
    quads = padded.reshape(codes.shape[0], -1, 4)
    rows = quads[:, :, 0] | quads[:, :, 1] << 2 | quads[:, :, 2] << 4 | quads[:, :, 3] << 6
    with open(f"{prefix}.bed", "wb") as f:
        f.write(magic + rows.astype(np.uint8).tobytes())
    with open(f"{prefix}.bim", "w") as f:
        for k in range(len(positions)):
            sep = "\t" if k % 2 else " "  # blanks and tabs are both separators
            f.write(sep.join([str(chroms[k]), str(ids[k]), "0", str(positions[k]), a1[k], a2[k]]) + "\n")
    with open(f"{prefix}.fam", "w") as f:
        for s in samples:
            f.write(f"fam_{s} {s} 0 0 0 -9\n")
    return f"{prefix}.bed"


def write_vcf(path, chroms, positions, ids, a1, a2, codes, samples, haploid=()):
    """The same calls as VCF text: REF = A2, ALT = A1; a sample in ``haploid`` is written as one allele."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(len(positions), len(samples))
    dip = {HOM_A1: "1|1", MISSING: ".|.", HET: "0|1", HOM_A2: "0|0"}
    hap = {HOM_A1: "1", MISSING: ".", HOM_A2: "0"}
    hap_cols = {samples.index(s) for s in haploid}
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")
        for k in range(len(positions)):
            calls = [(hap if c in hap_cols else dip)[int(codes[k, c])] for c in range(len(samples))]
            f.write("\t".join([str(chroms[k]), str(positions[k]), str(ids[k]), a2[k], a1[k], ".", "PASS", ".", "GT", *calls]) + "\n")
    return str(path)


def fileset_from_vcf(vcf, prefix):
    """A fixture VCF (biallelic, diploid, no half-missing call) as a fileset; refuses anything else."""
    opener = gzip.open if str(vcf).endswith(".gz") else open
    chroms, positions, ids, a1, a2, rows, samples = [], [], [], [], [], [], None
    of_call = {("0", "0"): HOM_A2, ("1", "1"): HOM_A1, ("0", "1"): HET, ("1", "0"): HET, (".", "."): MISSING}
    with opener(vcf, "rt") as f:
        for line in f:
            if line.startswith("##"):
                continue
            fields = line.rstrip("\n").split("\t")
            if line.startswith("#CHROM"):
                samples = fields[9:]
                continue
            assert "," not in fields[4] and fields[8].split(":")[0] == "GT"
            chroms.append(fields[0]), positions.append(int(fields[1])), ids.append(fields[2] if fields[2] != "." else f"v{len(ids)}")
            a2.append(fields[3]), a1.append(fields[4])
            rows.append([of_call[tuple(c.split(":")[0].replace("/", "|").split("|"))] for c in fields[9:]])
    write_fileset(prefix, chroms, positions, ids, a1, a2, np.array(rows, dtype=np.uint8), samples)
    return np.array(positions), chroms


FIXTURES = [
    ("tests/data/example.vcf", "21", "tests/data/example.u_and_q.config.yaml", None),
    ("tests/data/test.data.vcf", "21", "tests/data/test.uq.config.yaml", "tests/data/test.anc.allele.bed"),
    ("tests/data/test.with.outgroup.vcf.gz", "1", "tests/data/test.with.outgroup.config.yaml", "tests/data/test.with.outgroup.anc.alleles"),
]  # fmt: skip


def regions_of(pos):
    """Whole chromosome, and regions whose bounds fall on, between and outside positions."""
    pos = np.unique(pos)
    mid = len(pos) // 2
    out = [(None, None), (int(pos[1]), int(pos[-2])), (int(pos[0]) - 5, int(pos[-1]) + 5), (int(pos[-1]) + 1, int(pos[-1]) + 10)]
    if pos[mid] + 1 < pos[mid + 1]:
        out.append((int(pos[1]) + 1, int(pos[mid]) + 1))
    out.append((int(pos[mid]), None))
    out.append((None, int(pos[mid])))
    return out


@pytest.mark.parametrize("vcf,chrom,cfgfile,anc", FIXTURES)
def test_fixture_filesets_read_like_their_vcf(in_repo_root, tmp_path, vcf, chrom, cfgfile, anc):
    from sai_amd.generators import ChunkGenerator
    from sai_amd.sai import load_config
    from sai_amd.utils import plink
    from sai_amd.utils.native_vcf import scan_first_last
    from sai_amd.utils.read_data import read_dosage_data

    prefix = str(tmp_path / "fx")
    positions, chroms = fileset_from_vcf(vcf, prefix)
    assert plink.is_fileset(prefix) and plink.is_fileset(prefix + ".bed") and not plink.is_fileset(vcf)
    if anc:
        assert not plink.is_fileset(anc)  # a .bed of ancestral alleles is not a fileset
    cfg = load_config(cfgfile)
    groups = dict(ref_ind_file=cfg.populations.get_population("ref"), tgt_ind_file=cfg.populations.get_population("tgt"),
                  src_ind_file=cfg.populations.get_population("src"), out_ind_file=cfg.populations.get_population("outgroup"))  # fmt: skip
    here = positions[np.array(chroms) == chrom]
    compared = 0
    for anc_file in ([None, anc] if anc else [None]):
        for start, end in regions_of(here):
            kw = dict(chr_name=chrom, ploidy_config=cfg.ploidies, anc_allele_file=anc_file, start=start, end=end, **groups)
            try:
                want = read_dosage_data(vcf_file=vcf, **kw)
            except ValueError as exc:  # "No ancestral allele is found ...": the fileset must say the same
                with pytest.raises(ValueError) as got_exc:
                    read_dosage_data(vcf_file=prefix + ".bed", **kw)
                assert str(got_exc.value) == str(exc) and "No ancestral allele" in str(exc)
                continue
            for source in (prefix + ".bed", prefix):
                got = read_dosage_data(vcf_file=source, **kw)
                assert set(got) == set(want)
                for group in want:
                    assert got[group][1] == want[group][1]
                    assert (got[group][0] is None) == (want[group][0] is None), (group, start, end)
                    for pop, block in (want[group][0] or {}).items():
                        mine = got[group][0][pop]
                        assert mine.POS.dtype == block.POS.dtype and mine.POS.tolist() == block.POS.tolist()
                        assert mine.GT.dtype == block.GT.dtype == np.int8 and np.array_equal(mine.GT, block.GT)
                        compared += 1
    assert compared >= 6
    for name in sorted(set(chroms)) + ["nope"]:
        assert scan_first_last(prefix + ".bed", name) == scan_first_last(vcf, name) == plink.scan_first_last(prefix, name)
    for n_chunks in (1, 3):
        a = ChunkGenerator(vcf_file=prefix + ".bed", chr_name=chrom, window_size=5000, step_size=2500, num_chunks=n_chunks)
        b = ChunkGenerator(vcf_file=vcf, chr_name=chrom, window_size=5000, step_size=2500, num_chunks=n_chunks)
        assert a.chunks == b.chunks and a.windows == b.windows
    with pytest.raises(ValueError, match="Chromosome nope not found in VCF"):
        ChunkGenerator(vcf_file=prefix, chr_name="nope", window_size=5000, step_size=2500, num_chunks=1)


def random_case(seed, tmp_path):
    """A seeded matrix with decoy chromosomes around chromosome 7, written both ways, plus an ancestral-allele
    file that keeps, flips, drops and omits sites."""
    os.makedirs(tmp_path, exist_ok=True)
    rng = np.random.default_rng(seed)
    n_samples = int(rng.integers(1, 71))
    samples = [f"s{i}" for i in range(n_samples)]
    n_before, n_here, n_after = (int(rng.integers(0, 6)), int(rng.integers(5, 60)), int(rng.integers(0, 6)))
    chroms = ["6"] * n_before + ["7"] * n_here + ["77"] * n_after
    positions = np.concatenate([np.cumsum(rng.integers(1, 400, n)) for n in (n_before, n_here, n_after)]).tolist()
    n = len(chroms)
    letters = np.array(list("ACGT"))
    pick = np.array([rng.permutation(4)[:3] for _ in range(n)])
    a1, a2, other = (letters[pick[:, k]].tolist() for k in range(3))
    missing_rate = float(rng.uniform(0, 0.3))
    codes = rng.choice([HOM_A1, HET, HOM_A2], size=(n, n_samples)).astype(np.uint8)
    codes[rng.random(codes.shape) < missing_rate] = MISSING
    haploid = [s for s in samples if rng.random() < 0.4]
    both = samples[int(rng.integers(n_samples))]  # read at ploidy 1 AND 2: diploid in the VCF, never heterozygous
    if both in haploid:
        haploid.remove(both)
    for s in haploid + [both]:
        col = samples.index(s)
        het = codes[:, col] == HET
        codes[het, col] = rng.choice([HOM_A1, HOM_A2], size=int(het.sum()))
    ids = [f"rs{seed}_{k}" for k in range(n)]
    prefix = str(tmp_path / f"r{seed}")
    write_fileset(prefix, chroms, positions, ids, a1, a2, codes, samples)
    vcf = write_vcf(tmp_path / f"r{seed}.vcf", chroms, positions, ids, a1, a2, codes, samples, haploid)
    anc = tmp_path / f"r{seed}.anc.bed"
    fate = rng.choice(["keep", "flip", "drop", "omit"], size=n)
    with open(anc, "w") as f:
        for k in range(n):
            if fate[k] != "omit":
                allele = {"keep": a2[k], "flip": a1[k], "drop": other[k]}[fate[k]]
                f.write(f"{chroms[k]}\t{positions[k] - 1}\t{positions[k]}\t{allele}\n")
    # the request: a population list in non-file order, `both` at its two ploidies
    order = [samples[i] for i in rng.permutation(n_samples)]
    request = [(s, 1 if s in haploid else 2) for s in order]
    request.insert(int(rng.integers(len(request) + 1)), (both, 1))
    here = [p for c, p in zip(chroms, positions) if c == "7"]
    return dict(prefix=prefix, vcf=vcf, anc=str(anc), request=request, both=both, positions=here, codes=codes, samples=samples,
                chroms=chroms, fate=fate)  # fmt: skip


def vcf_expectation(case, start, end, anc):
    """What the VCF loader gives for the request; `both` at ploidy 1 comes from a call of its own (a VCF pass
    takes a sample once)."""
    from sai_amd.utils.native_vcf import load_dosage

    request = case["request"]
    second = request.index((case["both"], 1))
    rest = [r for i, r in enumerate(request) if i != second]
    pos, dos, n_matched, n_anc = load_dosage(case["vcf"], "7", [s for s, _ in rest], [p for _, p in rest], start, end, anc)
    pos1, dos1, _, _ = load_dosage(case["vcf"], "7", [case["both"]], [1], start, end, anc)
    assert pos1.tolist() == pos.tolist()
    return pos, np.insert(dos, second, dos1[:, 0], axis=1), n_matched, n_anc


@pytest.mark.parametrize("seed", range(24))
def test_host_decode_equals_the_vcf_loader_on_random_matrices(tmp_path, seed):
    from sai_amd.utils import plink

    case = random_case(seed, tmp_path)
    names, ploidies = [s for s, _ in case["request"]], [p for _, p in case["request"]]
    here = case["positions"]
    for anc in (None, case["anc"]):
        for start, end in [(None, None), (here[len(here) // 3], here[-2] + 1), (here[0] + 1, None)]:
            want = vcf_expectation(case, start, end, anc)
            for cap in (None, 64):  # 64 bytes: a few rows per batch
                pos, dos, n_matched, n_anc = plink.load_dosage(case["prefix"], "7", names, ploidies, start, end, anc, buffer_bytes=cap)
                assert pos.dtype == np.int32 and dos.dtype == np.int8 and dos.shape == (len(pos), len(names))
                assert pos.tolist() == want[0].tolist() and (n_matched, n_anc) == want[2:]
                assert np.array_equal(dos, want[1]), (seed, start, end, anc)
    if seed == 0:  # every cell of the table was reached, "missing and flipped" at both ploidies included
        seen = set()
        for s in range(24):
            c = random_case(s, tmp_path / "again") if s else case
            cols = {name: c["samples"].index(name) for name, _ in c["request"]}
            on7 = np.array(c["chroms"]) == "7"
            for name, ploidy in c["request"]:
                for fate in ("keep", "flip"):
                    rows = on7 & (c["fate"] == fate)
                    seen |= {(ploidy, fate, int(v)) for v in np.unique(c["codes"][rows, cols[name]])}
        assert {(2, f, v) for f in ("keep", "flip") for v in range(4)} | {(1, f, v) for f in ("keep", "flip") for v in (0, 1, 3)} <= seen


@pytest.fixture(scope="module")
def dump_program(tmp_path_factory):
    """tests/native/plink_dump.cpp + the host units of libsaihip under ASan + UBSan, the runtimes linked in."""
    return native_build.dump_program("plink_dump", tmp_path_factory)["san"]


def run_dump(exe, prefix, chrom, start, end, anc, request, n_threads=3):
    return native_build.run_native(exe, [prefix, chrom, -1 if start is None else start, -1 if end is None else end, anc or "-", n_threads,
                                         *[f"{s}:{p}" for s, p in request]])  # fmt: skip


def test_host_code_is_clean_under_asan_ubsan(tmp_path, dump_program):
    """The index and the host decoder, run (not only compiled) under the sanitizers on the filesets of the
    random cases: same positions, rows, flips and dosages as the library."""
    from sai_amd.utils import plink

    for seed in (1, 2, 3, 5, 8):
        case = random_case(seed, tmp_path)
        here = case["positions"]
        for anc in (None, case["anc"]):
            for start, end in [(None, None), (here[1], here[-1] - 1)]:
                res = run_dump(dump_program, case["prefix"], "7", start, end, anc, case["request"])
                assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-3000:]
                lines = res.stdout.splitlines()
                names, ploidies = [s for s, _ in case["request"]], [p for _, p in case["request"]]
                pos, dos, n_matched, n_anc = plink.load_dosage(case["prefix"], "7", names, ploidies, start, end, anc)
                first, last = plink.scan_first_last(case["prefix"], "7")
                assert lines[0].split() == ["info", str(len(pos)), str(n_matched), str(n_anc), str(first), str(last)]
                table = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], dtype=np.int64).reshape(len(pos), 4 + len(names))
                assert table[:, 0].tolist() == pos.tolist() and not table[:, 3].any()
                assert np.array_equal(table[:, 4:], dos)
    # refusals come back as a status and a message, also there
    case = random_case(1, tmp_path)
    res = run_dump(dump_program, case["prefix"], "7", None, None, None, [("nobody", 2)])
    assert res.returncode == 3 and "samples not found" in res.stderr and "Sanitizer" not in res.stderr
    res = run_dump(dump_program, str(tmp_path / "absent"), "7", None, None, None, [("s0", 2)])
    assert res.returncode == 3 and "cannot open" in res.stderr and "Sanitizer" not in res.stderr


def small_fileset(tmp_path, name="small", **kw):
    samples = ["a", "b", "c", "d", "e"]
    codes = np.array([[HOM_A1, HET, HOM_A2, MISSING, HOM_A1], [HOM_A2, HOM_A2, HET, HOM_A1, MISSING], [HET, HOM_A1, HOM_A1, HOM_A2, HOM_A2]])
    args = dict(chroms=["3", "3", "3"], positions=[100, 200, 300], ids=["v1", "v2", "v3"], a1=["A", "C", "G"], a2=["T", "G", "A"],
                codes=codes, samples=samples)  # fmt: skip
    args.update(kw)
    prefix = str(tmp_path / name)
    write_fileset(prefix, **args)
    return prefix, args


def test_the_table_row_by_row(tmp_path):
    """The dosage table of DESIGN_INGEST.md, restated: ploidy 2 and 1, kept and flipped rows."""
    from sai_amd.utils import plink

    prefix, args = small_fileset(tmp_path)
    pos, dos, n_matched, n_anc = plink.load_dosage(prefix, "3", ["e", "a", "d", "a"], [2, 2, 2, 2])
    assert pos.tolist() == [100, 200, 300] and (n_matched, n_anc) == (3, 0)
    assert dos.tolist() == [[2, 2, -2, 2], [-2, 0, 2, 0], [0, 1, 0, 1]]
    anc = tmp_path / "anc.bed"
    anc.write_text("3\t99\t100\tA\n3\t199\t200\tG\n3\t299\t300\tC\n9\t1\t2\tA\n")  # flip, keep, drop (neither allele)
    pos, dos, n_matched, n_anc = plink.load_dosage(prefix, "3", ["a", "b", "c", "d", "e"], [2] * 5, anc_allele_file=str(anc))
    assert pos.tolist() == [100, 200] and (n_matched, n_anc) == (3, 3)
    assert dos.tolist() == [[0, 1, 2, 4, 0], [0, 0, 1, 2, -2]]
    pos, dos, _, _ = plink.load_dosage(prefix, "3", ["d", "e", "a"], [1, 1, 1], start=100, end=100, anc_allele_file=str(anc))
    assert pos.tolist() == [100] and dos.tolist() == [[2, 0, 0]]  # flipped: missing 2, A1 A1 0
    pos, dos, _, _ = plink.load_dosage(prefix, "3", ["d", "e", "a"], [1, 1, 2], start=150, end=250)
    assert pos.tolist() == [200] and dos.tolist() == [[1, -1, 0]]


def test_refusals(tmp_path, in_repo_root):
    from sai_amd.sai import load_config
    from sai_amd.utils import plink
    from sai_amd.utils.native_vcf import load_dosage as vcf_load
    from sai_amd.utils.read_data import read_data, read_dosage_data

    prefix, args = small_fileset(tmp_path)
    ask = dict(chr_name="3", samples=["a", "b"], ploidies=[2, 2])
    bad, _ = small_fileset(tmp_path, "magic", magic=b"\x6c\x1c\x01")
    assert not plink.is_fileset(bad)
    with pytest.raises(ValueError, match="not a PLINK 1 .bed file"):
        plink.load_dosage(bad, **ask)
    bad, _ = small_fileset(tmp_path, "third", magic=b"\x6c\x1b\x02")
    with pytest.raises(ValueError, match="not a PLINK 1 .bed file .third byte 02"):
        plink.load_dosage(bad, **ask)
    bad, _ = small_fileset(tmp_path, "major", magic=b"\x6c\x1b\x00")
    assert plink.is_fileset(bad)
    with pytest.raises(ValueError, match="sample-major .bed files are not supported"):
        plink.load_dosage(bad + ".bed", **ask)
    bad, _ = small_fileset(tmp_path, "short")
    with open(bad + ".bed", "r+b") as f:
        f.truncate(3 + 2 * 2 + 1)
    with pytest.raises(ValueError, match=r"short.bed: 8 bytes, expected 9 \(3 \+ 3 variants of the .bim x 2 bytes"):
        plink.load_dosage(bad, **ask)
    for ext in (".bim", ".fam"):
        bad, _ = small_fileset(tmp_path, "no" + ext[1:])
        os.remove(bad + ext)
        assert not plink.is_fileset(bad)
        with pytest.raises(ValueError, match=f"cannot open .*no{ext[1:]}\\{ext}"):
            plink.load_dosage(bad + ".bed", **ask)
    # an unknown sample: the VCF reader's words
    vcf = write_vcf(tmp_path / "small.vcf", **args)
    with pytest.raises(ValueError) as from_vcf:
        vcf_load(vcf, "3", ["a", "zz"], [2, 2])
    with pytest.raises(ValueError) as from_set:
        plink.load_dosage(prefix, "3", ["a", "zz"], [2, 2])
    assert str(from_vcf.value) == f"samples not found in {vcf}: zz" and str(from_set.value) == f"samples not found in {prefix}.fam: zz"
    twice, _ = small_fileset(tmp_path, "twice", samples=["a", "b", "c", "b", "e"])
    with pytest.raises(ValueError, match="sample b occurs twice in .*twice.fam"):
        plink.load_dosage(twice, **ask)
    assert plink.load_dosage(twice, "3", ["a", "c"], [2, 2])[1].tolist() == [[2, 0], [0, 1], [1, 2]]  # only a requested name matters
    # a heterozygous call at ploidy 1 names the variant and the sample
    with pytest.raises(ValueError, match="heterozygous call of sample b at variant v1 .position 100., but the sample is configured with ploidy 1"):
        plink.load_dosage(prefix, "3", ["a", "b"], [1, 1])
    with pytest.raises(ValueError, match="heterozygous call of sample c at variant v2"):
        plink.load_dosage(prefix, "3", ["a", "c"], [2, 1], start=150)
    # ploidy above 2: refused before anything is read (the .bed of this one does not even exist)
    with pytest.raises(ValueError, match="sample b is configured with ploidy 4: a PLINK 1 fileset holds haploid and diploid calls only"):
        plink.load_dosage(str(tmp_path / "absent"), "3", ["a", "b"], [2, 4])
    # ... also through read_dosage_data, with the tetraploid fixture's configuration
    cfg = load_config("tests/data/test_mixed_ploidy.config.yaml")
    names = sorted({s for g in ("ref", "tgt", "src") for line in open(cfg.populations.get_population(g)) for s in line.split()[1:2]})
    tetra, _ = small_fileset(tmp_path, "tetra", samples=names, codes=np.full((3, len(names)), HOM_A2), chroms=["21"] * 3)
    kw = dict(chr_name="21", ploidy_config=cfg.ploidies, ref_ind_file=cfg.populations.get_population("ref"),
              tgt_ind_file=cfg.populations.get_population("tgt"), src_ind_file=cfg.populations.get_population("src"))  # fmt: skip
    with pytest.raises(ValueError, match="Failed to read VCF file .*tetra.bed from 21: sample .* is configured with ploidy 4"):
        read_dosage_data(vcf_file=tetra + ".bed", **kw)
    with pytest.raises(ValueError, match="a PLINK fileset is read as unphased dosages only"):
        read_data(vcf_file=tetra + ".bed", **kw)
    # a .bim line with fewer than six columns, and a buffer smaller than a row
    with open(prefix + ".bim", "a") as f:
        f.write("3 v4 0 400\n")
    with pytest.raises(ValueError, match="small.bim: variant line 4 has fewer than 6 columns"):
        plink.load_dosage(prefix, **ask)
    wide, _ = small_fileset(tmp_path, "wide")
    with pytest.raises(ValueError, match="SAI_AMD_INGEST_BUFFER of 1 bytes is smaller than one row of .*wide.bed .2 bytes."):
        plink.load_dosage(wide, buffer_bytes=1, **ask)


def test_one_pass_is_false_and_memory_estimate_is_four_times_the_bed(tmp_path, monkeypatch):
    from sai_amd import sai as sai_mod

    prefix, _ = small_fileset(tmp_path)
    assert sai_mod._reads_in_one_pass(prefix + ".bed") is False and sai_mod._reads_in_one_pass(prefix) is False
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", "12")  # the .bed is 3 + 3 * 2 = 9 bytes: 36 resident
    assert sai_mod.chunks_for_memory(prefix + ".bed") == sai_mod.chunks_for_memory(prefix) == 3
    argv = sai_mod._score_cli_arguments(prefix + ".bed", "3", 10, 5, None, "o.tsv", "c.yaml", 2)
    assert argv[:3] == ["score", "--bfile", prefix] and "--vcf" not in argv
    assert sai_mod._score_cli_arguments("x.vcf", "3", 10, 5, None, "o.tsv", "c.yaml", 2)[:3] == ["score", "--vcf", "x.vcf"]


def sai_cli(*argv, cwd=None):
    return subprocess.run([sys.executable, "-m", "sai_amd", *argv], cwd=str(cwd or ROOT), capture_output=True, text=True, timeout=600)


def test_command_line(tmp_path):
    prefix, _ = small_fileset(tmp_path)
    res = sai_cli("score", "--help")
    assert res.returncode == 0 and "--bfile PREFIX" in res.stdout and "--vcf VCF" in res.stdout
    rest = ["--chr-name", "3", "--output", str(tmp_path / "o.tsv"), "--config", "tests/data/test_sai.config.yaml"]
    res = sai_cli("score", "--vcf", "tests/data/example.vcf", "--bfile", prefix, *rest)
    assert res.returncode == 2 and "exactly one of the arguments --vcf and --bfile is required" in res.stderr
    res = sai_cli("score", *rest)
    assert res.returncode == 2 and "exactly one of the arguments --vcf and --bfile is required" in res.stderr
    os.remove(prefix + ".fam")
    res = sai_cli("score", "--bfile", prefix, *rest)
    assert res.returncode == 2 and f"{prefix}.fam is not found" in res.stderr
    assert not (tmp_path / "o.tsv").exists()


def test_header_and_binding_agree():
    """include/saihip_plink.h, sai_amd/_ffi_plink.py and the library name the same entry points; the first header
    and its version are as they were."""
    from sai_amd import _ffi, _ffi_plink

    names = abi_checks.declared_names("saihip_plink.h")
    assert names == sorted(_ffi_plink.SIGNATURES) and len(names) == 8 and all(n.startswith("sai_plink_") for n in names)
    lib = _ffi_plink.load()
    assert lib.sai_plink_abi_version() == _ffi_plink.SAI_PLINK_ABI_VERSION == abi_checks.header_macro("saihip_plink.h", "SAI_PLINK_ABI_VERSION")
    assert lib.sai_abi_version() == _ffi.SAI_ABI_VERSION == 16 and not any(n.startswith("sai_plink") for n in _ffi.SIGNATURES)
    assert lib.sai_plink_decode(None, None, 0, 0, 0, None, None, 0, 1, None, -1, None, 0, None, 0, None, None) == _ffi.SAI_ERR_ARG
    assert b"ctx is NULL" in lib.sai_last_error()
