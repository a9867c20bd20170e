"""The cases of the join family (include/saihip_join.h), shared by its CPU and its GPU tests: pairs of position lists
with what ``np.intersect1d`` says about them, and the two inputs of a ``score`` run cut out of
tests/data/test.with.outgroup.vcf.gz."""

import gzip

import numpy as np

from conftest import ROOT

TOP = 2**31 - 1
DATA = ROOT / "tests" / "data"
FIXTURE, ANC, CONFIG = DATA / "test.with.outgroup.vcf.gz", DATA / "test.with.outgroup.anc.alleles", DATA / "test.with.outgroup.config.yaml"
FORMATS = ("vcf", "vcf.gz", "bcf", "bed", "pgen", "geno-text", "geno-packed", "geno-transposed")


# -- sai_site_join -----------------------------------------------------------------------------------------------------


def ascending(rng, n, top=TOP, high=False):
    """n strictly ascending int32 positions in [1, top]: out of the lowest 4 n values, or with ``high`` out of the highest."""
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    span = min(top, max(4 * n, 16))
    return (np.sort(rng.choice(span, size=n, replace=False)) + 1 + (top - span) * high).astype(np.int32)


def join_cases(block, cap):
    """(name, a, b): lengths around ``block`` and one of ``(2 * cap + 3) * block`` rows."""
    rng = np.random.default_rng(20261020)
    some = ascending(rng, 300, 5000)
    cases = [("both empty", some[:0], some[:0]), ("a empty", some[:0], some), ("b empty", some, some[:0]),
             ("single equal", some[:1], some[:1]), ("single different", some[:1], some[1:2]), ("single in many", some[7:8], some),
             ("many against single", some, some[7:8]), ("disjoint", some[::2], some[1::2]), ("identical", some, some.copy()),
             ("a subset of b", some[::3], some), ("b subset of a", some, some[1::4]),
             ("interleaved", np.sort(np.concatenate([some[::2], some[1::6]])), np.sort(np.concatenate([some[1::2], some[::4]]))),
             ("up to the top", np.array([1, 5, TOP - 2, TOP - 1, TOP], dtype=np.int32), np.array([5, TOP - 3, TOP - 1, TOP], dtype=np.int32))]  # fmt: skip
    for k, n in enumerate((block - 1, block, block + 1, 2 * block + 3, (2 * cap + 3) * block)):
        pool = ascending(rng, 2 * n + 17, high=k % 2 == 1)  # a and b are drawn from one pool: about half of a is in b
        a, b = pool[np.sort(rng.choice(pool.size, size=n, replace=False))], pool[rng.random(pool.size) < 0.5]
        cases += [(f"{n} rows of a", a, b), (f"{n} rows of a, all in b", a.copy(), pool), (f"{n} rows of a, b inside", pool, a.copy())]
    return cases


def expected_join(a, b):
    """(rows_a, rows_b, info) by numpy."""
    common, ia, ib = np.intersect1d(a, b, return_indices=True)
    assert np.all(np.diff(ia) > 0) and np.all(np.diff(ib) > 0)
    return ia.astype(np.int32), ib.astype(np.int32), np.array([common.size, -1, -1, common.size == a.size], dtype=np.int64)


def disordered_cases(block):
    """(name, a, b, info[1], info[2]): a position that repeats or descends at the first index that can tell, at the last
    one and across a workgroup's boundary."""
    rng = np.random.default_rng(7)
    n = 3 * block + 5
    good = ascending(rng, n, 10**6)
    out = []
    for name, at in (("first", 1), ("last", n - 1), ("boundary", block), ("boundary of the second block", 2 * block)):
        for kind in ("repeats", "descends"):
            bad = good.copy()
            bad[at] = bad[at - 1] - (kind == "descends")
            out += [(f"a {kind} at the {name} index", bad, good, at, -1), (f"b {kind} at the {name} index", good, bad, -1, at)]
    twice = good.copy()
    twice[[block + 1, 2 * block + 2]] = twice[[block, 2 * block + 1]]
    out.append(("the first of two, both sides", twice, twice.copy(), block + 1, block + 1))
    return out


# -- two inputs of one run ---------------------------------------------------------------------------------------------


def _records():
    lines = gzip.open(FIXTURE, "rt").read().splitlines()
    meta = [ln for ln in lines if ln.startswith("##")]
    (head,) = [ln for ln in lines if ln.startswith("#CHROM")]
    return meta, head.split("\t"), [ln.split("\t") for ln in lines if not ln.startswith("#")]


def _vcf_text(meta, columns, records):
    return "\n".join([*meta, "\t".join(columns), *("\t".join(r) for r in records)]) + "\n"


def _swap(call):
    return call.translate(str.maketrans("01", "10"))


def write_inputs(tmp, complete=False):
    """The fixture cut in two, plus the one VCF that states what the two mean together.

    panel   every sample but the src group's (src_i1), every fixture site, and sites of its own;
    source  src_i1 alone; unless ``complete``: some sites removed, some written with REF and ALT swapped and the calls
            recoded, some homozygous-reference rows written with ALT = ".", one ALT = "." row whose REF is not the
            ancestral allele (its reader drops it), and sites of its own;
    common  all samples, the panel's REF / ALT, exactly the sites both readers keep.
    Returns {"panel", "common", "anc", "src_sample", "source": {...what ``write_source`` needs}}."""
    meta, columns, records = _records()
    s = columns.index("src_i1")
    anc_lines = open(ANC).read().splitlines()
    ancestral = {int(ln.split("\t")[2]): ln.split("\t")[3] for ln in anc_lines}
    extra = lambda pos, calls: ["1", str(pos), ".", "A", "T", "1000", "PASS", ".", "GT", *calls]  # noqa: E731
    n_samples = len(columns) - 9
    taken = {int(r[1]) for r in records}
    own_panel = [] if complete else [p for p in (50, 5001, 20001, 39990) if p not in taken]  # complete: the source covers the panel
    own_source = [p for p in (60, 7001, 30001, 39995) if p not in taken]
    panel, source, common = [], [], []
    for k, r in enumerate(records):
        panel.append(r[:s] + r[s + 1 :])
        src = r[:9] + [r[s]]
        if not complete:
            if k % 7 == 3:
                continue  # absent from the source file
            if k % 5 == 1:
                src[3], src[4], src[9] = r[4], r[3], _swap(r[s])
            elif r[s] in ("0/0", "0|0") and k % 4 == 0 and ancestral[int(r[1])] == r[3]:
                src[4] = "."  # kept with dosage 0: the ancestral allele is its REF
            elif k % 31 == 2 and ancestral[int(r[1])] not in (r[4], "."):
                # written with the panel's ALT as REF and no ALT: its REF is not the ancestral allele, the reader drops the row
                src[3], src[4], src[9] = r[4], ".", "0/0"
                source.append(src)
                continue
        source.append(src)
        common.append(r)
    panel += [extra(p, ["0|1"] * (n_samples - 1)) for p in own_panel]
    source += [extra(p, ["1|1"]) for p in own_source]
    anc_lines += [f"1\t{p - 1}\t{p}\tA" for p in own_panel + own_source]
    by_pos = lambda rows: sorted(rows, key=lambda r: int(r[1]))  # noqa: E731
    out = {"panel": str(tmp / "panel.vcf"), "common": str(tmp / "common.vcf"), "anc": str(tmp / "anc.bed"), "src_sample": "src_i1"}
    open(out["panel"], "w").write(_vcf_text(meta, columns[:s] + columns[s + 1 :], by_pos(panel)))
    open(out["common"], "w").write(_vcf_text(meta, columns, common))
    open(out["anc"], "w").write("\n".join(sorted(anc_lines, key=lambda ln: int(ln.split("\t")[2]))) + "\n")
    out["source"] = {"meta": meta, "columns": columns[:9] + ["src_i1"], "records": by_pos(source)}
    out["n_common"] = len(common)
    assert complete or sum(1 for r in source if r[4] == "." and r[3] == "T") >= 5  # the dropped ALT = "." rows exist
    out["n_fixture"] = len(records)
    return out


def write_source(inputs, fmt, tmp):
    """The source file of ``write_inputs`` in one of FORMATS; returns the path ``score`` takes."""
    import bcf_builder
    import pgen_builder
    from test_eigenstrat_cpu import write_eigenstrat
    from test_plink_cpu import write_fileset

    src = inputs["source"]
    text = _vcf_text(src["meta"], src["columns"], src["records"])
    recs = src["records"]
    if fmt == "vcf":
        path = tmp / "source.vcf"
        path.write_text(text)
        return str(path)
    if fmt == "vcf.gz":
        path = tmp / "source.vcf.gz"
        path.write_bytes(b"".join(bcf_builder.bgzf_members(text.encode())))
        return str(path)
    if fmt == "bcf":
        return bcf_builder.write_bcf(tmp / "source.bcf", text)
    chroms, positions, ids = [r[0] for r in recs], [int(r[1]) for r in recs], [f"v{k}" for k in range(len(recs))]
    ref, alt = [r[3] for r in recs], [r[4] for r in recs]
    n_alt = np.array([[sum(c == "1" for c in r[9])] for r in recs], dtype=np.uint8)  # copies of ALT: 0, 1 or 2
    prefix = str(tmp / f"source_{fmt}")
    if fmt == "bed":
        write_fileset(prefix, chroms, positions, ids, alt, ref, np.array([3, 2, 0], dtype=np.uint8)[n_alt], ["src_i1"])
        return prefix + ".bed"
    if fmt == "pgen":
        pgen_builder.write_fileset(prefix, chroms, positions, ids, ref, alt, n_alt, ["src_i1"])
        return prefix + ".pgen"
    write_eigenstrat(prefix, fmt.split("-")[1], chroms, positions, ids, ref, alt, 2 - n_alt, ["src_i1"])
    return prefix + ".geno"
