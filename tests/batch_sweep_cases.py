"""The cases of the batch-boundary sweeps (test_batch_planner_cpu.py, test_batch_sweep_cpu.py,
test_batch_sweep_device.py): one seeded matrix of hard calls written once per format with the builders the suite has,
three requests per format, the block a request must give -- computed from the matrix alone -- and the sweep of
buffer sizes that moves a batch boundary past every selected row.

The matrix holds PLINK 2 hard-call codes (0 hom REF, 1 het, 2 hom ALT, 3 missing), [variants][samples]: a few variants of
chromosome 6, ``n_here`` of chromosome 7 (the one every request asks for) and a few of chromosome 77 behind them.  The
requests are ``fast`` (a run of consecutive columns at ploidy 2: the kernels' fast path, 37 slots), ``general`` (a
permutation with a repeat at ploidies 1 / 2, or 1 .. 4 with ``wide``: 19 slots) and ``sparse`` (the columns of ``fast``
with a region and an ancestral-allele file that drops about a third of the rows and flips about a third of the rest:
the selected rows have gaps).  37 and 19 are coprime to 16, so ``out_row0 * n_slots mod 16`` -- which bytes of a kernel
call's first and last 16-byte chunk belong to the neighbouring batch -- takes every residue within 16 consecutive row
boundaries."""

import functools
import os
from types import SimpleNamespace

import numpy as np

import bcf_builder
import pgen_builder
from test_eigenstrat_cpu import write_eigenstrat
from test_pgen_cpu import expected as expected_fileset
from test_plink_cpu import write_fileset as write_bed_fileset
from test_plink_cpu import write_vcf

CHROM = "7"
N_IND = 45
N_BEFORE, N_AFTER = 4, 3
SAMPLES = [f"s{i}" for i in range(N_IND)]
HAPLOID_COLS = (1, 8, 15, 22, 29, 36, 43)  # never heterozygous: the columns a request reads at ploidy 1
FAST_COLS = tuple(range(3, 40))
FLIP_MISSING_FROM = 40  # a flipped row holds missing calls in the columns from here on only (dosage 4 does not fit 2 bits)
REQUESTS = ("fast", "general", "sparse")
BED_OF_CODE = np.array([3, 2, 0, 1], dtype=np.uint8)  # hard call -> PLINK 1 code (A1 = ALT, A2 = REF)
G_OF_CODE = np.array([2, 1, 0, 3], dtype=np.uint8)  # hard call -> copies of the first (REF) allele of the .snp line; 3 = missing

# the forced record types of the first variants of a .pgen, from the first variant of the file on: the region's first
# row differs from a record of chromosome 6, two runs of three and four difference rows follow one base each
_HEAD_TYPES = (0, 1, 4, 2) + (2, 3, 0, 2, 2, 3, 1, 3, 3, 2, 2, 4, 2, 6, 3, 7, 2, 3, 3)


@functools.lru_cache(maxsize=None)
def matrix(n_here: int = 60):
    """The case data: codes, site columns, the forced .pgen types and every variant's fate under the ancestral-allele
    file of ``sparse`` ("keep", "flip", "drop", or "out" of the region)."""
    rng = np.random.default_rng(20261020 + n_here)
    n = N_BEFORE + n_here + N_AFTER
    chroms = ["6"] * N_BEFORE + [CHROM] * n_here + ["77"] * N_AFTER
    positions = np.concatenate([np.cumsum(rng.integers(1, 400, k)) + 1000 for k in (N_BEFORE, n_here, N_AFTER)]).tolist()
    types = list(_HEAD_TYPES) + [(0, 0, 1, 2, 2, 3, 3, 4, 6, 7)[int(rng.integers(10))] for _ in range(n - len(_HEAD_TYPES))]
    # Every record type at a length of its own, so that the records of a .pgen are 4 .. 12 bytes: a row and its base
    # then never need more than two plain rows, and the sweep can end a batch behind every row.  A row is either free
    # of missing calls in the columns below FLIP_MISSING_FROM or not (``clean``); a difference row inherits that.
    codes = np.zeros((n, N_IND), dtype=np.uint8)
    clean = np.zeros(n, dtype=bool)
    diploid = np.array([c for c in range(N_IND) if c not in HAPLOID_COLS])
    hap = np.array(HAPLOID_COLS)
    base = -1

    def differ(row, count):
        """``count`` diploid columns of ``row`` changed to another call that is not missing."""
        for c in rng.choice(diploid, size=count, replace=False):
            row[c] = rng.choice([x for x in (0, 1, 2) if x != row[c]])
        return row

    for v in range(n):
        kind = types[v]
        if kind in (2, 3):
            start = pgen_builder.swap02(codes[base]) if kind == 3 else codes[base].copy()
            clean[v] = clean[base]
            codes[v] = differ(start, 2 + v % 3)
        elif kind in (4, 6):
            clean[v] = True
            codes[v] = differ(np.full(N_IND, {4: 0, 6: 2}[kind], dtype=np.uint8), 8)
        elif kind == 7:
            codes[v] = differ(np.full(N_IND, 3, dtype=np.uint8), 8)
        elif kind == 1:
            clean[v] = bool(v % 2)
            lo, hi = ((0, 1), (1, 2), (0, 2))[v % 3] if clean[v] else ((0, 3), (2, 3), (0, 3))[v % 3]
            row = np.where(rng.random(N_IND) < 0.5, lo, hi).astype(np.uint8)
            row[hap] = np.where(row[hap] == 1, hi if lo == 1 else lo, row[hap])
            if not clean[v]:
                row[:FLIP_MISSING_FROM][row[:FLIP_MISSING_FROM] == 3] = lo  # the missing calls lie in the last columns
                row[FLIP_MISSING_FROM:] = 3
                clean[v] = True
            third = next(c for c in (0, 2, 1) if c not in (lo, hi))
            codes[v] = row
            codes[v, rng.choice(diploid[diploid < FLIP_MISSING_FROM], size=3, replace=False)] = third
        else:
            clean[v] = bool(v % 2)
            row = rng.integers(0, 3 if clean[v] else 4, N_IND).astype(np.uint8)
            row[hap] = np.where(row[hap] == 1, 2, row[hap])
            codes[v] = row
        if kind not in (2, 3):
            base = v
    first, last = N_BEFORE + 5, N_BEFORE + n_here - 5  # the region of ``sparse``: variants [first, last] of the file
    fate = np.array(["out"] * n, dtype=object)
    fate[first : last + 1] = rng.choice(["keep", "flip", "drop"], size=last + 1 - first)
    # a gap behind the first row, whose base lies before the region; then a dropped base with four difference rows kept
    fate[first : first + 6] = ["keep", "drop", "flip", "keep", "keep", "keep"]
    fate[last] = "keep"
    for v in range(first + 1, last):  # one base that is itself dropped, its difference rows kept
        if types[v] not in (2, 3) and types[v + 1] in (2, 3) and v > first + 5:
            fate[v], fate[v + 1] = "drop", "keep"
            break
    fate[(fate == "flip") & ~clean] = "keep"  # a flipped row holds no missing call below FLIP_MISSING_FROM: 4 does not fit two bits
    assert clean[first + 2] and (fate == "flip").sum() >= (last - first) // 8
    letters = np.array(list("ACGT"))
    pick = np.array([rng.permutation(4)[:3] for _ in range(n)])
    ref, alt, other = (letters[pick[:, k]].tolist() for k in range(3))
    assert {0, 1, 2, 3} <= set(np.unique(codes).tolist())
    return SimpleNamespace(n=n, n_here=n_here, codes=codes, chroms=chroms, positions=positions, ids=[f"rs{k}" for k in range(n)], ref=ref,
                           alt=alt, other=other, types=types, fate=fate, first=first, last=last)  # fmt: skip


def request(name: str, wide: bool = False, n_here: int = 60):
    """``names``, ``ploidies``, ``cols``, the region and whether the ancestral-allele file is given.  ``wide``: the
    ploidies of ``general`` run from 1 to 4 (the VCF and BCF routes; a haploid column stays at ploidy 1)."""
    m = matrix(n_here)
    if name in ("fast", "sparse"):
        cols, ploidies = list(FAST_COLS), [2] * len(FAST_COLS)
    else:
        rng = np.random.default_rng(19)
        cols = [int(c) for c in rng.permutation(N_IND)[:18]]
        if not wide:
            cols.insert(7, cols[2])  # a repeat: a fileset serves a sample as often as it is asked for
        else:
            cols.insert(7, next(c for c in range(N_IND) if c not in cols))  # a VCF pass takes a sample once
        ploidies = [1 if c in HAPLOID_COLS else (2 + k % 3 if wide else 2) for k, c in enumerate(cols)]
        assert 1 in ploidies and 2 in ploidies and len(cols) == 19
    sparse = name == "sparse"
    return SimpleNamespace(name=name, names=[SAMPLES[c] for c in cols], ploidies=ploidies, cols=cols, anc=sparse,
                           start=m.positions[m.first] if sparse else None, end=m.positions[m.last] if sparse else None)  # fmt: skip


def selection(name: str, n_here: int = 60):
    """(file rows, flips, n_matched, n_anc) of a request: what the index must select."""
    m = matrix(n_here)
    if name != "sparse":
        rows = np.arange(N_BEFORE, N_BEFORE + m.n_here)
        return rows, np.zeros(len(rows), dtype=np.uint8), len(rows), 0
    rows = np.flatnonzero((m.fate == "keep") | (m.fate == "flip"))
    return rows, (m.fate[rows] == "flip").astype(np.uint8), m.last + 1 - m.first, int((m.fate != "out").sum()) - _omitted(m)


def _omitted(m) -> int:
    """Every other dropped variant is not in the ancestral-allele file at all; the others name a third allele."""
    return len(np.flatnonzero(m.fate == "drop")[::2])


def write_anc(path, n_here: int = 60) -> str:
    m = matrix(n_here)
    omitted = set(np.flatnonzero(m.fate == "drop")[::2].tolist())
    with open(path, "w") as f:
        for v in range(m.n):
            if m.fate[v] != "out" and v not in omitted:
                allele = {"keep": m.ref[v], "flip": m.alt[v], "drop": m.other[v]}[m.fate[v]]
                f.write(f"{m.chroms[v]}\t{m.positions[v] - 1}\t{m.positions[v]}\t{allele}\n")
    return str(path)


def expected_vcf(codes, cols, ploidies, flips):
    """The dosage rule of VCF text and BCF (DESIGN_INGEST.md, "Dosage"), for diploid calls in the file: a slot of
    ploidy p sums the alleles at positions 0 .. p - 1 of the call, a missing allele and a position the call does not
    have counting -1; a flipped row counts the other allele, a missing one 2."""
    alleles = np.array([[0, 0], [0, 1], [1, 1], [-1, -1]], dtype=np.int64)[np.asarray(codes)[:, list(cols)]]  # [rows][slots][2]
    alleles = np.concatenate([alleles, np.full(alleles.shape, -1, dtype=np.int64)], axis=2)
    used = np.arange(4)[None, None, :] < np.asarray(ploidies)[None, :, None]
    kept = np.where(used, alleles, 0).sum(axis=2)
    turned = np.where(used, np.where(alleles >= 1, alleles - 1, 1 - alleles), 0).sum(axis=2)
    return np.where(np.asarray(flips, dtype=bool)[:, None], turned, kept).astype(np.int8)


def expected(name: str, wide: bool = False, n_here: int = 60):
    """(pos int32, block int8 [rows][slots], n_matched, n_anc) of a request, from the matrix alone."""
    m, req = matrix(n_here), request(name, wide, n_here)
    rows, flips, n_matched, n_anc = selection(name, n_here)
    if wide:
        block = expected_vcf(m.codes[rows], req.cols, req.ploidies, flips)
    else:
        block, status = expected_fileset(m.codes[rows], req.cols, req.ploidies, flips)
        assert not status.any()  # no heterozygous call in a haploid slot
    return np.asarray(m.positions, dtype=np.int32)[rows], block, n_matched, n_anc


# ---- the files -----------------------------------------------------------------------------------------------


def write_bed(prefix, n_here: int = 60) -> str:
    m = matrix(n_here)
    write_bed_fileset(str(prefix), m.chroms, m.positions, m.ids, m.alt, m.ref, BED_OF_CODE[m.codes], SAMPLES)
    return str(prefix)


def write_pgen(prefix, n_here: int = 60):
    """-> (prefix, the builder's table: (offset, length, vrtype, base variant or -1) of every variant)."""
    m = matrix(n_here)
    table = pgen_builder.write_fileset(str(prefix), m.chroms, m.positions, m.ids, m.ref, m.alt, m.codes, SAMPLES, m.types)
    return str(prefix), table


def write_geno(prefix, encoding: str, n_here: int = 60, **options) -> str:
    m = matrix(n_here)
    write_eigenstrat(str(prefix), encoding, m.chroms, m.positions, m.ids, m.ref, m.alt, G_OF_CODE[m.codes], SAMPLES, **options)
    return str(prefix)


def vcf_text(n_here: int = 60, newline: str = "\n") -> str:
    """Every sample diploid; the haploid columns are never heterozygous, so a slot of ploidy 1 reads their first allele."""
    import tempfile

    m = matrix(n_here)
    with tempfile.TemporaryDirectory() as tmp:
        path = write_vcf(os.path.join(tmp, "m.vcf"), m.chroms, m.positions, m.ids, m.alt, m.ref, BED_OF_CODE[m.codes], SAMPLES)
        with open(path, newline="") as f:
            text = f.read()
    return text.replace("\n", newline)


def write_text(path, text: str) -> str:
    with open(path, "w", newline="") as f:
        f.write(text)
    return str(path)


def write_bcf(path, n_here: int = 60, **options) -> str:
    return bcf_builder.write_bcf(path, vcf_text(n_here), **options)


def write_bgzip(path, text: str, member_size: int = 300, first_member: int = 0) -> tuple:
    """``text`` as BGZF members of ``member_size`` bytes behind one of ``first_member`` bytes.
    -> (path, the inflated size of every member but the EOF marker)."""
    data = text.encode()
    members = bcf_builder.bgzf_members(data[:first_member], 65280, eof=False) + bcf_builder.bgzf_members(data[first_member:], member_size)
    sizes = [min(65280, first_member - at) for at in range(0, first_member, 65280)]
    sizes += [min(member_size, len(data) - at) for at in range(first_member, len(data), member_size)]
    with open(path, "wb") as f:
        f.write(b"".join(members))
    return str(path), sizes


# ---- the indexes of the requests, without the library ---------------------------------------------------------


def pgen_tables(table, rows):
    """(rec, base) int64 [rows][3] as the index of a .pgen gives them for the selected ``rows``."""
    rec = np.array([table[v][:3] for v in rows], dtype=np.int64).reshape(-1, 3)
    base = np.array([list(table[table[v][3]][:3]) if table[v][3] >= 0 else [-1, -1, -1] for v in rows], dtype=np.int64).reshape(-1, 3)
    return rec, base


# ---- the sweep -----------------------------------------------------------------------------------------------

N_LONG = 400  # variants of chromosome 7 in the transposed .geno and the VCF that ``convert`` reads: seven, four and three batches at the three smallest strides


def write_all(folder) -> dict:
    """Every file of the sweeps, written once."""
    folder = str(folder)
    at = lambda name: os.path.join(folder, name)  # noqa: E731
    files = dict(bed=write_bed(at("bed")), anc=write_anc(at("anc.bed")), anc_long=write_anc(at("anc_long.bed"), N_LONG))
    files["pgen"], files["pgen_table"] = write_pgen(at("pgen"))
    files["text"] = write_geno(at("text"), "text")
    files["text_open"] = write_geno(at("text_open"), "text", final_newline=False)  # the last line lacks its newline
    files["packed"] = write_geno(at("packed"), "packed")
    files["transposed"] = write_geno(at("transposed"), "transposed", N_LONG)
    files["bcf"] = write_bcf(at("m.bcf"), member_size=300)
    files["vcf_long"] = write_text(at("long.vcf"), vcf_text(N_LONG))
    return files


N_BGZIP = 700  # variants of chromosome 7 in the two VCFs of the text routes: more than two batches of the smallest size, 64 KiB
BGZIP_FIRST = 65280  # the first member is a full one, so that a batch can end behind each of the small ones that follow
BGZIP_MEMBER = 1000


def bgzip_text(newline: str = "\n") -> str:
    """The VCF of ``N_BGZIP`` variants with meta lines in front that fill the first member."""
    text = vcf_text(N_BGZIP, newline)
    head, rest = text.split(newline, 1)
    pad = "".join(f"##pad{k:04d}=" + "x" * 80 + newline for k in range(BGZIP_FIRST // (90 + len(newline)) + 1))
    return head + newline + pad + rest


def plan_key(batches):
    """What makes two batch lists the same plan: the rows and the reads of every batch."""
    if batches and hasattr(batches[0], "k0"):
        return tuple((b.k0, b.k1, b.stride, tuple(b.reads)) for b in batches)
    return tuple((int(b[0]), int(b[1]), tuple(tuple(int(x) for x in r) for r in b[-1])) for b in batches)


def rows_of(batches):
    return [(b.k0, b.k1) if hasattr(b, "k0") else (int(b[0]), int(b[1])) for b in batches]


def boundaries(plans):
    """(rows that open a batch, rows that close one, batches without a row) over ``plans`` = lists of (k0, k1, ...)."""
    firsts, lasts, empty = set(), set(), 0
    for batches in plans:
        for b in batches:
            if b[1] > b[0]:
                firsts.add(int(b[0]))
                lasts.add(int(b[1]) - 1)
            else:
                empty += 1
    return firsts, lasts, empty


def cap_sweep(batches_at, limit: int = 150, start: int = 1):
    """The sweep of caps of one route and one request.  ``batches_at(cap)`` = the planner's batches, or ValueError where
    the cap is refused.  The planner is run at EVERY integer cap from ``start`` until it gives one batch; kept are the caps
    under which its batch list differs from the list at the next smaller cap, the cap below the smallest legal one
    (``refused``) and one above the one-batch size.  More than ``limit``: the caps that bring a new first or last row
    of a batch (or the first batch without a row) stay, the others are thinned evenly.
    -> caps, refused, plans {cap: [(k0, k1)]}, and the cover reached: firsts, lasts, empty, most batches at one cap."""
    caps, plans, before, cap = [], {}, None, start - 1
    while True:
        cap += 1
        assert cap < 1 << 20, "the planner never comes to one batch"
        try:
            batches = list(batches_at(cap))
        except ValueError:
            assert not caps, f"a cap of {cap} is refused above a legal one"
            continue
        key = plan_key(batches)
        if key != before:
            caps.append(cap)
            plans[cap] = rows_of(batches)
        before = key
        if len(batches) <= 1:
            break
    refused, full = caps[0] - 1, boundaries(plans.values())
    caps.append(cap + 1)
    plans[cap + 1] = plans[cap]
    if len(caps) > limit:
        keep, firsts, lasts, empty = {caps[0], caps[-2], caps[-1]}, set(), set(), 0
        for c in caps:
            f, l, e = boundaries([plans[c]])
            if not (f <= firsts and l <= lasts) or (e and not empty):
                keep.add(c)
            firsts, lasts, empty = firsts | f, lasts | l, empty + e
        rest = [c for c in caps if c not in keep]
        room = max(0, limit - len(keep))
        keep |= set(rest[:: -(-len(rest) // room)]) if room else set()
        caps = sorted(keep)
        plans = {c: plans[c] for c in caps}
        thinned = boundaries(plans.values())
        assert thinned[:2] == full[:2] and bool(thinned[2]) == bool(full[2])  # the thinned set covers what the full one did
    firsts, lasts, empty = boundaries(plans.values())
    return SimpleNamespace(caps=caps, refused=refused, plans=plans, firsts=firsts, lasts=lasts, empty=empty,
                           most=max(len(p) for p in plans.values()), several=sum(1 for p in plans.values() if len(p) >= 3))  # fmt: skip


def bcf_plan(sizes, cap: int, align: int = 16):
    """The batches of the BCF host route (bcf/bcf_index.cpp, restated): GT arrays back to back, each at a multiple of
    ``align``, a batch closed before the array that would pass ``cap``.  -> [(k0, k1)], ValueError below one array."""
    if any(s > cap for s in sizes):
        raise ValueError("smaller than the GT array")
    out, at, k0 = [], 0, 0
    for k, s in enumerate(sizes):
        start = -(-at // align) * align
        if k > k0 and start + s > cap:
            out.append((k0, k, ((0, 0, at),)))
            k0, start = k, 0
        at = start + s
    if len(sizes) > k0:
        out.append((k0, len(sizes), ((0, 0, at),)))
    return out


def member_plan(sizes, cap: int):
    """The batches of the GPU-walk route of a BCF (bcf/bcf_feed.cpp, restated): whole members, a batch closed before
    the member that would pass ``cap`` inflated bytes, one member at least.  -> [(first member, behind the last)]"""
    out, at, m0 = [], 0, 0
    for m, s in enumerate(sizes):
        if m > m0 and at + s > cap:
            out.append((m0, m, ((0, 0, at),)))
            m0, at = m, 0
        at += s
    out.append((m0, len(sizes), ((0, 0, at),)))
    return out
