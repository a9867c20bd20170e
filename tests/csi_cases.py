"""The files, regions and wrong indexes that tests/test_bcf_index_cpu.py and tests/test_bcf_index_device.py share.

One VCF text of three contigs ("1", "2", "3"; the wanted one in the middle), 60 + 300 + 60 records of 5 samples,
written as a BCF in members of 700 inflated bytes, so that a few dozen members are in play and records span them.
Contig 2 has repeated positions, gaps of several leaf bins, a few records whose ``rlen`` reaches a level-1 or the
level-0 bin, and positions beyond 4096, which a (min_shift 6, depth 2) index does not cover.
"""

from __future__ import annotations

import os

import numpy as np

import bcf_builder as B
import csi_builder as X

SAMPLES = [f"s{k}" for k in range(5)]
MEMBER = 700
LAYOUTS = [(4, 3), (6, 2), (5, 2)]  # (min_shift, depth): 8192, 4096 and 2048 bases
LONG = {20: 100, 30: 100, 40: 100, 70: 3000, 120: 700, 200: 5000, 260: 90}  # record number -> rlen


def vcf_text(seed=5, rotate_ids=0) -> str:
    """``rotate_ids`` hands every record the ID of the record that many places on: the same bytes in total, but every
    record at another offset."""
    rng = np.random.default_rng(seed)
    lines = ["##fileformat=VCFv4.2", "##contig=<ID=1>", "##contig=<ID=2>", "##contig=<ID=3>",
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(SAMPLES)]  # fmt: skip
    rows = []
    for chrom, n in (("1", 60), ("2", 300), ("3", 60)):
        pos = 3
        for k in range(n):
            pos += int(rng.choice([0, 1, 3, 10, 25, 60])) + (600 if chrom == "2" and k == 150 else 0)
            ref, alt = rng.permutation(["A", "C", "G", "T"])[:2]
            calls = [f"{a}{'|' if rng.random() < 0.5 else '/'}{b}" for a, b in rng.integers(0, 2, size=(len(SAMPLES), 2))]
            rows.append([chrom, str(pos), "x" * int(rng.integers(0, 14)) or ".", ref, alt, ".", ".", ".", "GT"] + calls)
    ids = [r[2] for r in rows]
    for k, r in enumerate(rows):
        r[2] = ids[(k + rotate_ids) % len(rows)]
    return "\n".join(lines + ["\t".join(r) for r in rows]) + "\n"


def _long(i, rec):
    if i - 60 in LONG:
        rec["rlen"] = LONG[i - 60]


def write_bcf(path, level=6, rotate_ids=0) -> str:
    return B.write_bcf(path, vcf_text(rotate_ids=rotate_ids), member_size=MEMBER, level=level, on_record=_long)


def records(path) -> list:
    with open(path, "rb") as f:
        return X.records_of(f.read())


def anc_file(path, bcf_path) -> str:
    """Ancestral alleles of contig 2 that keep, flip, drop and miss records, by position."""
    text = vcf_text()
    rows = []
    for k, ln in enumerate(ln.split("\t") for ln in text.split("\n") if ln.startswith("2\t")):
        allele = [ln[3], ln[4], "N", None][k % 4]
        if allele is not None:
            rows.append(f"2\t{int(ln[1]) - 1}\t{ln[1]}\t{allele}")
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")
    return str(path)


def empty_leaf(recs, tid, min_shift):
    """The number (inside its level) of a leaf bin without a record start that has such bins on both sides, or None."""
    filled = {r["pos0"] >> min_shift for r in recs if r["chrom"] == tid}
    return next((b + 1 for b in sorted(filled) if b + 1 not in filled and any(c > b + 1 for c in filled)), None)


def regions(recs, tid, min_shift, depth) -> list:
    """(start, end) with None = open: around every bin boundary of a sample of the contig's records and one base to
    either side, before the first and behind the last record, an empty leaf bin with records on both sides, open start,
    open end, and a start beyond the index's range."""
    pos = sorted({r["pos0"] + 1 for r in recs if r["chrom"] == tid})
    leaf = 1 << min_shift
    out = [(None, pos[len(pos) // 2]), (pos[len(pos) // 3], None), (1, max(1, pos[0] - 1)), (pos[-1] + 1, pos[-1] + 50), (pos[-1] + 1, None)]
    for p in pos[:: max(1, len(pos) // 12)] + pos[-2:]:
        edge = (p - 1) // leaf * leaf + 1  # the first 1-based base of p's leaf bin
        for start in (edge - 1, edge, edge + 1, p):
            if start >= 1:
                out += [(start, start + leaf - 1), (start, start + 3 * leaf), (start, None)]
        out += [(max(1, p - 40), edge - 1), (max(1, p - 40), edge), (max(1, p - 40), edge + 1)]
    gap = empty_leaf(recs, tid, min_shift)  # contig 2 has one in every layout (test_the_files_hold_what_they_promise)
    if gap is not None:
        out += [(gap * leaf + 1, (gap + 1) * leaf), (gap * leaf + 1, None), (gap * leaf + 1, gap * leaf + 1)]
    out += [((1 << (min_shift + 3 * depth)) + 1, None), (1 << (min_shift + 3 * depth), None)]
    return list(dict.fromkeys(out))


def last_quarter(path, tid=1) -> tuple:
    """(start, None) of contig ``tid`` whose first record lies behind 3/4 of the file's bytes -- checked here, without
    the reader -- and the record itself."""
    size = os.path.getsize(path)
    r = next(r for r in records(path) if r["chrom"] == tid and (r["voff"] >> 16) > 0.78 * size)
    assert (r["voff"] >> 16) > 0.75 * size
    return (r["pos0"] + 1, None), r


# ---- every way an index can be wrong ------------------------------------------------------------------------------


def field_boundaries(stream: bytes) -> list:
    """The offsets at which a field of the index's inflated bytes begins, and its end."""
    import struct

    out, o = [0, 4, 8, 12, 16], 16
    n_ref = struct.unpack_from("<i", stream, 16)[0]
    o = 20
    for _ in range(n_ref):
        out.append(o)
        n_bin = struct.unpack_from("<i", stream, o)[0]
        o += 4
        for _ in range(n_bin):
            out += [o, o + 4, o + 12]
            n_chunk = struct.unpack_from("<i", stream, o + 12)[0]
            o += 16
            for _ in range(n_chunk):
                out += [o, o + 8]
                o += 16
    out.append(o)
    if o < len(stream):
        out.append(len(stream))
    return sorted(set(out))


def wrong_indexes(bcf_path, other_path, min_shift=4, depth=3) -> list:
    """(name, writer): each writer puts one wrong index beside ``bcf_path``; the time of every one is its own, so that
    none is taken for another by the reader's cache.  ``other_path``: a file of the same size with other record
    offsets."""
    recs, size = records(bcf_path), os.path.getsize(bcf_path)
    good = X.index_stream(recs, min_shift, depth)
    t0 = os.stat(bcf_path).st_mtime_ns
    bounds = field_boundaries(good)
    cases = []

    def case(name, stream, mtime_ns=None):
        k = len(cases) + 1
        cases.append((name, lambda: X.write_index_bytes(bcf_path, stream, t0 + k * 10**9 if mtime_ns is None else mtime_ns)))

    for cut in [bounds[1], bounds[4], bounds[5], bounds[6], bounds[len(bounds) // 2], bounds[-3]]:
        case(f"truncated at {cut}", good[:cut])
    case("bad magic", b"CSJ\x01" + good[4:])
    case("n_ref above the contigs", X.index_stream(recs, min_shift, depth, n_ref=4))

    def changed(**how):
        out = [dict(r) for r in recs]
        for r in out:
            if r["chrom"] == 1:
                for key, f in how.items():
                    r[key] = f(r)
        return X.index_stream(out, min_shift, depth)

    case("coffset beyond the file", changed(voff=lambda r: r["voff"] + (size << 16), end=lambda r: r["end"] + (size << 16)))
    case("chunk_beg >= chunk_end", changed(end=lambda r: r["voff"], g_end=lambda r: -1))
    case("older than the data file", good, t0 - 10 * 10**9)
    case("v in the middle of a record", changed(voff=lambda r: r["voff"] + 5, end=lambda r: r["end"] + 5))
    case("built for another file of the same size", X.index_stream(records(other_path), min_shift, depth))
    return cases
