"""A writer of PLINK 2 filesets for the tests, in pure Python and written from the format rules of DESIGN_INGEST.md
("PLINK 2 filesets") alone -- nothing here is shared with, or derived from, sai_amd/csrc/pgen.

``build_pgen`` takes a matrix of hard-call codes (0 hom REF, 1 het, 2 hom ALT, 3 missing), [variants][samples], and
per variant a forced record type 0-7 or None for the smallest encoding, and writes storage mode 0x02 or 0x10 with
either vrtype width, any record-length width, optional allele-count and flag arrays in the header, and optional
junk bytes behind the hard-call track of a record (with vrtype bits 4-7 set: they stand for the phase and dosage
tracks a reader has to skip).  ``write_pvar`` / ``write_psam`` write the two text files in their several forms."""

import numpy as np

BLOCK = 65536
# PLINK 1 .bed code (0 A1 A1, 1 missing, 2 het, 3 A2 A2; A1 = ALT) -> PLINK 2 hard-call code
FROM_BED_CODE = np.array([2, 3, 1, 0], dtype=np.uint8)


def varint(value: int) -> bytes:
    """Base 128, low group first, the high bit set on every byte but the last."""
    assert value >= 0
    out = bytearray()
    while True:
        if value < 128:
            out.append(value)
            return bytes(out)
        out.append(128 | (value & 127))
        value >>= 7


def index_width(sample_ct: int) -> int:
    """Bytes of a difflist sample index: what the number sample_ct itself takes."""
    return 1 if sample_ct < 1 << 8 else 2 if sample_ct < 1 << 16 else 3 if sample_ct < 1 << 24 else 4


def pack2(codes) -> bytes:
    """2-bit codes, entry k in bits [2 (k mod 4), +2) of byte k / 4."""
    codes = np.asarray(codes, dtype=np.uint8)
    padded = np.zeros(-(-len(codes) // 4) * 4, dtype=np.uint8)
    padded[: len(codes)] = codes
    q = padded.reshape(-1, 4)
    return (q[:, 0] | q[:, 1] << 2 | q[:, 2] << 4 | q[:, 3] << 6).astype(np.uint8).tobytes()


def difflist_parts(samples, codes, sample_ct: int):
    """The five parts of a difflist: (L, first index of every group, group sizes - 63, 2-bit codes, deltas per group)."""
    samples = [int(s) for s in samples]
    assert all(b > a for a, b in zip(samples, samples[1:])) and all(0 <= s < sample_ct for s in samples)
    if not samples:
        return varint(0), b"", b"", b"", []
    w = index_width(sample_ct)
    groups = [samples[k : k + 64] for k in range(0, len(samples), 64)]
    firsts = b"".join(g[0].to_bytes(w, "little") for g in groups)
    deltas = [b"".join(varint(b - a) for a, b in zip(g, g[1:])) for g in groups]
    sizes = bytes(len(d) - 63 for d in deltas[:-1])
    return varint(len(samples)), firsts, sizes, pack2(codes), deltas


def difflist(samples, codes, sample_ct: int) -> bytes:
    L, firsts, sizes, code_bytes, deltas = difflist_parts(samples, codes, sample_ct)
    return L + firsts + sizes + code_bytes + b"".join(deltas)


def _diff_against(row, start):
    where = np.flatnonzero(row != start)
    return difflist(where, row[where], len(row))


def swap02(row):
    return (row ^ ((~row & 1) << 1)).astype(np.uint8)


def onebit_pair(row):
    """The two codes a type 1 record stores as bits: the two most common of the row, a tie going to the higher code."""
    counts = np.bincount(row, minlength=4)
    lo, hi = sorted(sorted(range(4), key=lambda c: (-int(counts[c]), -c))[:2])
    return lo, hi


def encode(row, kind: int, base=None) -> bytes:
    """The hard-call track of one record of type ``kind``; ``base`` = the codes of the base record (types 2, 3)."""
    row = np.asarray(row, dtype=np.uint8)
    n = len(row)
    if kind == 0:
        return pack2(row)
    if kind == 1:
        lo, hi = onebit_pair(row)
        bits = np.packbits((row == hi).astype(np.uint8), bitorder="little").tobytes()
        start = np.where(row == hi, hi, lo).astype(np.uint8)
        return bytes([4 * lo + (hi - lo)]) + bits + _diff_against(row, start)
    if kind == 2:
        return _diff_against(row, np.asarray(base, dtype=np.uint8))
    if kind == 3:
        return _diff_against(row, swap02(np.asarray(base, dtype=np.uint8)))
    if kind in (4, 6, 7):
        return _diff_against(row, np.full(n, {4: 0, 6: 2, 7: 3}[kind], dtype=np.uint8))
    raise ValueError(f"type {kind} cannot be written")


def build_pgen(matrix, types=None, mode=0x10, wide_types=False, len_bytes=None, allele_bytes=0, flags=False, junk=None,
               allow_bad_first=False):  # fmt: skip
    """-> (file bytes, table): ``table[v] = (offset, length, vrtype, base variant or -1)``.  ``types[v]`` = 0 .. 7 or
    None (the smallest); ``junk[v]`` = bytes appended to record v, whose vrtype then gets bit 4; ``len_bytes`` = None
    takes the fewest bytes that hold the longest record."""
    matrix = np.asarray(matrix, dtype=np.uint8)
    n_var, n = matrix.shape
    types = list(types) if types is not None else [None] * n_var
    head = b"\x6c\x1b" + bytes([mode]) + n_var.to_bytes(4, "little") + n.to_bytes(4, "little")
    if mode == 0x02:
        assert all(t in (None, 0) for t in types)
        row_bytes = -(-n // 4)
        body = b"".join(pack2(r) for r in matrix)
        return head + b"\x00" + body, [(12 + v * row_bytes, row_bytes, 0, -1) for v in range(n_var)]
    assert mode == 0x10
    records, vrtypes, bases = [], [], []
    last_base = -1
    for v in range(n_var):
        first_of_block = v % BLOCK == 0
        kind = types[v]
        if kind is None:
            options = {k: encode(matrix[v], k) for k in (0, 1, 4, 6, 7)}
            if last_base >= 0 and not first_of_block:
                options.update({k: encode(matrix[v], k, matrix[last_base]) for k in (2, 3)})
            kind = min(options, key=lambda k: (len(options[k]), k))
            track = options[kind]
        else:
            if kind in (2, 3):
                assert (last_base >= 0 and not first_of_block) or allow_bad_first
            track = encode(matrix[v], kind, matrix[last_base] if kind in (2, 3) else None)
        vr = kind
        if junk is not None and junk[v]:
            track += bytes(junk[v])
            vr |= 0x10
        bases.append(last_base if kind in (2, 3) else -1)
        if kind not in (2, 3):
            last_base = v
        records.append(track)
        vrtypes.append(vr)
    if len_bytes is None:
        len_bytes = max(1, -(-max(len(r) for r in records).bit_length() // 8)) if records else 1
    n_blocks = -(-n_var // BLOCK)
    control = (4 if wide_types else 0) | (len_bytes - 1) | allele_bytes << 4 | (3 << 6 if flags else 0)
    header_blocks = []
    for b in range(n_blocks):
        lo, hi = b * BLOCK, min(n_var, (b + 1) * BLOCK)
        vt = vrtypes[lo:hi]
        if wide_types:
            part = bytes(vt)
        else:
            assert all(t < 16 or (t & 0xF0) == 0x10 for t in vt)
            nib = [t & 15 for t in vt] + [0]
            part = bytes(nib[k] | nib[k + 1] << 4 for k in range(0, len(vt), 2))
        part += b"".join(len(records[v]).to_bytes(len_bytes, "little") for v in range(lo, hi))
        part += b"\x02" * ((hi - lo) * allele_bytes)  # skipped by size: every variant is said to have two alleles
        if flags:
            part += b"\xff" * (-(-(hi - lo) // 8))
        header_blocks.append(part)
    header_len = 12 + 8 * n_blocks + sum(len(p) for p in header_blocks)
    offsets, table, at = [], [], header_len
    for v in range(n_var):
        if v % BLOCK == 0:
            offsets.append(at)
        table.append((at, len(records[v]), vrtypes[v], bases[v]))
        at += len(records[v])
    data = head + bytes([control]) + b"".join(o.to_bytes(8, "little") for o in offsets) + b"".join(header_blocks) + b"".join(records)
    assert len(data) == at
    return data, table


def write_pvar(path, chroms, positions, ids, ref, alt, header=True, meta_lines=True, extra_columns=False):
    """``header``: #CHROM POS ID REF ALT [QUAL FILTER INFO]; without it the file is a .bim (A1 = ALT, A2 = REF)."""
    with open(path, "w") as f:
        if meta_lines:
            f.write("##fileformat=PVARv1.0\n##contig=<ID=1>\n")
        if header:
            f.write("#CHROM\tPOS\tID\tREF\tALT" + ("\tQUAL\tFILTER\tINFO" if extra_columns else "") + "\n")
        for k in range(len(positions)):
            sep = "\t" if k % 2 or header else " "
            if header:
                fields = [str(chroms[k]), str(positions[k]), str(ids[k]), ref[k], alt[k]] + ([".", "PASS", "."] if extra_columns else [])
            else:
                fields = [str(chroms[k]), str(ids[k]), "0", str(positions[k]), alt[k], ref[k]]
            f.write(sep.join(fields) + "\n")


def write_psam(path, samples, form="#FID IID"):
    """``form``: "#FID IID", "#IID" or "fam" (no header line: FID IID father mother sex phenotype)."""
    with open(path, "w") as f:
        if form == "#FID IID":
            f.write("#FID\tIID\tSEX\n")
            f.writelines(f"fam_{s}\t{s}\tNA\n" for s in samples)
        elif form == "#IID":
            f.write("#IID\tSEX\n")
            f.writelines(f"{s}\tNA\n" for s in samples)
        else:
            f.writelines(f"fam_{s} {s} 0 0 0 -9\n" for s in samples)


def write_fileset(prefix, chroms, positions, ids, ref, alt, matrix, samples, types=None, pvar=None, psam="#FID IID", **pgen_options):
    """PREFIX.pgen / .pvar / .psam; returns the table of ``build_pgen``."""
    matrix = np.asarray(matrix, dtype=np.uint8).reshape(len(positions), len(samples))
    data, table = build_pgen(matrix, types, **pgen_options)
    with open(f"{prefix}.pgen", "wb") as f:
        f.write(data)
    write_pvar(f"{prefix}.pvar", chroms, positions, ids, ref, alt, **(pvar or {}))
    write_psam(f"{prefix}.psam", samples, psam)
    return table


def from_bed_fileset(bed_prefix, prefix, types=None, **options):
    """The PLINK 1 fileset BED_PREFIX (.bed / .bim / .fam; A1 = ALT, A2 = REF) as a PLINK 2 one."""
    bim = [line.split() for line in open(bed_prefix + ".bim") if line.strip()]
    samples = [line.split()[1] for line in open(bed_prefix + ".fam") if line.strip()]
    raw = np.fromfile(bed_prefix + ".bed", dtype=np.uint8)[3:].reshape(len(bim), -1)
    bed_codes = np.stack([(raw >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(len(bim), -1)[:, : len(samples)]
    return write_fileset(prefix, [b[0] for b in bim], [int(b[3]) for b in bim], [b[1] for b in bim], [b[5] for b in bim],
                         [b[4] for b in bim], FROM_BED_CODE[bed_codes], samples, types, **options)  # fmt: skip


def parse_hex(text: str) -> bytes:
    """The bytes of a hex listing with comments: of every line the two-digit tokens (and "|" separators) up to the
    first other word."""
    out = bytearray()
    for line in text.splitlines():
        for token in line.split():
            if token == "|":
                continue
            if len(token) == 2 and all(c in "0123456789ABCDEFabcdef" for c in token):
                out.append(int(token, 16))
            else:
                break
    return bytes(out)
