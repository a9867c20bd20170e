"""A BGZF-compressed BCF -> its .csi index (CSI v1), in pure Python, written from the rules of DESIGN_INGEST.md ("BCF
files: a region is a seek") alone: the tests' writer, independent of the reader in sai_amd/csrc/bcf/csi_index.cpp.

``records_of(bcf_bytes)`` finds the members from their BSIZE fields, inflates them with zlib and walks ``l_shared`` /
``l_indiv``: one dict per record with its virtual offsets (``voff``, ``end``), ``chrom``, ``pos0`` and ``rlen``.
``index_stream(records, ...)`` bins them, merges the chunks of a bin that are adjacent in the file, computes
``loffset`` and returns the inflated bytes of the index; ``write_csi(bcf_path, ...)`` writes them as BGZF beside the
file.  Parameters: ``min_shift`` and ``depth``, whether the pseudo-bin and ``n_no_coor`` are written, the index's mtime.

Conventions where the rules leave a choice: a record's bin is the deepest one that holds all of [pos0, pos0 +
max(rlen, 1)); the virtual offset of a record's END that falls on a member boundary stays in the member that holds the
record's last byte (uoffset = that member's ISIZE), while a record's START there is byte 0 of the next member; the
``loffset`` of a bin is the smallest virtual offset of a record of the contig that overlaps the bin's interval.
"""

from __future__ import annotations

import bisect
import os
import struct
import zlib

from bcf_builder import bgzf_members


def members_of(data: bytes) -> list:
    """[(file offset, inflated bytes)] of every BGZF member."""
    out, at = [], 0
    while at < len(data):
        assert data[at : at + 4] == b"\x1f\x8b\x08\x04", at
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        extra, bsize, o = data[at + 12 : at + 12 + xlen], None, 0
        while o + 4 <= len(extra):
            slen = struct.unpack_from("<H", extra, o + 2)[0]
            if extra[o : o + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", extra, o + 4)[0] + 1
            o += 4 + slen
        assert bsize is not None, at
        out.append((at, zlib.decompress(data[at + 12 + xlen : at + bsize - 8], -15)))
        at += bsize
    return out


def records_of(data: bytes) -> list:
    members = [m for m in members_of(data) if m[1]]
    starts, total = [], 0
    for _, text in members:
        starts.append(total)
        total += len(text)
    stream = b"".join(text for _, text in members)

    def voff(g: int, is_end: bool) -> int:
        k = (bisect.bisect_left(starts, g) - 1) if is_end else (bisect.bisect_right(starts, g) - 1)
        k = max(k, 0)
        return members[k][0] << 16 | (g - starts[k])

    assert stream[:5] == b"BCF\x02\x02"
    g = 9 + struct.unpack_from("<I", stream, 5)[0]
    out = []
    while g < len(stream):
        l_shared, l_indiv, chrom, pos0, rlen = struct.unpack_from("<IIiii", stream, g)
        nxt = g + 8 + l_shared + l_indiv
        out.append({"g": g, "g_end": nxt, "voff": voff(g, False), "end": voff(nxt, True), "chrom": chrom, "pos0": pos0, "rlen": rlen})
        g = nxt
    assert g == len(stream)
    return out


def level_start(level: int) -> int:
    return ((1 << 3 * level) - 1) // 7


def pseudo_bin(depth: int) -> int:
    return ((1 << (3 * depth + 3)) - 1) // 7 + 1


def bin_of(beg: int, fin: int, min_shift: int, depth: int) -> int:
    """The deepest bin that holds all of [beg, fin)."""
    for level in range(depth, -1, -1):
        s = min_shift + 3 * (depth - level)
        if beg >> s == (fin - 1) >> s and beg >> s < 1 << 3 * level:
            return level_start(level) + (beg >> s)
    return 0  # beyond the range of the index: level 0 takes it


def bin_interval(b: int, min_shift: int, depth: int) -> tuple:
    level = max(lv for lv in range(depth + 1) if level_start(lv) <= b)
    s = min_shift + 3 * (depth - level)
    return (b - level_start(level)) << s, (b - level_start(level) + 1) << s


def index_stream(records, min_shift=14, depth=5, pseudo=True, n_no_coor=True, n_ref=None) -> bytes:
    n_ref = (max((r["chrom"] for r in records), default=-1) + 1) if n_ref is None else n_ref
    out = bytearray(b"CSI\x01" + struct.pack("<iiii", min_shift, depth, 0, n_ref))
    for tid in range(n_ref):
        mine = [r for r in records if r["chrom"] == tid]
        bins: dict = {}
        for r in mine:
            beg, fin = r["pos0"], r["pos0"] + max(r["rlen"], 1)
            r["bin"] = bin_of(beg, fin, min_shift, depth)
            chunks = bins.setdefault(r["bin"], [])
            if chunks and chunks[-1][2] == r["g"]:  # adjacent in the file: one chunk
                chunks[-1] = (chunks[-1][0], r["end"], r["g_end"])
            else:
                chunks.append((r["voff"], r["end"], r["g_end"]))
        body = bytearray()
        for b in sorted(bins):
            lo, hi = bin_interval(b, min_shift, depth)
            loffset = min(r["voff"] for r in mine if r["bin"] == b or (r["pos0"] < hi and r["pos0"] + max(r["rlen"], 1) > lo))
            body += struct.pack("<IQi", b, loffset, len(bins[b]))
            for beg, end, _ in bins[b]:
                body += struct.pack("<QQ", beg, end)
        n_bin = len(bins)
        if pseudo and mine:
            body += struct.pack("<IQi", pseudo_bin(depth), 0, 2)
            body += struct.pack("<QQQQ", min(r["voff"] for r in mine), max(r["end"] for r in mine), len(mine), 0)
            n_bin += 1
        out += struct.pack("<i", n_bin) + body
    if n_no_coor:
        out += struct.pack("<Q", 0)
    return bytes(out)


def write_csi(bcf_path, min_shift=14, depth=5, pseudo=True, n_no_coor=True, mtime_ns=None, member_size=65280, on_stream=None, n_ref=None) -> str:
    """Writes ``<bcf_path>.csi``; ``on_stream(bytes)`` may damage the inflated bytes first.  ``mtime_ns`` sets the
    index's time (default: that of the data file, so that the index counts as current)."""
    bcf_path = os.fspath(bcf_path)
    with open(bcf_path, "rb") as f:
        records = records_of(f.read())
    stream = index_stream(records, min_shift, depth, pseudo, n_no_coor, n_ref)
    if on_stream is not None:
        stream = on_stream(stream)
    return write_index_bytes(bcf_path, stream, mtime_ns, member_size)


def write_index_bytes(bcf_path, stream: bytes, mtime_ns=None, member_size=65280) -> str:
    bcf_path = os.fspath(bcf_path)
    with open(bcf_path + ".csi", "wb") as f:
        f.write(b"".join(bgzf_members(stream, member_size)))
    t = os.stat(bcf_path).st_mtime_ns if mtime_ns is None else mtime_ns
    os.utime(bcf_path + ".csi", ns=(t, t))
    return bcf_path + ".csi"
