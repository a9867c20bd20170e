"""VCF text -> BGZF-compressed BCF 2.2, in pure Python, written from the rules of DESIGN_INGEST.md ("BCF files")
alone: the tests' writer, independent of the reader in sai_amd/csrc/bcf.

``vcf_to_bcf(text, ...)`` returns the file's bytes; ``write_bcf(path, text, ...)`` writes them.  Options: the bytes
of a GT value (1 / 2 / 4; widened when an allele does not fit), a header with or without ``IDX=`` (with: the
dictionary indices are NOT the ordinals, so a reader that ignores them fails), extra FORMAT fields before and
after GT, the member size (200 bytes, so that records, GT arrays and the header span members, up to 65 280), an
EOF member or none, and hooks that damage one field:

  on_record(i, rec)   ``rec`` is the dict ``encode_record`` takes; change it in place (``l_shared`` / ``l_indiv``
                      override the lengths written)
  on_stream(bytes)    the inflated stream before it is cut into members
  on_members(list)    the BGZF members before they are joined

INFO is not carried over (n_info = 0): the reader never looks at it.
"""

from __future__ import annotations

import gzip
import struct
import zlib

from deflate_builder import bgzf_member

MAGIC = b"BCF\x02\x02"
INT8, INT16, INT32, FLOAT, CHAR = 1, 2, 3, 5, 7
_FMT = {INT8: "<b", INT16: "<h", INT32: "<i"}
_EOV = {INT8: -127, INT16: -32767, INT32: -(2**31) + 1}
_MISSING = {INT8: -128, INT16: -32768, INT32: -(2**31)}
_TYPE_OF_WIDTH = {1: INT8, 2: INT16, 4: INT32}


def read_vcf_text(path) -> str:
    with open(path, "rb") as f:
        head = f.read(2)
    opener = gzip.open if head == b"\x1f\x8b" else open
    with opener(path, "rt") as f:
        return f.read()


def typed_int(v: int) -> bytes:
    for t, lo, hi in ((INT8, -120, 127), (INT16, -32760, 32767), (INT32, -(2**31) + 8, 2**31 - 1)):
        if lo <= v <= hi:
            return bytes([1 << 4 | t]) + struct.pack(_FMT[t], v)
    raise ValueError(v)


def descriptor(t: int, count: int) -> bytes:
    return bytes([count << 4 | t]) if count < 15 else bytes([15 << 4 | t]) + typed_int(count)


def typed_string(s: str) -> bytes:
    raw = s.encode()
    return descriptor(CHAR, len(raw)) + raw


def typed_ints(values, t=None) -> bytes:
    if not values:
        return bytes([0])
    t = t or (INT8 if all(-120 <= v <= 127 for v in values) else INT16 if all(-32760 <= v <= 32767 for v in values) else INT32)
    return descriptor(t, len(values)) + b"".join(struct.pack(_FMT[t], v) for v in values)


def _id_of(line: str) -> str:
    inner = line[line.index("<") + 1 :]
    for part in inner.split(","):
        if part.startswith("ID="):
            return part[3:].rstrip(">")
    raise ValueError(line)


def build_header(vcf_header_lines, chroms, idx: bool, extra_before: bool, extra_after: bool):
    """-> (header text with its final NUL, contig -> index, string -> index, sample names)."""
    meta = [ln for ln in vcf_header_lines if ln.startswith("##")]
    chrom_line = next(ln for ln in vcf_header_lines if ln.startswith("#CHROM"))
    have = {(ln.split("=<")[0], _id_of(ln)) for ln in meta if "=<" in ln and "ID=" in ln}
    for c in chroms:
        if ("##contig", c) not in have:
            meta.append(f"##contig=<ID={c}>")
    if ("##FORMAT", "GT") not in have:
        meta.append('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype, with a comma">')
    if extra_before and ("##FORMAT", "DP") not in have:
        meta.insert(1 if meta else 0, '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Depth">')
    if extra_after and ("##FORMAT", "PL") not in have:
        meta.append('##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Likelihoods">')
    if not meta or not meta[0].startswith("##fileformat"):
        meta.insert(0, "##fileformat=VCFv4.2")
    # the dictionaries: contigs in order; strings (FILTER, INFO, FORMAT) in order of first appearance, PASS = 0
    contig_ids, string_ids = [], ["PASS"]
    for ln in meta:
        kind = ln.split("=<")[0] if "=<" in ln else ""
        if kind == "##contig" and _id_of(ln) not in contig_ids:
            contig_ids.append(_id_of(ln))
        elif kind in ("##FILTER", "##INFO", "##FORMAT") and _id_of(ln) not in string_ids:
            string_ids.append(_id_of(ln))
    if idx:  # indices that are not the ordinals: contigs and strings (but PASS) counted backwards from 2 n
        contigs = {c: 2 * len(contig_ids) - k for k, c in enumerate(contig_ids)}
        strings = {s: (0 if s == "PASS" else 2 * len(string_ids) - k) for k, s in enumerate(string_ids)}
        out = []
        for ln in meta:
            kind = ln.split("=<")[0] if "=<" in ln else ""
            if kind == "##contig":
                ln = ln[:-1] + f",IDX={contigs[_id_of(ln)]}>"
            elif kind in ("##FILTER", "##INFO", "##FORMAT"):
                ln = ln[:-1] + f",IDX={strings[_id_of(ln)]}>"
            out.append(ln)
        meta = out
    else:
        contigs = {c: k for k, c in enumerate(contig_ids)}
        strings = {s: k for k, s in enumerate(string_ids)}
    text = "\n".join(meta + [chrom_line]) + "\n"
    return text.encode() + b"\0", contigs, strings, chrom_line.split("\t")[9:]


def gt_values(field: str):
    """The values of one sample's GT sub-field: (allele + 1) << 1 | phased, 0 = missing allele."""
    out, phased, tok = [], 0, ""
    for ch in field + "/":
        if ch in "/|":
            out.append((0 if tok in (".", "") else (int(tok) + 1) << 1) | phased)
            phased, tok = int(ch == "|"), ""
        else:
            tok += ch
    return out


def record_of(line: str, contigs, strings, width: int, extra_before: bool, extra_after: bool) -> dict:
    col = line.split("\t")
    chrom, pos, vid, ref, alt, _qual, flt, _info = col[:8]
    fmt_keys = col[8].split(":") if len(col) > 8 else []
    samples = col[9:]
    alleles = [ref] + ([] if alt == "." else alt.split(","))
    fmt = []
    if "GT" in fmt_keys:
        gi = fmt_keys.index("GT")
        per_sample = [gt_values((s.split(":") + [""] * gi)[gi]) for s in samples]
        length = max((len(v) for v in per_sample), default=1)
        biggest = max((x for v in per_sample for x in v), default=0)
        t = _TYPE_OF_WIDTH[max(width, 1 if biggest <= 127 else 2 if biggest <= 32767 else 4)]
        flat = [x for v in per_sample for x in v + [_EOV[t]] * (length - len(v))]
        fmt.append({"key": strings["GT"], "type": t, "L": length, "values": flat})
    n = len(samples)
    if extra_before:
        fmt.insert(0, {"key": strings["DP"], "type": INT8, "L": 1, "values": [(7 * k + 3) % 100 for k in range(n)]})
    if extra_after:
        fmt.append({"key": strings["PL"], "type": INT16, "L": 3, "values": [(31 * k) % 999 for k in range(3 * n)]})
    return {"chrom": contigs[chrom], "pos0": int(pos) - 1, "rlen": len(ref), "n_allele": len(alleles), "n_info": 0, "n_sample": n,
            "id": "" if vid == "." else vid, "alleles": alleles,
            "filter": [] if flt == "." else [strings.get(f, 0) for f in flt.split(";")], "fmt": fmt}  # fmt: skip


def encode_record(rec: dict) -> bytes:
    shared = struct.pack("<iiiI", rec["chrom"], rec["pos0"], rec["rlen"], 0x7F800001)  # QUAL: the missing float
    shared += struct.pack("<II", rec["n_allele"] << 16 | rec["n_info"], len(rec["fmt"]) << 24 | rec["n_sample"])
    shared += typed_string(rec["id"]) + b"".join(typed_string(a) for a in rec["alleles"]) + typed_ints(rec["filter"])
    indiv = b""
    for f in rec["fmt"]:
        indiv += typed_int(f["key"]) + descriptor(f["type"], f["L"])
        if "payload" in f:
            indiv += f["payload"]
        elif f["type"] in _FMT:
            indiv += b"".join(struct.pack(_FMT[f["type"]], v) for v in f["values"])
        else:
            indiv += b"".join(struct.pack("<f", v) for v in f["values"])
    return struct.pack("<II", rec.get("l_shared", len(shared)), rec.get("l_indiv", len(indiv))) + shared + indiv


def inflated_stream(text: str, width=1, idx=False, extra_before=False, extra_after=False, on_record=None, magic=MAGIC,
                    l_text=None, drop_chrom_line=False) -> bytes:  # fmt: skip
    lines = [ln for ln in text.split("\n") if ln]
    header = [ln for ln in lines if ln.startswith("#")]
    records = [ln.rstrip("\r") for ln in lines if not ln.startswith("#")]
    chroms = list(dict.fromkeys(ln.split("\t", 1)[0] for ln in records))
    htext, contigs, strings, _ = build_header(header, chroms, idx, extra_before, extra_after)
    if drop_chrom_line:
        htext = b"\n".join(ln for ln in htext.split(b"\n") if not ln.startswith(b"#CHROM"))
    out = bytearray(magic + struct.pack("<I", len(htext) if l_text is None else l_text) + htext)
    for i, ln in enumerate(records):
        rec = record_of(ln, contigs, strings, width, extra_before, extra_after)
        if on_record is not None:
            on_record(i, rec)
        out += encode_record(rec)
    return bytes(out)


def bgzf_members(stream: bytes, member_size=65280, level=6, eof=True) -> list:
    members = []
    for at in range(0, len(stream), member_size):
        piece = stream[at : at + member_size]
        comp = zlib.compressobj(level, zlib.DEFLATED, -15)
        members.append(bgzf_member(comp.compress(piece) + comp.flush(), piece))
    if eof:
        comp = zlib.compressobj(level, zlib.DEFLATED, -15)
        members.append(bgzf_member(comp.compress(b"") + comp.flush(), b""))
    return members


def vcf_to_bcf(text: str, member_size=65280, level=6, eof=True, on_stream=None, on_members=None, raw=False, **stream_options) -> bytes:
    stream = inflated_stream(text, **stream_options)
    if on_stream is not None:
        stream = on_stream(stream)
    if raw:
        return stream
    members = bgzf_members(stream, member_size, level, eof)
    if on_members is not None:
        members = on_members(members)
    return b"".join(members)


def write_bcf(path, text: str, **options) -> str:
    with open(path, "wb") as f:
        f.write(vcf_to_bcf(text, **options))
    return str(path)
