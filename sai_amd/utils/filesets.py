"""Which reader serves a path: the one place the callers (``read_data``, ``native_vcf.scan_first_last``,
``sai.score``) ask whether ``vcf_file`` names a genotype fileset instead of a VCF.

``reader_for(path)`` gives the reader module (``plink``, ``eigenstrat``, ``pgen`` or ``bcf``: all have ``fileset_prefix``,
``scan_first_last``, ``load_dosage``, ``load_dosage_device`` and ``release_buffers``) or None for anything else,
which is then read as a VCF.  Detection is by content; a bare prefix that has several kinds of files is
served in the order of ``READERS``: PLINK 1, EIGENSOFT, PLINK 2.  ``FILE_READERS`` are asked after them: the
readers of a single file that is not a VCF -- a BCF, which is still named with ``--vcf``."""

from __future__ import annotations

import os
from typing import Optional

from . import bcf, eigenstrat, pgen, plink

READERS = (plink, eigenstrat, pgen)
FILE_READERS = (bcf,)
# per reader: the flag of `sai score` that takes its prefix, the file whose size tells the genotype count, what it is called
_FLAG = {plink: "--bfile", eigenstrat: "--eigenstrat", pgen: "--pfile"}
_DATA = {plink: ".bed", eigenstrat: ".geno", pgen: ".pgen"}
_NAME = {plink: "a PLINK fileset", eigenstrat: "an EIGENSTRAT fileset", pgen: "a PLINK 2 fileset", bcf: "a BCF file"}


def reader_for(path):
    for reader in READERS + FILE_READERS:
        if reader.fileset_prefix(path) is not None:
            return reader
    return None


def is_fileset(path) -> bool:
    return reader_for(path) is not None


def name_of(path) -> Optional[str]:
    """"a PLINK fileset" / "an EIGENSTRAT fileset" / "a PLINK 2 fileset" / "a BCF file", else None."""
    reader = reader_for(path)
    return None if reader is None else _NAME[reader]


def cli_source(path) -> list:
    """The input arguments of ``sai score`` that name ``path``: ``--vcf``, ``--bfile``, ``--eigenstrat`` or ``--pfile``."""
    reader = reader_for(path)
    return ["--vcf", path] if reader is None or reader in FILE_READERS else [_FLAG[reader], reader.fileset_prefix(path)]


def resident_bytes(path) -> Optional[int]:
    """The int8 genotype bytes that stay resident for a fileset (None for anything else): a 2-bit file holds four
    genotypes per byte, a text ``.geno`` one; a ``.pgen`` is compressed, so its header's counts say it, and for a BCF
    the scan's."""
    reader = reader_for(path)
    if reader is None:
        return None
    if reader is pgen:
        variant_ct, sample_ct = pgen.header_counts(path)
        return variant_ct * sample_ct
    if reader is bcf:  # compressed as well: the scan has counted the records
        n_records_total, n_samples = bcf.header_counts(path)
        return n_records_total * n_samples
    data = reader.fileset_prefix(path) + _DATA[reader]
    size = os.path.getsize(data)
    if reader is eigenstrat:
        with open(data, "rb") as f:
            if not f.read(6).lstrip(b"T").startswith(b"GENO"):
                return size
    return size * 4


def _chrom_line_samples(path, lines) -> list:
    for line in lines:
        if line.startswith("#CHROM"):
            return line.rstrip("\r\n").split("\t")[9:]
        if not line.startswith("#"):
            break
    raise ValueError(f"{path}: no #CHROM header line")


def input_samples(path) -> list:
    """The sample names an input holds, in its order, for anything the readers take: the ``#CHROM`` line of a plain,
    gzip or bgzip VCF or of a BCF's header text, the second column (IID) of a ``.fam``, the first of an ``.ind``, the
    IID column of a ``.psam`` (a file without a header line is read as a ``.fam``).  The names are those the readers
    match the sample lists against."""
    import gzip
    import struct

    reader = reader_for(path)
    if reader in (plink, eigenstrat, pgen):
        with open(reader.fileset_prefix(path) + {plink: ".fam", eigenstrat: ".ind", pgen: ".psam"}[reader]) as f:
            rows = [line.split() for line in f if line.split()]
        if reader is eigenstrat:  # a line whose first word begins with # is a comment
            return [row[0] for row in rows if not row[0].startswith("#")]
        column = 1
        if reader is pgen and rows and rows[0][0].startswith("#"):  # a header line: #IID ..., or #FID IID ...
            column = 0 if rows[0][0] == "#IID" else 1
            rows = [row for row in rows if not row[0].startswith("#")]
        return [row[column] for row in rows]
    with open(path, "rb") as f:
        compressed = f.read(2) == b"\x1f\x8b"
    if reader is bcf:
        with gzip.open(path, "rb") as f:
            magic, l_text = struct.unpack("<5sI", f.read(9))
            text = f.read(l_text).split(b"\0", 1)[0].decode("utf-8", "replace")
        return _chrom_line_samples(path, text.splitlines())
    with (gzip.open(path, "rt") if compressed else open(path)) as f:
        return _chrom_line_samples(path, f)


def release_buffers(eng) -> None:
    for reader in READERS + FILE_READERS:
        reader.release_buffers(eng)
