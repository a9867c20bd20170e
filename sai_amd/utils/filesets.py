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


def release_buffers(eng) -> None:
    for reader in READERS + FILE_READERS:
        reader.release_buffers(eng)
