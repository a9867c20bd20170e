"""A VCF's calls written as an EIGENSOFT fileset (PREFIX.geno + PREFIX.snp + PREFIX.ind): ``sai convert --out-eigenstrat``.

ADMIXTOOLS (``qpDstat``, ``qpF4ratio``) reads nothing else, and the archaic and ancient genomes come in this form
(DESIGN_INGEST.md, "EIGENSTRAT filesets").  ``convert`` reads one chromosome (or a range of it) as ``bed_writer.convert``
does -- the sample checks, the read, the site scan beside it and the agreement of the two are that module's, shared --
and writes the ``.geno`` in one of its two binary forms, encoded on the GPU (sai_amd/csrc/eigenstrat/geno_encode.hip):

 * ``packed`` (PACKEDANCESTRYMAP, "GENO", the default): one record per variant; ``sai_geno_encode``, the inverse of
   ``sai_eigenstrat_decode``, batch by batch over the variants like a ``.bed``;
 * ``transposed`` ("TGENO"): one record per individual; ``sai_geno_encode_transposed``, the inverse of
   ``sai_eigenstrat_decode_transposed``, turns the 2-bit matrix in LDS.  The batches run over the INDIVIDUALS: one call
   encodes some of them over every variant of the resident block, so the file is still written front to back.

A genotype is the number of copies of the first allele of the ``.snp`` line, and the first allele is REF.  What the
fileset promises is what ``bed_writer`` promises: reading it at the ploidies it was written with gives the block the VCF
reader gives for the same samples, byte for byte.  The two hashes of the header record follow EIGENSOFT's ``hasharr`` as
remembered from ``admutils.c``; no EIGENSOFT program was at hand to check them, this project's reader ignores them, and
``hashcheck: NO`` in a ``convertf`` / ADMIXTOOLS parameter file is the way around a mismatch.  The table, the format and
the refusals are in DESIGN_INGEST.md ("EIGENSOFT filesets written from a VCF").

The entry points are internal to the package: their declarations are in sai_amd/csrc/eigenstrat/geno_export.hpp, not
under include/, and this module -- their only caller -- binds them, with a version number of their own.
"""

from __future__ import annotations

import ctypes as C
import os
import time
from typing import Mapping, Optional, Sequence

import numpy as np

from .. import _ffi
from .._binding import extension
from . import bed_writer
from ._ingest import check_io, default_threads

SAI_GENO_EXPORT_ABI_VERSION = 1
FORMATS = ("packed", "transposed")
MIN_RECORD = 48  # bytes: the header record has to fit

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names sai_amd/csrc/eigenstrat/geno_export.hpp declares
SIGNATURES = {
    "sai_geno_export_abi_version": (C.c_int, []),
    "sai_geno_encode_host": (C.c_int, [_p, _i64, _i32, _p, _i32, _i32, _i32, _i32, _p, _p, _i32]),
    "sai_geno_encode": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _p, _p, _p]),
    "sai_geno_encode_transposed": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _i32, _i32, _p, _p, _p]),
    "sai_geno_hash_lines": (C.c_int, [C.c_char_p, _i64, C.POINTER(C.c_uint32)]),
    "sai_geno_snp_lines": (C.c_int, [C.c_char_p, _i64, _p, _i64, C.POINTER(_i64)]),
}
HOST_SYMBOLS = ("sai_geno_export_abi_version", "sai_geno_encode_host", "sai_geno_hash_lines", "sai_geno_snp_lines")

load, load_host = extension("geno export", "sai_amd/csrc/eigenstrat/geno_export.hpp", "sai_geno_export_abi_version", SAI_GENO_EXPORT_ABI_VERSION,
                            SIGNATURES, HOST_SYMBOLS, built_from="eigenstrat")  # fmt: skip

_WORDS = dict(fileset="EIGENSOFT fileset", sample_file=".ind", row=".geno record")
_ptr = bed_writer._ptr


def record_bytes(n: int) -> int:
    """Bytes of a record of ``n`` genotypes: the individuals of a packed file, the variants of a transposed one."""
    return max(MIN_RECORD, (n + 3) // 4)


def encode_host(dosage: np.ndarray, ploidies, transposed: bool = False, slot0: int = 0, n_out: Optional[int] = None,
                status: Optional[np.ndarray] = None, n_threads: Optional[int] = None):  # fmt: skip
    """(records uint8 [rows or n_out][record_bytes], status int32 [rows]) of an int8 [rows][slots] block:
    ``sai_geno_encode_host``.  ``ploidies`` = 1, 2 or one value per slot.  Transposed: the records of the slots
    [slot0, slot0 + n_out) (default: all); ``status`` is raised in place where one is given (the calls over the slot
    groups of a block share it), else it starts at zero."""
    lib = load_host()
    dosage = np.ascontiguousarray(dosage, dtype=np.int8)
    n_rows, n_slots = dosage.shape
    uniform, per_slot = bed_writer._ploidy_arguments(ploidies)
    n_out = n_slots - slot0 if n_out is None else n_out
    records = np.empty((n_out, record_bytes(n_rows)) if transposed else (n_rows, record_bytes(n_slots)), dtype=np.uint8)
    if status is None:
        status = np.zeros(n_rows, dtype=np.int32)
    check_io(lib, lib.sai_geno_encode_host(_ptr(dosage), n_rows, n_slots, _ptr(per_slot), uniform, int(bool(transposed)), slot0, n_out, _ptr(records),
                                           _ptr(status), n_threads or default_threads()))  # fmt: skip
    return records, status


def hash_lines(text: bytes) -> int:
    """EIGENSOFT's ``hasharr`` over the first word of every line (``sai_geno_hash_lines``, where the rule is stated)."""
    lib = load_host()
    h = C.c_uint32()
    check_io(lib, lib.sai_geno_hash_lines(text, len(text), C.byref(h)))
    return int(h.value)


def snp_text(bim: bytes) -> bytes:
    """The ``.snp`` lines "ID CHROM 0.0 POS REF ALT" of the ``.bim`` lines "CHROM ID 0 POS ALT REF" the site columns
    give, an ID of "." written CHROM:POS (``sai_geno_snp_lines``: one pass in C, as ``pgen_writer.pvar_text``)."""
    lib = load_host()
    n = _i64()
    check_io(lib, lib.sai_geno_snp_lines(bim, len(bim), None, 0, C.byref(n)))
    out = C.create_string_buffer(max(int(n.value), 1))
    check_io(lib, lib.sai_geno_snp_lines(bim, len(bim), out, int(n.value), C.byref(n)))
    return out.raw[: int(n.value)]


def ind_text(samples: Sequence[str], labels: Optional[Mapping[str, str]] = None) -> bytes:
    """The ``.ind`` lines "NAME U LABEL": the label is what ADMIXTOOLS takes as the population."""
    labels = labels or {}
    return "".join(f"{s} U {labels.get(s, s)}\n" for s in samples).encode()


def header_record(geno_format: str, n_ind: int, n_snp: int, ind: bytes, snp: bytes) -> bytes:
    """The first record of the ``.geno``: "GENO" or "TGENO", the two counts and the two hashes, zero-padded."""
    transposed = geno_format == "transposed"
    text = "%s %7d %7d %x %x" % ("TGENO" if transposed else "GENO", n_ind, n_snp, hash_lines(ind), hash_lines(snp))
    return text.encode().ljust(record_bytes(n_snp if transposed else n_ind), b"\0")


def labels_of(path) -> dict:
    """name -> second word of its line, for the lines of a ``--samples`` file that have one."""
    with open(path) as f:
        return {w[0]: w[1] for w in (line.split() for line in f) if len(w) > 1}


class _Target:
    """The three files of a conversion, written under temporary names and renamed at the end."""

    def __init__(self, prefix: str):
        self.final = {ext: prefix + ext for ext in (".geno", ".snp", ".ind")}
        if os.path.exists(self.final[".geno"]):
            raise ValueError(f"{self.final['.geno']} exists: name another prefix (nothing is appended to a .geno: its counts sit in the header record)")
        self.paths = {ext: f"{p}.tmp{os.getpid()}" for ext, p in self.final.items()}

    def open_geno(self, header: bytes):
        f = open(self.paths[".geno"], "wb")
        f.write(header)
        return f

    def write_text(self, snp: bytes, ind: bytes) -> None:
        with open(self.paths[".snp"], "wb") as f:
            f.write(snp)
        with open(self.paths[".ind"], "wb") as f:
            f.write(ind)

    def commit(self) -> None:
        for ext in (".snp", ".ind", ".geno"):  # the .geno last: its presence is what refuses a second conversion
            os.replace(self.paths[ext], self.final[ext])

    def rollback(self) -> None:
        for p in self.paths.values():
            if os.path.exists(p):
                os.remove(p)


def _batch_budget() -> int:
    return int(os.environ.get("SAI_AMD_CONVERT_BATCH", bed_writer.BATCH_BYTES))


def _batches(transposed: bool, n_rows: int, n_slots: int):
    """[(first, end)] of the batches -- rows of the packed form, slots of the transposed one -- and the record size.
    Packed batches start at a multiple of 16 rows, so that every batch of the block starts at a 16-byte boundary."""
    if transposed:
        rlen = record_bytes(n_rows)
        step = max(1, _batch_budget() // rlen)
        n = n_slots
    else:
        rlen = record_bytes(n_slots)
        step = bed_writer._batch_rows(rlen)
        n = n_rows
    return [(k0, min(k0 + step, n)) for k0 in range(0, n, step)], rlen


def _write_records_host(dos, uniform, per_slot, transposed, f, ms, n_threads):
    """Host route: ``sai_geno_encode_host`` batch by batch, written as it comes.  -> status"""
    lib = load_host()
    n_rows, n_slots = dos.shape
    batches, rlen = _batches(transposed, n_rows, n_slots)
    status = np.zeros(n_rows, dtype=np.int32)  # the transposed calls only raise it
    out = np.empty(max(k1 - k0 for k0, k1 in batches) * rlen, dtype=np.uint8)
    for k0, k1 in batches:
        t0 = time.perf_counter()
        if transposed:
            rc = lib.sai_geno_encode_host(_ptr(dos), n_rows, n_slots, _ptr(per_slot), uniform, 1, k0, k1 - k0, _ptr(out), _ptr(status), n_threads)
        else:
            rc = lib.sai_geno_encode_host(_ptr(dos[k0:k1]), k1 - k0, n_slots, _ptr(per_slot), uniform, 0, 0, n_slots, _ptr(out), _ptr(status[k0:k1]), n_threads)
        check_io(lib, rc)
        t1 = time.perf_counter()
        f.write(memoryview(out)[: (k1 - k0) * rlen])
        ms["encode"] += (t1 - t0) * 1e3
        ms["write"] += (time.perf_counter() - t1) * 1e3
    return status


def _write_records_device(eng, dos, uniform, per_slot, transposed, f, ms):
    """GPU route: ``bed_writer._stream_batches`` over the batches of ``_batches``.  The status words of the transposed
    form are zeroed here, once, and raised by every call.  -> status"""
    import torch

    lib = eng.lib
    load()
    n_rows, n_slots = dos.shape
    batches, rlen = _batches(transposed, n_rows, n_slots)
    status = torch.zeros((n_rows,), dtype=torch.int32, device=eng.device)
    ploidy_dev = None if per_slot is None else torch.from_numpy(per_slot).to(eng.device)

    def launch(i, out_ptr, side):
        k0, k1 = batches[i]
        if transposed:
            rc = lib.sai_geno_encode_transposed(eng.ctx, C.c_void_p(dos.data_ptr()), n_rows, n_slots, eng._ptr(ploidy_dev), uniform, k0, k1 - k0, out_ptr,
                                                C.c_void_p(status.data_ptr()), C.c_void_p(side.cuda_stream))  # fmt: skip
        else:
            rc = lib.sai_geno_encode(eng.ctx, C.c_void_p(dos.data_ptr() + k0 * n_slots), k1 - k0, n_slots, eng._ptr(ploidy_dev), uniform, out_ptr,
                                     C.c_void_p(status.data_ptr() + 4 * k0), C.c_void_p(side.cuda_stream))  # fmt: skip
        _ffi.check(rc)

    sizes = [(k1 - k0) * rlen for k0, k1 in batches]
    bed_writer._stream_batches(eng, f, max(sizes), sizes, launch, ms, "sai-geno-writer")
    return status.cpu().numpy()


def convert(vcf_file: str, chr_name: str, out_prefix: str, ploidy: int = 2, haploid_samples: Optional[Sequence[str]] = None,
            samples: Optional[Sequence[str]] = None, start: Optional[int] = None, end: Optional[int] = None, append: bool = False,
            skip_multiallelic: bool = False, geno_format: str = "packed", labels: Optional[Mapping[str, str]] = None) -> dict:  # fmt: skip
    """Write the records of ``chr_name`` (inside [start, end]) of a plain, gzip or bgzip VCF as the EIGENSOFT fileset
    ``out_prefix``; see the module's text for what the fileset promises.  The arguments and the summary are those of
    ``bed_writer.convert``; ``append`` is refused.  ``geno_format`` = "packed" or "transposed"; ``labels`` = sample
    name -> the third column of its ``.ind`` line (default: the name).  Every refusal is a ValueError that names the file
    and the cause and leaves nothing behind."""
    t_all = time.perf_counter()
    vcf_file, chr_name, out_prefix = os.fspath(vcf_file), str(chr_name), os.fspath(out_prefix)
    if out_prefix.endswith(".geno"):
        out_prefix = out_prefix[: -len(".geno")]
    if geno_format not in FORMATS:
        raise ValueError(f"geno_format {geno_format!r}: a .geno is written packed or transposed")
    if append:
        raise ValueError(f"{out_prefix}.geno: --append does not go with --out-eigenstrat, because the counts of a .geno sit in its header record and the "
                         "record length of the transposed form follows from them (write one fileset per chromosome, or use --out-bfile)")  # fmt: skip
    in_file, names, ploidies = bed_writer._samples_to_write(vcf_file, ploidy, samples, haploid_samples, _WORDS)
    target = _Target(out_prefix)
    transposed = geno_format == "transposed"
    ms = dict(read=0.0, site_scan=0.0, encode=0.0, d2h=0.0, write=0.0)
    with bed_writer._calls(vcf_file, chr_name, in_file, names, ploidies, start, end, skip_multiallelic, ms, _WORDS) as calls:
        pos, dos, sites = calls.pos, calls.dos, calls.sites
        if max(len(pos), len(names)) > 9999999:
            raise ValueError(f"{vcf_file}: {len(pos)} records and {len(names)} samples, and the header record of a .geno has seven digits for each count")
        uniform, per_slot = bed_writer._ploidy_arguments(ploidies)
        try:
            t0 = time.perf_counter()
            snp, ind = snp_text(sites.bim_text(calls.skip)), ind_text(names, labels)
            header = header_record(geno_format, len(names), len(pos), ind, snp)
            ms["write"] += (time.perf_counter() - t0) * 1e3
            with target.open_geno(header) as f:
                if calls.host:
                    status = _write_records_host(np.ascontiguousarray(dos), uniform, per_slot, transposed, f, ms, calls.n_threads)
                    dosage_at = lambda k, s: dos[k, s]  # noqa: E731
                else:
                    status = _write_records_device(calls.eng, dos.contiguous(), uniform, per_slot, transposed, f, ms)
                    dosage_at = lambda k, s: dos[k, s].item()  # noqa: E731
                bed_writer._refuse_unfit(vcf_file, status, pos, names, ploidies, dosage_at, row=_WORDS["row"])
                written = f.tell()
            t0 = time.perf_counter()
            target.write_text(snp, ind)
            ms["write"] += (time.perf_counter() - t0) * 1e3
            target.commit()
        except BaseException:
            target.rollback()
            raise
    ms["total"] = (time.perf_counter() - t_all) * 1e3
    return {"rows_written": int(len(pos)), "rows_skipped": int(sites.n_rows - len(pos)), "samples": len(names), "bytes": int(written),
            "ms": {k: round(v, 3) for k, v in ms.items()}}  # fmt: skip
