"""A VCF's calls written as a PLINK 2 fileset (PREFIX.pgen + PREFIX.pvar + PREFIX.psam): ``sai convert --out-pfile``.

A ``.pgen`` holds the hard calls of a panel in a third of the bytes of its ``.bed`` (DESIGN_INGEST.md, "PLINK 2
filesets"): every record takes the smallest of five forms -- dense 2-bit codes, one bit per sample and a list of
exceptions, or a list of the samples that differ from a constant row.  ``convert`` reads one chromosome (or a range of
it) as ``bed_writer.convert`` does -- the sample checks, the read, the site scan beside it and the agreement of the two
are that module's, shared -- and ``sai_pgen_encode`` (sai_amd/csrc/pgen/pgen_encode.hip), the inverse of
``sai_pgen_decode``, chooses and writes the records on the GPU, so only the compressed bytes cross PCIe.  The header's
size follows from the row count alone: records stream to the file from ``header_len`` on, batch by batch, and the block
offsets, record types and record lengths are written over the front at the end.

What the fileset promises is what ``bed_writer`` promises: reading it at the ploidies it was written with gives the
block the VCF reader gives for the same samples, byte for byte.  The format rules were written from memory of the
specification; the output is read back by this project's readers and equals its test writer's, and has not been opened
with plink2.  The table, the size rules and the refusals are in DESIGN_INGEST.md ("PLINK 2 filesets written from a VCF").

With ``ld_compress`` every row but the first of each 16 may also be written as its differences from an earlier row of
its 16 (record types 2 and 3: ``sai_pgen_encode_ld``, sai_amd/csrc/pgen/pgen_encode_ld.hip; the rule is in
sai_amd/csrc/pgen/pgen_export_ld.hpp and DESIGN_INGEST.md, "LD-compressed records").  Neighbouring variants in linkage
disequilibrium are near copies of each other, so such a file is smaller; it promises the same block.  Off by default:
without it nothing here differs from what it was.

The entry points are internal to the package: their declarations are in sai_amd/csrc/pgen/pgen_export.hpp and
pgen_export_ld.hpp, not under include/, and this module -- their only caller -- binds them, with version numbers of
their own.
"""

from __future__ import annotations

import ctypes as C
import os
import queue
import threading
import time
from typing import Optional, Sequence

import numpy as np

from .. import _ffi
from .._binding import extension
from . import bed_writer
from ._ingest import check_io, default_threads

SAI_PGEN_EXPORT_ABI_VERSION = 1
MAGIC = b"\x6c\x1b\x10"  # storage mode 0x10: variable-length records
BLOCK = 65536  # variants of a header block
ENCODE_PLAN, ENCODE_SCAN, ENCODE_WRITE, ENCODE_ALL = 1, 2, 4, 7  # the stages of sai_pgen_encode

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names sai_amd/csrc/pgen/pgen_export.hpp declares
SIGNATURES = {
    "sai_pgen_export_abi_version": (C.c_int, []),
    "sai_pgen_encode_host": (C.c_int, [_p, _i64, _i32, _p, _i32, _p, _i64, _p, _p, _p, C.POINTER(_i64), _i32]),
    "sai_pgen_encode": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _p, _p, _p, _p, _p, _i32, _p]),
    "sai_pgen_encode_grid_cap": (_i64, [_p]),
    "sai_pgen_pvar_lines": (C.c_int, [C.c_char_p, _i64, _p, C.POINTER(_i64)]),
}
HOST_SYMBOLS = ("sai_pgen_export_abi_version", "sai_pgen_encode_host", "sai_pgen_pvar_lines")

load, load_host = extension("pgen export", "sai_amd/csrc/pgen/pgen_export.hpp", "sai_pgen_export_abi_version", SAI_PGEN_EXPORT_ABI_VERSION,
                            SIGNATURES, HOST_SYMBOLS, built_from="pgen")  # fmt: skip

# the LD-compressing encoder: a group of its own, so that the table above stays what pgen_export.hpp declares
SAI_PGEN_EXPORT_LD_VERSION = 1
LD_SEGMENT = 16  # rows of a segment: the first is an anchor, the others may list their differences from an earlier one
LD_SIGNATURES = {
    "sai_pgen_export_ld_version": (C.c_int, []),
    "sai_pgen_ld_segment": (C.c_int, []),
    "sai_pgen_encode_ld_host": SIGNATURES["sai_pgen_encode_host"],
    "sai_pgen_encode_ld": SIGNATURES["sai_pgen_encode"],
}
LD_HOST_SYMBOLS = ("sai_pgen_export_ld_version", "sai_pgen_ld_segment", "sai_pgen_encode_ld_host")

load_ld, load_ld_host = extension("pgen LD export", "sai_amd/csrc/pgen/pgen_export_ld.hpp", "sai_pgen_export_ld_version", SAI_PGEN_EXPORT_LD_VERSION,
                                  LD_SIGNATURES, LD_HOST_SYMBOLS, built_from="pgen")  # fmt: skip

_WORDS = dict(fileset="PLINK 2 fileset", sample_file=".psam", row=".pgen record")
_ptr = bed_writer._ptr


def length_bytes(n_samples: int) -> int:
    """Bytes of a record length in the header: the fewest that hold the dense size, which no record exceeds."""
    return max(1, ((n_samples + 3) // 4).bit_length() + 7 >> 3)


def header_len(n_rows: int, n_samples: int) -> int:
    """Bytes before the first record: they follow from the counts alone."""
    n_blocks = -(-n_rows // BLOCK)
    return 12 + 8 * n_blocks + sum((c + 1) // 2 + c * length_bytes(n_samples) for c in (min(BLOCK, n_rows - b * BLOCK) for b in range(n_blocks)))


def assemble_header(n_samples: int, vrtypes: np.ndarray, lengths: np.ndarray) -> bytes:
    """Everything before the first record: magic and storage mode, the counts, the control byte (4-bit vrtypes, no
    allele counts, no flags), one uint64 file offset per block of 65 536 variants, then block by block the vrtype
    nibbles and the record lengths."""
    vrtypes, lengths = np.asarray(vrtypes, dtype=np.uint8), np.asarray(lengths, dtype=np.uint64)
    n_rows, lb = len(vrtypes), length_bytes(n_samples)
    start = header_len(n_rows, n_samples)
    ends = np.cumsum(lengths, dtype=np.uint64)
    parts = [MAGIC, n_rows.to_bytes(4, "little"), int(n_samples).to_bytes(4, "little"), bytes([lb - 1])]
    parts += [(start + (int(ends[b - 1]) if b else 0)).to_bytes(8, "little") for b in range(0, n_rows, BLOCK)]
    for b in range(0, n_rows, BLOCK):
        vt = vrtypes[b : b + BLOCK]
        nib = np.zeros(len(vt) + (len(vt) & 1), dtype=np.uint8)
        nib[: len(vt)] = vt & 15
        parts.append((nib[0::2] | nib[1::2] << 4).astype(np.uint8).tobytes())
        parts.append(lengths[b : b + BLOCK].astype("<u8").view(np.uint8).reshape(-1, 8)[:, :lb].tobytes())
    head = b"".join(parts)
    assert len(head) == start
    return head


def _host_encoder(ld_compress: bool):
    """``sai_pgen_encode_host``, or with ``ld_compress`` ``sai_pgen_encode_ld_host``, and the library that holds it."""
    if ld_compress:
        lib = load_ld_host()
        if lib.sai_pgen_ld_segment() != LD_SEGMENT:
            raise RuntimeError(f"libsaihip: LD segments of {lib.sai_pgen_ld_segment()} rows, and this module expects {LD_SEGMENT}")
        return lib, lib.sai_pgen_encode_ld_host
    lib = load_host()
    return lib, lib.sai_pgen_encode_host


def encode_host(dosage: np.ndarray, ploidies, n_threads: Optional[int] = None, ld_compress: bool = False):
    """(records uint8 [total], vrtype uint8 [n], length uint32 [n], status int32 [n]) of an int8 [n][slots] block:
    ``sai_pgen_encode_host``, with ``ld_compress`` ``sai_pgen_encode_ld_host``.  ``ploidies`` = 1, 2 or one value per
    slot."""
    lib, encode = _host_encoder(ld_compress)
    dosage = np.ascontiguousarray(dosage, dtype=np.int8)
    n_rows, n_slots = dosage.shape
    uniform, per_slot = bed_writer._ploidy_arguments(ploidies)
    out = np.empty(n_rows * ((n_slots + 3) // 4), dtype=np.uint8)
    vrtype, length, status = np.zeros(n_rows, dtype=np.uint8), np.zeros(n_rows, dtype=np.uint32), np.zeros(n_rows, dtype=np.int32)
    total = _i64()
    check_io(lib, encode(_ptr(dosage), n_rows, n_slots, _ptr(per_slot), uniform, _ptr(out), out.size, _ptr(vrtype), _ptr(length), _ptr(status),
                         C.byref(total), n_threads or default_threads()))  # fmt: skip
    return out[: total.value], vrtype, length, status


class _Target:
    """The three files of a conversion, written under temporary names and renamed at the end."""

    def __init__(self, prefix: str):
        self.final = {ext: prefix + ext for ext in (".pgen", ".pvar", ".psam")}
        if os.path.exists(self.final[".pgen"]):
            raise ValueError(f"{self.final['.pgen']} exists: name another prefix (nothing is appended to a .pgen: its record table sits at the front of the file)")
        self.paths = {ext: f"{p}.tmp{os.getpid()}" for ext, p in self.final.items()}

    def open_pgen(self, first_record_at: int):
        f = open(self.paths[".pgen"], "wb")
        f.seek(first_record_at)
        return f

    def write_text(self, pvar: bytes, samples: Sequence[str]) -> None:
        with open(self.paths[".pvar"], "wb") as f:
            f.write(b"#CHROM\tPOS\tID\tREF\tALT\n")
            f.write(pvar)
        with open(self.paths[".psam"], "w") as f:
            f.write("#IID\tSEX\n" + "".join(f"{s}\tNA\n" for s in samples))

    def commit(self) -> None:
        for ext in (".pvar", ".psam", ".pgen"):  # the .pgen last: its presence is what refuses a second conversion
            os.replace(self.paths[ext], self.final[ext])

    def rollback(self) -> None:
        for p in self.paths.values():
            if os.path.exists(p):
                os.remove(p)


def pvar_text(bim: bytes) -> bytes:
    """The ``.pvar`` lines "CHROM POS ID REF ALT" of the ``.bim`` lines "CHROM ID 0 POS ALT REF" the site columns give
    (``sai_pgen_pvar_lines``: one pass in C; in Python 200 000 lines cost more than the whole conversion)."""
    lib = load_host()
    out, n = C.create_string_buffer(max(len(bim), 1)), _i64()
    check_io(lib, lib.sai_pgen_pvar_lines(bim, len(bim), out, C.byref(n)))
    return out.raw[: n.value]


def _write_records_host(dos, uniform, per_slot, f, ms, n_threads, ld_compress=False):
    """Host route: ``sai_pgen_encode_host`` (``sai_pgen_encode_ld_host``) batch by batch, written as it comes.  A batch
    is a multiple of 16 rows, so the LD segments of a file do not depend on it.  -> (vrtype, length, status)"""
    lib, encode = _host_encoder(ld_compress)
    n_rows, n_slots = dos.shape
    row_bytes = (n_slots + 3) // 4
    vrtype, length, status = np.zeros(n_rows, dtype=np.uint8), np.zeros(n_rows, dtype=np.uint32), np.zeros(n_rows, dtype=np.int32)
    step = bed_writer._batch_rows(row_bytes)
    out = np.empty(min(step, n_rows) * row_bytes, dtype=np.uint8)
    total = _i64()
    for k0 in range(0, n_rows, step):
        k1 = min(k0 + step, n_rows)
        t0 = time.perf_counter()
        check_io(lib, encode(_ptr(dos[k0:k1]), k1 - k0, n_slots, _ptr(per_slot), uniform, _ptr(out), out.size, _ptr(vrtype[k0:k1]), _ptr(length[k0:k1]),
                             _ptr(status[k0:k1]), C.byref(total), n_threads))  # fmt: skip
        t1 = time.perf_counter()
        f.write(memoryview(out)[: total.value])
        ms["encode"] += (t1 - t0) * 1e3
        ms["write"] += (time.perf_counter() - t1) * 1e3
    return vrtype, length, status


def _write_records_device(eng, dos, uniform, per_slot, f, ms, ld_compress=False):
    """GPU route, shaped like ``bed_writer._write_rows_device``: batch k is planned, scanned and written into a device
    buffer on a side stream, its total comes back (four bytes, the one wait of the batch), that many bytes are copied
    into one of two pinned buffers, and a thread writes batch k - 1 out of the other meanwhile.  The record types,
    lengths and status values stay on the device until the last batch.  ``ld_compress``: ``sai_pgen_encode_ld``.
    -> (vrtype, length, status)"""
    import torch

    lib = eng.lib
    load()
    encode = lib.sai_pgen_encode
    if ld_compress:
        load_ld()
        if lib.sai_pgen_ld_segment() != LD_SEGMENT:
            raise RuntimeError(f"libsaihip: LD segments of {lib.sai_pgen_ld_segment()} rows, and this module expects {LD_SEGMENT}")
        encode = lib.sai_pgen_encode_ld
    n_rows, n_slots = dos.shape
    row_bytes = (n_slots + 3) // 4
    step = bed_writer._batch_rows(row_bytes)
    cap = min(step, n_rows) * row_bytes  # the dense upper bound of a batch
    vrtype = torch.empty((n_rows,), dtype=torch.uint8, device=eng.device)
    length = torch.empty((n_rows,), dtype=torch.int32, device=eng.device)
    status = torch.empty((n_rows,), dtype=torch.int32, device=eng.device)
    ploidy_dev = None if per_slot is None else torch.from_numpy(per_slot).to(eng.device)
    rec_dev = [torch.empty((cap,), dtype=torch.uint8, device=eng.device) for _ in range(2)]
    off_dev = [torch.empty((min(step, n_rows) + 1,), dtype=torch.int32, device=eng.device) for _ in range(2)]
    pinned = [eng.pinned_acquire(cap) for _ in range(2)]
    totals = torch.empty((2,), dtype=torch.int32).pin_memory()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))  # the block was written on the current stream
    free = [threading.Semaphore(1), threading.Semaphore(1)]
    jobs, failure, events = queue.Queue(), [], []

    def writer():
        while True:
            job = jobs.get()
            if job is None:
                return
            b, nbytes, copied = job
            try:
                if not failure:
                    copied.synchronize()
                    t0 = time.perf_counter()
                    f.write(memoryview(pinned[b].numpy())[:nbytes])
                    ms["write"] += (time.perf_counter() - t0) * 1e3
            except Exception as exc:  # noqa: BLE001 - reported by the caller's thread
                failure.append(exc)
            finally:
                free[b].release()

    try:
        thread = threading.Thread(target=writer, name="sai-pgen-writer")
        thread.start()
        try:
            for i, k0 in enumerate(range(0, n_rows, step)):
                k1, b = min(k0 + step, n_rows), i & 1
                free[b].acquire()  # the writer has left this pinned buffer
                if failure:
                    free[b].release()
                    break
                marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                with torch.cuda.stream(side):
                    marks[0].record(side)
                    _ffi.check(encode(eng.ctx, C.c_void_p(dos.data_ptr() + k0 * n_slots), k1 - k0, n_slots, eng._ptr(ploidy_dev), uniform,
                                      C.c_void_p(rec_dev[b].data_ptr()), C.c_void_p(vrtype.data_ptr() + k0), C.c_void_p(length.data_ptr() + 4 * k0),
                                      C.c_void_p(off_dev[b].data_ptr()), C.c_void_p(status.data_ptr() + 4 * k0), ENCODE_ALL, C.c_void_p(side.cuda_stream)))  # fmt: skip
                    totals[b : b + 1].copy_(off_dev[b][k1 - k0 : k1 - k0 + 1], non_blocking=True)
                    marks[1].record(side)
                    marks[1].synchronize()
                    nbytes = int(totals[b]) & 0xFFFFFFFF
                    if nbytes > (k1 - k0) * row_bytes:
                        raise RuntimeError(f"sai_pgen_encode: {nbytes} bytes of records for {k1 - k0} rows of at most {row_bytes} bytes")
                    pinned[b][:nbytes].copy_(rec_dev[b][:nbytes], non_blocking=True)
                    marks[2].record(side)
                events.append(marks)
                jobs.put((b, nbytes, marks[2]))
        finally:
            jobs.put(None)
            thread.join()
            side.synchronize()
        if failure:
            raise failure[0]
    finally:
        for buf in pinned:
            eng.pinned_release(buf, (side,))
    for start, encoded, copied in events:
        ms["encode"] += start.elapsed_time(encoded)
        ms["d2h"] += encoded.elapsed_time(copied)
    torch.cuda.current_stream(eng.device).wait_stream(side)
    t0 = time.perf_counter()
    tables = vrtype.cpu().numpy(), length.cpu().numpy().view(np.uint32), status.cpu().numpy()
    ms["d2h"] += (time.perf_counter() - t0) * 1e3
    return tables


def convert(vcf_file: str, chr_name: str, out_prefix: str, ploidy: int = 2, haploid_samples: Optional[Sequence[str]] = None,
            samples: Optional[Sequence[str]] = None, start: Optional[int] = None, end: Optional[int] = None, append: bool = False,
            skip_multiallelic: bool = False, ld_compress: bool = False) -> dict:  # fmt: skip
    """Write the records of ``chr_name`` (inside [start, end]) of a plain, gzip or bgzip VCF as the PLINK 2 fileset
    ``out_prefix``; see the module's text for what the fileset promises.  The arguments and the summary are those of
    ``bed_writer.convert``; ``append`` is refused.  ``ld_compress`` also writes record types 2 and 3 (the module's text),
    and the summary then gains ``"record_types"``: record type -> how many records took it.  Every refusal is a ValueError that names the file and the cause and
    leaves nothing behind."""
    t_all = time.perf_counter()
    vcf_file, chr_name, out_prefix = os.fspath(vcf_file), str(chr_name), os.fspath(out_prefix)
    if out_prefix.endswith(".pgen"):
        out_prefix = out_prefix[: -len(".pgen")]
    if append:
        raise ValueError(f"{out_prefix}.pgen: --append does not go with --out-pfile, because the record table of a .pgen sits at the front of the file "
                         "(write one fileset per chromosome, or use --out-bfile)")  # fmt: skip
    in_file, names, ploidies = bed_writer._samples_to_write(vcf_file, ploidy, samples, haploid_samples, _WORDS)
    target = _Target(out_prefix)
    ms = dict(read=0.0, site_scan=0.0, encode=0.0, d2h=0.0, write=0.0)
    with bed_writer._calls(vcf_file, chr_name, in_file, names, ploidies, start, end, skip_multiallelic, ms, _WORDS) as calls:
        pos, dos, sites = calls.pos, calls.dos, calls.sites
        if len(pos) >= 1 << 32:
            raise ValueError(f"{vcf_file}: {len(pos)} records of chromosome {chr_name}, and the header of a .pgen counts its variants in 32 bits")
        uniform, per_slot = bed_writer._ploidy_arguments(ploidies)
        first = header_len(len(pos), len(names))
        try:
            with target.open_pgen(first) as f:
                if calls.host:
                    vrtype, length, status = _write_records_host(np.ascontiguousarray(dos), uniform, per_slot, f, ms, calls.n_threads, ld_compress)
                    dosage_at = lambda k, s: dos[k, s]  # noqa: E731
                else:
                    vrtype, length, status = _write_records_device(calls.eng, dos.contiguous(), uniform, per_slot, f, ms, ld_compress)
                    dosage_at = lambda k, s: dos[k, s].item()  # noqa: E731
                bed_writer._refuse_unfit(vcf_file, status, pos, names, ploidies, dosage_at, row=_WORDS["row"])
                t0 = time.perf_counter()
                written = f.tell()
                f.seek(0)
                f.write(assemble_header(len(names), vrtype, length))
            target.write_text(pvar_text(sites.bim_text(calls.skip)), names)
            ms["write"] += (time.perf_counter() - t0) * 1e3
            target.commit()
        except BaseException:
            target.rollback()
            raise
    ms["total"] = (time.perf_counter() - t_all) * 1e3
    summary = {"rows_written": int(len(pos)), "rows_skipped": int(sites.n_rows - len(pos)), "samples": len(names), "bytes": int(written),
               "ms": {k: round(v, 3) for k, v in ms.items()}}  # fmt: skip
    if ld_compress:
        summary["record_types"] = {int(t): int(c) for t, c in zip(*np.unique(np.asarray(vrtype), return_counts=True))}
    return summary
