"""A VCF's calls written as a PLINK 1 fileset (PREFIX.bed + PREFIX.bim + PREFIX.fam): ``sai convert``.

A ``.bed`` holds the genotypes of a VCF in a sixteenth of its bytes, loads an order of magnitude faster and is the
way into ``--layout packed2``.  ``convert`` reads one chromosome (or a range of it) with the VCF readers -- the int8
[record][sample] block every reader returns, left in HBM by ``device_vcf.load_dosage_device`` -- and writes it out:
``sai_bed_encode`` (sai_amd/csrc/plink/bed_encode.hip), the inverse of ``sai_plink_decode``, turns the block into
``.bed`` rows on the GPU, so a quarter of the block's bytes cross PCIe; beside the read a host thread passes over the
text once more for what the readers do not keep -- ID, REF, ALT and the sample names (``sai_vcf_sites_open``,
sai_amd/csrc/plink/vcf_sites.cpp) -- and its positions must be the reader's.  A2 = REF and A1 = ALT, the convention the
fileset reader relies on; no allele is ever swapped by frequency.

What the fileset promises: reading it at the ploidies it was written with gives the block the VCF reader gives for the
same samples, byte for byte, so ``score`` on it writes the same files as ``score`` on the VCF.  The VCF is read without
ancestral alleles; polarisation happens when the fileset is scored, from the ``.bim`` alleles, as it would from the
VCF's.  The table, the rules and the refusals are in DESIGN_INGEST.md ("PLINK 1 filesets written from a VCF").

The entry points are internal to the package: their declarations are in sai_amd/csrc/plink/bed_export.hpp, not
under include/, and this module -- their only caller -- binds them, with a version number of their own.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import os
import queue
import threading
import time
import types
from typing import Optional, Sequence

import numpy as np

from .. import _ffi, _ffi_plink
from .._binding import extension
from . import filesets
from ._ingest import check_io, default_threads
from .vcf import _open_text

SAI_BED_EXPORT_ABI_VERSION = 1
MAGIC = b"\x6c\x1b\x01"
BATCH_BYTES = 8 << 20  # .bed bytes per encoded batch; SAI_AMD_CONVERT_BATCH overrides it

_p, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes): the names sai_amd/csrc/plink/bed_export.hpp declares
SIGNATURES = {
    "sai_bed_export_abi_version": (C.c_int, []),
    "sai_bed_encode_host": (C.c_int, [_p, _i64, _i32, _p, _i32, _p, _p, _i32]),
    "sai_bed_encode": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _p, _p, _p]),
    "sai_vcf_sites_open": (C.c_int, [C.c_char_p, C.c_char_p, _i64, _i64, _i32, C.POINTER(_p)]),
    "sai_vcf_sites_info": (C.c_int, [_p] + [C.POINTER(_i64)] * 4),
    "sai_vcf_sites_copy": (C.c_int, [_p, _p, _p, _p, _p, _p, _p]),
    "sai_vcf_sites_bim": (C.c_int, [_p, _p, _p, _i64, C.POINTER(_i64)]),
    "sai_vcf_sites_close": (C.c_int, [_p]),
}
HOST_SYMBOLS = tuple(n for n in SIGNATURES if n != "sai_bed_encode")

load, load_host = extension("bed export", "sai_amd/csrc/plink/bed_export.hpp", "sai_bed_export_abi_version", SAI_BED_EXPORT_ABI_VERSION,
                            SIGNATURES, HOST_SYMBOLS, built_from="plink")  # fmt: skip


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def encode_host(dosage: np.ndarray, ploidies, n_threads: Optional[int] = None):
    """(rows uint8 [n][ceil(slots / 4)], status int32 [n]) of an int8 [n][slots] block: ``sai_bed_encode_host``.
    ``ploidies`` = 1, 2 or one value per slot."""
    lib = load_host()
    dosage = np.ascontiguousarray(dosage, dtype=np.int8)
    n_rows, n_slots = dosage.shape
    uniform, per_slot = _ploidy_arguments(ploidies)
    rows = np.zeros((n_rows, (n_slots + 3) // 4), dtype=np.uint8)
    status = np.zeros(n_rows, dtype=np.int32)
    check_io(lib, lib.sai_bed_encode_host(_ptr(dosage), n_rows, n_slots, _ptr(per_slot), uniform, _ptr(rows), _ptr(status), n_threads or default_threads()))
    return rows, status


def _ploidy_arguments(ploidies):
    """(uniform_ploidy, int32 array or None) as the encoders take them."""
    if np.ndim(ploidies) == 0:
        return int(ploidies), None
    per_slot = np.ascontiguousarray(ploidies, dtype=np.int32)
    if per_slot.size and bool((per_slot == per_slot[0]).all()) and int(per_slot[0]) in (1, 2):
        return int(per_slot[0]), None
    return 0, per_slot


class SiteColumns:
    """The records of ``chr_name`` inside [start, end] in file order, from one host pass over the text: ``pos`` int32,
    ``multi`` (ALT holds a comma), ``ids`` / ``ref`` / ``alt`` (the first ALT) and ``samples`` (the #CHROM line).
    ``bim_text(skip)`` gives the ``.bim`` lines of the rows that are not skipped."""

    def __init__(self, vcf_file, chr_name, start=None, end=None, n_threads=None):
        self.lib, self.handle = load_host(), C.c_void_p()
        check_io(self.lib, self.lib.sai_vcf_sites_open(os.fsencode(vcf_file), str(chr_name).encode(), -1 if start is None else int(start),
                                                       -1 if end is None else int(end), n_threads or default_threads(), C.byref(self.handle)))  # fmt: skip
        try:
            v = [C.c_int64() for _ in range(4)]
            check_io(self.lib, self.lib.sai_vcf_sites_info(self.handle, *[C.byref(x) for x in v]))
            self.n_rows, n_samples, self._text_bytes, names_bytes = (int(x.value) for x in v)
            self.pos = np.empty(self.n_rows, dtype=np.int32)
            self.multi = np.empty(self.n_rows, dtype=np.uint8)
            name_off, names = np.empty(n_samples + 1, dtype=np.int64), C.create_string_buffer(max(names_bytes, 1))
            check_io(self.lib, self.lib.sai_vcf_sites_copy(self.handle, _ptr(self.pos), _ptr(self.multi), None, None, _ptr(name_off), names))
        except BaseException:  # nobody gets the object, so nobody would close the handle
            self.close()
            raise
        raw = names.raw
        self.samples = [raw[name_off[i] : name_off[i + 1]].decode() for i in range(n_samples)]

    def columns(self):
        """(ids, ref, alt) as lists of str: the tests' view; the converter takes ``bim_text``."""
        off, text = np.empty(3 * self.n_rows + 1, dtype=np.int64), C.create_string_buffer(max(self._text_bytes, 1))
        check_io(self.lib, self.lib.sai_vcf_sites_copy(self.handle, None, None, _ptr(off), text, None, None))
        raw, off = text.raw, off.tolist()
        strings = [raw[off[i] : off[i + 1]].decode() for i in range(3 * self.n_rows)]
        return strings[0::3], strings[1::3], strings[2::3]

    def bim_text(self, skip: Optional[np.ndarray] = None) -> bytes:
        skip = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
        n = C.c_int64()
        check_io(self.lib, self.lib.sai_vcf_sites_bim(self.handle, _ptr(skip), None, 0, C.byref(n)))
        out = C.create_string_buffer(max(int(n.value), 1))
        check_io(self.lib, self.lib.sai_vcf_sites_bim(self.handle, _ptr(skip), out, int(n.value), C.byref(n)))
        return out.raw[: int(n.value)]

    def close(self):
        if self.handle:
            self.lib.sai_vcf_sites_close(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def header_samples(vcf_file) -> list:
    """The sample names of the #CHROM line, in column order."""
    with _open_text(vcf_file) as f:
        for line in f:
            if line.startswith("#CHROM"):
                return line.rstrip("\r\n").split("\t")[9:]
            if not line.startswith("#"):
                break
    raise ValueError(f"{vcf_file}: not a VCF (no #CHROM header)")


def names_of(path) -> list:
    """The first word of every non-empty line: a ``--samples`` / ``--haploid`` file."""
    with open(path) as f:
        return [line.split()[0] for line in f if line.split()]


class _Target:
    """The three files of a conversion.  A new fileset is written under temporary names and renamed at the end; an
    appended one is checked first, and truncated back to the sizes it had on any error."""

    def __init__(self, prefix: str, append: bool, samples: Sequence[str], row_bytes: int):
        self.final = {ext: prefix + ext for ext in (".bed", ".bim", ".fam")}
        self.append = append and any(os.path.exists(p) for p in self.final.values())  # nothing there yet: --append starts the fileset
        if not self.append:
            if os.path.exists(self.final[".bed"]):
                raise ValueError(f"{self.final['.bed']} exists: name another prefix, or add its rows to it with --append")
            self.paths = {ext: f"{p}.tmp{os.getpid()}" for ext, p in self.final.items()}
            self.sizes = None
            return
        for p in self.final.values():
            if not os.path.isfile(p):
                raise ValueError(f"{p} is not found: --append needs the three files of {prefix}")
        with open(self.final[".bed"], "rb") as f:
            magic = f.read(3)
        if magic != MAGIC:
            raise ValueError(f"{self.final['.bed']}: not a variant-major PLINK 1 .bed file (it starts with {magic.hex() or 'nothing'}): nothing is appended to it")
        with open(self.final[".fam"]) as f:
            have = [line.split()[1] for line in f if len(line.split()) > 1]
        if have != list(samples):
            at = next((i for i, (a, b) in enumerate(zip(have, samples)) if a != b), min(len(have), len(samples)))
            raise ValueError(f"{self.final['.fam']} names {len(have)} samples and the conversion {len(samples)}, the first difference at line {at + 1}: "
                             "--append needs the same samples in the same order")  # fmt: skip
        with open(self.final[".bim"], "rb") as f:
            n_lines = sum(1 for line in f if line.strip())
        size = os.path.getsize(self.final[".bed"])
        if size != 3 + n_lines * row_bytes:
            raise ValueError(f"{self.final['.bed']}: {size} bytes, but 3 + {n_lines} variants of the .bim x {row_bytes} bytes for {len(samples)} samples "
                             f"is {3 + n_lines * row_bytes}: nothing is appended to it")  # fmt: skip
        self.paths = dict(self.final)
        self.sizes = {ext: os.path.getsize(p) for ext, p in self.final.items()}

    def open_bed(self):
        if self.append:
            return open(self.paths[".bed"], "ab")
        f = open(self.paths[".bed"], "wb")
        f.write(MAGIC)
        return f

    def write_text(self, bim: bytes, samples: Sequence[str]) -> None:
        with open(self.paths[".bim"], "ab" if self.append else "wb") as f:
            f.write(bim)
        if not self.append:
            with open(self.paths[".fam"], "w") as f:
                f.write("".join(f"{s} {s} 0 0 0 -9\n" for s in samples))

    def commit(self) -> None:
        if not self.append:
            for ext in (".bim", ".fam", ".bed"):  # the .bed last: its presence is what refuses a second conversion
                os.replace(self.paths[ext], self.final[ext])

    def rollback(self) -> None:
        if self.append:
            for ext, size in self.sizes.items():
                try:
                    os.truncate(self.paths[ext], size)
                except OSError:
                    pass
        else:
            for p in self.paths.values():
                if os.path.exists(p):
                    os.remove(p)


def _refuse_unfit(vcf_file, status, pos, samples, ploidies, dosage_at, row=".bed row") -> None:
    """The first flagged row of ``status`` as the converter's ValueError; ``dosage_at(row, slot)`` fetches the value;
    ``row`` names what a row is written as."""
    bad = np.flatnonzero(status)
    if bad.size == 0:
        return
    k, st = int(bad[0]), int(status[bad[0]])
    if st == _ffi_plink.SAI_PLINK_STATUS_BAD_INDEX:
        raise ValueError(f"{vcf_file}: the record at position {int(pos[k])} was encoded with a ploidy other than 1 or 2")
    slot = len(samples) - st
    raise ValueError(
        f"{vcf_file}: the call of sample {samples[slot]} at position {int(pos[k])} has dosage {int(dosage_at(k, slot))} at ploidy {int(ploidies[slot])}: "
        f"a {row} holds 0, 1, 2 or a wholly missing call at ploidy 2 and 0, 1 or a missing call at ploidy 1 "
        "(a half-missing call, a third allele or another ploidy does not fit)"
    )


def _batch_rows(row_bytes: int) -> int:
    """Rows per encoded batch: a multiple of 16, so that every batch of the block starts at a 16-byte boundary."""
    cap = int(os.environ.get("SAI_AMD_CONVERT_BATCH", BATCH_BYTES))
    return max(16, cap // row_bytes // 16 * 16)


def _write_rows_host(dos, uniform, per_slot, target, ms, n_threads):
    """Host route: ``sai_bed_encode_host`` batch by batch, written as it comes.  -> (status, bytes written)"""
    lib = load_host()
    n_rows, n_slots = dos.shape
    row_bytes = (n_slots + 3) // 4
    status = np.zeros(n_rows, dtype=np.int32)
    step, written = _batch_rows(row_bytes), 0
    rows = np.empty((min(step, n_rows), row_bytes), dtype=np.uint8)
    with target.open_bed() as f:
        for k0 in range(0, n_rows, step):
            k1 = min(k0 + step, n_rows)
            t0 = time.perf_counter()
            check_io(lib, lib.sai_bed_encode_host(_ptr(dos[k0:k1]), k1 - k0, n_slots, _ptr(per_slot), uniform, _ptr(rows), _ptr(status[k0:k1]), n_threads))
            t1 = time.perf_counter()
            f.write(memoryview(rows[: k1 - k0]).cast("B"))
            ms["encode"] += (t1 - t0) * 1e3
            ms["write"] += (time.perf_counter() - t1) * 1e3
            written += (k1 - k0) * row_bytes
    return status, written


def _stream_batches(eng, f, cap, sizes, launch, ms, thread_name):
    """The device writers' loop: ``launch(i, out_ptr, side)`` encodes batch i (``sizes[i]`` bytes, at most ``cap``) into
    the device buffer at ``out_ptr`` on the side stream; the bytes are copied into one of two pinned buffers there while
    a thread writes batch i - 1 to ``f`` out of the other.  -> bytes written"""
    import torch

    rows_dev = [torch.empty((cap,), dtype=torch.uint8, device=eng.device) for _ in range(2)]
    pinned = [eng.pinned_acquire(cap) for _ in range(2)]
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))  # the block was written on the current stream
    free = [threading.Semaphore(1), threading.Semaphore(1)]
    jobs, failure, events = queue.Queue(), [], []
    written = 0

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
        thread = threading.Thread(target=writer, name=thread_name)
        thread.start()
        try:
            for i, nbytes in enumerate(sizes):
                b = i & 1
                free[b].acquire()  # the writer has left this pinned buffer
                if failure:
                    free[b].release()
                    break
                marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                with torch.cuda.stream(side):
                    marks[0].record(side)
                    launch(i, C.c_void_p(rows_dev[b].data_ptr()), side)
                    marks[1].record(side)
                    pinned[b][:nbytes].copy_(rows_dev[b][:nbytes], non_blocking=True)
                    marks[2].record(side)
                events.append(marks)
                jobs.put((b, nbytes, marks[2]))
                written += nbytes
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
    return written


def _write_rows_device(eng, dos, uniform, per_slot, target, ms):
    """GPU route: batch k is encoded and copied into one of two pinned buffers on a side stream while a thread writes
    batch k - 1 out of the other (``_stream_batches``).  -> (status, bytes written)"""
    import torch

    lib = eng.lib
    load()
    n_rows, n_slots = dos.shape
    row_bytes = (n_slots + 3) // 4
    step = _batch_rows(row_bytes)
    status = torch.empty((n_rows,), dtype=torch.int32, device=eng.device)
    ploidy_dev = None if per_slot is None else torch.from_numpy(per_slot).to(eng.device)
    starts = list(range(0, n_rows, step))

    def launch(i, out_ptr, side):
        k0 = starts[i]
        k1 = min(k0 + step, n_rows)
        _ffi.check(lib.sai_bed_encode(eng.ctx, C.c_void_p(dos.data_ptr() + k0 * n_slots), k1 - k0, n_slots, eng._ptr(ploidy_dev), uniform,
                                      out_ptr, C.c_void_p(status.data_ptr() + 4 * k0), C.c_void_p(side.cuda_stream)))  # fmt: skip

    with target.open_bed() as f:
        written = _stream_batches(eng, f, min(step, n_rows) * row_bytes, [(min(k0 + step, n_rows) - k0) * row_bytes for k0 in starts], launch, ms,
                                  "sai-bed-writer")  # fmt: skip
    return status.cpu().numpy(), written


# the words a refusal names the output by: the shared steps serve this module, utils/pgen_writer.py and utils/geno_writer.py
_BED_WORDS = dict(fileset="PLINK 1 fileset", sample_file=".fam", row=".bed row")


def _samples_to_write(vcf_file, ploidy, samples, haploid_samples, words):
    """The checks of the input and of the sample lists that come before anything is read or written.
    -> (names of the #CHROM line, names to write, their ploidies)"""
    kind = filesets.name_of(vcf_file)
    if kind is not None:
        raise ValueError(f"{vcf_file} is {kind}, already a binary format: `sai score` reads it as it is; `sai convert` takes VCF text (plain, gzip or bgzip)")
    if ploidy not in (1, 2):
        article = "an" if words["fileset"][0] in "AEIOU" else "a"
        raise ValueError(f"ploidy {ploidy}: {article} {words['fileset']} holds haploid and diploid calls only (--ploidy 1 or 2)")
    if not os.path.isfile(vcf_file):
        raise ValueError(f"{vcf_file} is not found")
    in_file = header_samples(vcf_file)
    names = list(in_file) if samples is None else list(samples)
    haploid = list(haploid_samples or ())
    known = set(in_file)
    missing = [s for s in [*names, *haploid] if s not in known]
    if missing:  # the VCF reader's words: it names the first one
        raise ValueError(f"samples not found in {vcf_file}: {missing[0]}")
    if len(set(names)) != len(names):
        twice = next(s for s in names if names.count(s) > 1)
        raise ValueError(f"sample {twice} is asked for twice: a {words['sample_file']} names a sample once")
    if not names:
        raise ValueError(f"{vcf_file} has no sample to write")
    hap = set(haploid)
    return in_file, names, [1 if s in hap else int(ploidy) for s in names]


@contextlib.contextmanager
def _calls(vcf_file, chr_name, in_file, names, ploidies, start, end, skip_multiallelic, ms, words):
    """The block of the rows to write, read with the VCF readers while a host thread scans the site columns, the two
    checked against each other and the multiallelic records refused or dropped.  Yields an object with ``host``,
    ``eng``, ``n_threads``, ``pos`` and ``dos`` (the rows to write), ``sites`` (every row of the region) and ``skip``;
    the site columns are closed on the way out."""
    host = os.environ.get("SAI_AMD_INGEST") == "host"
    n_threads = default_threads()
    scanned = {}

    def scan():
        t0 = time.perf_counter()
        try:
            scanned["sites"] = SiteColumns(vcf_file, chr_name, start, end, n_threads)
        except Exception as exc:  # noqa: BLE001 - raised by the caller's thread
            scanned["error"] = exc
        ms["site_scan"] = (time.perf_counter() - t0) * 1e3

    scanner = threading.Thread(target=scan, name="sai-vcf-sites")
    scanner.start()
    sites = None
    try:
        try:
            t0 = time.perf_counter()
            if host:
                from .native_vcf import load_dosage

                eng = None
                pos, dos, _, _ = load_dosage(vcf_file, chr_name, names, ploidies, start, end, None, n_threads)
            else:
                import torch

                from ..engine import Engine
                from .device_vcf import load_dosage_device

                eng = Engine.get()
                pos, dos, _, _ = load_dosage_device(eng, vcf_file, chr_name, names, ploidies, start, end, None, n_threads)
                torch.cuda.current_stream(eng.device).synchronize()
            ms["read"] = (time.perf_counter() - t0) * 1e3
        finally:
            scanner.join()
            sites = scanned.get("sites")
        if "error" in scanned:
            raise scanned["error"]
        if sites.samples != in_file:  # the names were needed before the read, which the scan runs beside: it confirms them
            raise RuntimeError(f"{vcf_file}: the site scan found {len(sites.samples)} sample names on the #CHROM line and the header pass "
                               f"{len(in_file)}, or other names: nothing is written")  # fmt: skip
        if sites.n_rows != len(pos) or not np.array_equal(sites.pos, pos):
            differ = next((i for i in range(min(sites.n_rows, len(pos))) if sites.pos[i] != pos[i]), min(sites.n_rows, len(pos)))
            raise RuntimeError(f"{vcf_file}: the site scan found {sites.n_rows} records of chromosome {chr_name} and the genotype reader {len(pos)} "
                               f"(they differ first at record {differ + 1}): nothing is written")  # fmt: skip
        if len(pos) == 0:
            where = "" if start is None and end is None else f" in the region {start}-{end}"
            raise ValueError(f"{vcf_file}: no record of chromosome {chr_name}{where}")
        skip = None
        if sites.multi.any():
            if not skip_multiallelic:
                k = int(np.flatnonzero(sites.multi)[0])
                raise ValueError(f"{vcf_file}: the record at position {int(pos[k])} of chromosome {chr_name} has more than one ALT allele, and a {words['row']} "
                                 f"holds two alleles ({int(sites.multi.sum())} such records: --skip-multiallelic drops and counts them)")  # fmt: skip
            skip = sites.multi
            keep = np.flatnonzero(skip == 0)
            if keep.size == 0:
                raise ValueError(f"{vcf_file}: every record of chromosome {chr_name} has more than one ALT allele: nothing to write")
            pos = pos[keep]
            if host:
                dos = np.ascontiguousarray(dos[keep])
            else:
                dos = dos.index_select(0, torch.from_numpy(keep).to(eng.device))
        yield types.SimpleNamespace(host=host, eng=eng, n_threads=n_threads, pos=pos, dos=dos, sites=sites, skip=skip)
    finally:
        if sites is not None:
            sites.close()


def convert(vcf_file: str, chr_name: str, out_prefix: str, ploidy: int = 2, haploid_samples: Optional[Sequence[str]] = None,
            samples: Optional[Sequence[str]] = None, start: Optional[int] = None, end: Optional[int] = None, append: bool = False,
            skip_multiallelic: bool = False) -> dict:  # fmt: skip
    """Write the records of ``chr_name`` (inside [start, end]) of a plain, gzip or bgzip VCF as the PLINK 1 fileset
    ``out_prefix``; see the module's text for what the fileset promises.  ``samples`` = the names to write, in this
    order (default: every sample of the file in column order); those of ``haploid_samples`` are read at ploidy 1, all
    others at ``ploidy``.  ``append`` adds the rows to an existing fileset of the same samples (22 chromosomes into one
    fileset; a chromosome range by range).  ``skip_multiallelic`` drops and counts the records whose ALT holds a comma
    instead of refusing them.  Returns ``{"rows_written", "rows_skipped", "samples", "bytes", "ms": {phase: ms}}``.
    Every refusal is a ValueError that names the file and the cause and leaves nothing behind."""
    t_all = time.perf_counter()
    vcf_file, chr_name, out_prefix = os.fspath(vcf_file), str(chr_name), os.fspath(out_prefix)
    if out_prefix.endswith(".bed"):
        out_prefix = out_prefix[: -len(".bed")]
    in_file, names, ploidies = _samples_to_write(vcf_file, ploidy, samples, haploid_samples, _BED_WORDS)
    row_bytes = (len(names) + 3) // 4
    target = _Target(out_prefix, append, names, row_bytes)
    ms = dict(read=0.0, site_scan=0.0, encode=0.0, d2h=0.0, write=0.0)
    with _calls(vcf_file, chr_name, in_file, names, ploidies, start, end, skip_multiallelic, ms, _BED_WORDS) as calls:
        pos, dos, sites = calls.pos, calls.dos, calls.sites
        uniform, per_slot = _ploidy_arguments(ploidies)
        try:
            if calls.host:
                status, written = _write_rows_host(np.ascontiguousarray(dos), uniform, per_slot, target, ms, calls.n_threads)
                dosage_at = lambda k, s: dos[k, s]  # noqa: E731
            else:
                status, written = _write_rows_device(calls.eng, dos.contiguous(), uniform, per_slot, target, ms)
                dosage_at = lambda k, s: dos[k, s].item()  # noqa: E731
            _refuse_unfit(vcf_file, status, pos, names, ploidies, dosage_at)
            t0 = time.perf_counter()
            target.write_text(sites.bim_text(calls.skip), names)
            ms["write"] += (time.perf_counter() - t0) * 1e3
            target.commit()
        except BaseException:
            target.rollback()
            raise
    ms["total"] = (time.perf_counter() - t_all) * 1e3
    return {"rows_written": int(len(pos)), "rows_skipped": int(sites.n_rows - len(pos)), "samples": len(names), "bytes": int(written) + (0 if target.append else 3),
            "ms": {k: round(v, 3) for k, v in ms.items()}}  # fmt: skip
