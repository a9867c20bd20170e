"""EIGENSOFT filesets (PREFIX.geno + PREFIX.snp + PREFIX.ind) as an input of ``score``: the text EIGENSTRAT
form, PACKEDANCESTRYMAP and its transposed form.

A packed ``.geno`` holds a genotype in 2 bits, as a PLINK ``.bed`` does, in records of fixed length.  The host
index (``sai_eigenstrat_open``, sai_amd/csrc/eigenstrat/eigenstrat_index.cpp) tells the three encodings apart,
checks the header and the size, resolves the samples and selects the variants; the bytes cross PCIe as they
are and a kernel turns them into the int8 [record][sample] block ``sai_tokenize_gt`` writes for VCF text, so
everything behind the readers is shared with the VCF and the PLINK route.

 * text and packed: a record is a variant.  The selected records are byte ranges (``_ingest.row_batches``, as for
   a ``.bed``) and ``sai_eigenstrat_decode`` recodes them.
 * transposed: a record is an individual.  A batch is a range of variants; for every DISTINCT requested
   individual one ``pread`` brings the bytes of that range into the staging buffer, which is thus already
   gathered by individual, and ``sai_eigenstrat_decode_transposed`` turns the 2-bit matrix.

Column 5 of the ``.snp`` plays REF and column 6 plays ALT; the dosage table, and what is refused, are in
DESIGN_INGEST.md ("EIGENSTRAT filesets").  The surface is that of ``plink``: ``load_dosage`` /
``load_dosage_device`` return what ``native_vcf.load_dosage`` / ``device_vcf.load_dosage_device`` return, and
every request of a (sample, ploidy) is a slot.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from .. import _ffi, _ffi_eigenstrat
from ._ingest import check_io, default_threads, read_batches, region_args, row_batches, staged_copy

BUFFER_BYTES = 32 << 20  # as the other routes; SAI_AMD_INGEST_BUFFER overrides it
_EXTENSIONS = (".geno", ".snp", ".ind")
_READ_THROUGH_BYTES = 64 << 10  # unselected records between two selected ones are read along up to this many bytes
_STRIDE_ALIGN = 16  # the transposed kernel loads a staged record in 128-bit words
TEXT, PACKED, TRANSPOSED = _ffi_eigenstrat.TEXT, _ffi_eigenstrat.PACKED, _ffi_eigenstrat.TRANSPOSED


def _starts_like_geno(head: bytes) -> bool:
    return head[:5] in (b"GENO ", b"GENO\t") or head[:6] in (b"TGENO ", b"TGENO\t") or head[:1] in (b"0", b"1", b"2", b"9")


def fileset_prefix(path) -> Optional[str]:
    """PREFIX when ``path`` (``PREFIX.geno`` or the bare ``PREFIX``) names an EIGENSOFT fileset: the three files
    exist and the ``.geno`` starts as one of the three encodings.  A bare prefix that is also a PLINK fileset
    stays PLINK."""
    if path is None:
        return None
    text = os.fspath(path)
    candidates = ([text[: -len(".geno")]] if text.endswith(".geno") else []) + [text]
    for prefix in candidates:
        if prefix and all(os.path.isfile(prefix + ext) for ext in _EXTENSIONS):
            if prefix == text:
                from .plink import fileset_prefix as plink_prefix

                if plink_prefix(text) is not None:
                    return None
            try:
                with open(prefix + ".geno", "rb") as f:
                    if _starts_like_geno(f.read(6)):
                        return prefix
            except OSError:
                pass
    return None


def is_fileset(path) -> bool:
    return fileset_prefix(path) is not None


def _prefix_of(path) -> str:
    """The prefix a reader hands to the library: the detected one, else the path as a prefix (the library then
    says which file is missing or what is wrong with the ``.geno``)."""
    found = fileset_prefix(path)
    if found is not None:
        return found
    text = os.fspath(path)
    return text[: -len(".geno")] if text.endswith(".geno") else text


def scan_first_last(path, chr_name: str):
    """First and last position of the first contiguous run of ``chr_name`` in the ``.snp`` (None, None if absent):
    ``native_vcf.scan_first_last`` for a fileset."""
    lib = _ffi_eigenstrat.load_host()
    first, last = C.c_int64(-1), C.c_int64(-1)
    check_io(lib, lib.sai_eigenstrat_scan(os.fsencode(_prefix_of(path)), str(chr_name).encode(), C.byref(first), C.byref(last)))
    return (None, None) if first.value < 0 else (int(first.value), int(last.value))


class _Batch:
    """One batch of a read: the rows ``[k0, k1)`` of the index, where each of them lies in the batch
    (``row_in_batch``), the ``pread`` calls that fill the staging buffer (``reads``) and the bytes they fill
    (``nbytes``).  ``n_batch`` is the number of records (variant-major) or variants (transposed) staged;
    ``stride`` the bytes of a staged record and ``first_code`` where the first variant sits in its byte
    (transposed)."""

    __slots__ = ("k0", "k1", "row_in_batch", "n_batch", "reads", "nbytes", "stride", "first_code")

    def __init__(self, k0, k1, row_in_batch, n_batch, reads, nbytes, stride, first_code=0):
        self.k0, self.k1, self.row_in_batch, self.n_batch, self.reads = k0, k1, row_in_batch, n_batch, reads
        self.nbytes, self.stride, self.first_code = nbytes, stride, first_code


class _Index:
    """The host index of one region: positions, the ``.snp`` line and the flip flag of every selected variant,
    the ``.ind`` line of every slot, and how the ``.geno`` is laid out."""

    def __init__(self, lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads):
        self.prefix = _prefix_of(path)
        self.geno = self.prefix + ".geno"
        n, handle = len(samples), C.c_void_p()
        args = region_args(self.prefix, chr_name, start, end, samples, ploidies, anc_allele_file, n_threads)
        check_io(lib, lib.sai_eigenstrat_open(*args, C.byref(handle)))
        try:
            v = [C.c_int64() for _ in range(10)]
            check_io(lib, lib.sai_eigenstrat_index_info(handle, *[C.byref(x) for x in v]))
            (n_rows, self.n_matched, self.n_anc, self.n_ind, self.n_snp, self.first, self.last, self.encoding, self.record_bytes,
             self.data_offset) = (int(x.value) for x in v)  # fmt: skip
            self.pos = np.empty(n_rows, dtype=np.int32)
            self.file_row = np.empty(n_rows, dtype=np.int64)
            self.flip = np.empty(n_rows, dtype=np.uint8)
            self.col_of_slot = np.empty(n, dtype=np.int32)
            arrays = (self.pos, self.file_row, self.flip, self.col_of_slot)
            check_io(lib, lib.sai_eigenstrat_index_copy(handle, *(a.ctypes.data_as(C.c_void_p) for a in arrays)))
        finally:
            lib.sai_eigenstrat_index_close(handle)
        self.samples = list(samples)
        self.ploidies = np.asarray([int(p) for p in ploidies], dtype=np.int32)
        self.n_rows, self.n_slots = n_rows, n
        cols = self.col_of_slot
        self.transposed = self.encoding == TRANSPOSED
        if self.transposed:
            # the staging buffer holds every distinct requested individual once; a slot names its place there
            self.staged_lines, self.staged_of_slot = np.unique(cols, return_inverse=True)
            self.staged_of_slot = np.ascontiguousarray(self.staged_of_slot, dtype=np.int32).reshape(-1)
            self.n_cols = len(self.staged_lines)
            self.first_col = self.uniform_ploidy = -1
        else:
            self.n_cols = self.n_ind
            # the two promises that select the kernel's fast path
            self.first_col = int(cols[0]) if n and np.array_equal(cols, np.arange(cols[0], cols[0] + n, dtype=np.int32)) else -1
            self.uniform_ploidy = int(self.ploidies[0]) if n and bool((self.ploidies == self.ploidies[0]).all()) else 0

    @property
    def cols(self) -> np.ndarray:
        """What the decoders take as ``col_of_slot``: ``.ind`` lines, or places in the staging buffer."""
        return self.staged_of_slot if self.transposed else self.col_of_slot

    def staging_bytes(self, cap: int) -> int:
        """The bytes a staging buffer of this read needs: ``cap``, except that a staged record of the transposed
        form is at least one aligned word long."""
        return max(cap, _STRIDE_ALIGN * self.n_cols) if self.transposed else cap

    def batches(self, cap: int):
        """The read cut into ``_Batch`` es of at most ``cap`` bytes of staging."""
        if self.n_rows == 0 or self.n_slots == 0:
            return
        if not self.transposed:
            size = os.path.getsize(self.geno)  # the last line of a text file may lack its newline
            for k0, k1, rib, n_batch_rows, reads in row_batches(self.file_row, self.record_bytes, self.data_offset, cap,
                                                                _READ_THROUGH_BYTES, self.geno, self.prefix + ".snp"):  # fmt: skip
                if self.encoding == TEXT:  # a packed file has the size the index checked: one that ends early since is a read error
                    reads = [(at, off, min(n, size - off)) for at, off, n in reads]
                yield _Batch(k0, k1, rib, n_batch_rows, reads, n_batch_rows * self.record_bytes, self.record_bytes)
            return
        n_staged = self.n_cols
        if cap < n_staged:
            raise ValueError(f"SAI_AMD_INGEST_BUFFER of {cap} bytes is smaller than one byte for each of the {n_staged} requested "
                             f"individuals of {self.geno}")  # fmt: skip
        if bool((np.diff(self.file_row) <= 0).any()):
            raise ValueError(f"{self.prefix}.snp: the index is not in file order")
        stride = max(_STRIDE_ALIGN, cap // n_staged // _STRIDE_ALIGN * _STRIDE_ALIGN)
        width = 4 * stride - 3  # variants of a batch: they fit the staged bytes wherever the first one sits in its byte
        k0 = 0
        while k0 < self.n_rows:
            s0 = int(self.file_row[k0])
            k1 = int(np.searchsorted(self.file_row, s0 + width))
            s1 = int(self.file_row[k1 - 1]) + 1
            b0, b1 = s0 // 4, -(-s1 // 4)
            reads = [(d * stride, self.data_offset + int(line) * self.record_bytes + b0, b1 - b0) for d, line in enumerate(self.staged_lines)]
            yield _Batch(k0, k1, (self.file_row[k0:k1] - s0).astype(np.int32), s1 - s0, reads, n_staged * stride, stride, s0 & 3)
            k0 = k1

    def staged(self, cap: int):
        """``batches`` as the shared loops take them: ``(reads, bytes staged, batch)``."""
        return ((bt.reads, bt.nbytes, bt) for bt in self.batches(cap))

    def raise_flagged(self, status: np.ndarray, row0: int = 0) -> None:
        """The first flagged row of ``status`` (rows ``row0 ..`` of the index) as the reader's ValueError."""
        bad = np.flatnonzero(status)
        if bad.size == 0:
            return
        k, st = row0 + int(bad[0]), int(status[bad[0]])
        row = int(self.file_row[k])
        if st == _ffi_eigenstrat.SAI_EIGENSTRAT_STATUS_BAD_INDEX:
            raise ValueError(f"{self.geno}: variant {row} was decoded with an index outside its range")
        if st == _ffi_eigenstrat.SAI_EIGENSTRAT_STATUS_BAD_CHAR:
            raise ValueError(f"{self.geno}: line {row + 1} holds a character other than 0, 1, 2 and 9")
        slot = self.n_slots - st
        raise ValueError(
            f"{self.geno}: heterozygous call (one copy of each allele) of sample {self.samples[slot]} at variant {_variant_id(self.prefix, row)} "
            f"(position {int(self.pos[k])}), but the sample is configured with ploidy 1: a fileset has no phase to pick an allele by"
        )


def _variant_id(prefix: str, file_row: int) -> str:
    """Column 1 of record line ``file_row`` of the ``.snp`` (error path only)."""
    try:
        with open(prefix + ".snp", "rb") as f:
            k = -1
            for line in f:
                fields = line.split()
                if fields and not fields[0].startswith(b"#"):
                    k += 1
                    if k == file_row:
                        return fields[0].decode("utf-8", "replace")
    except OSError:
        pass
    return f"#{file_row + 1}"


def _cap(buffer_bytes) -> int:
    return int(buffer_bytes or os.environ.get("SAI_AMD_INGEST_BUFFER", BUFFER_BYTES))


def load_dosage(path, chr_name: str, samples: Sequence[str], ploidies: Sequence[int], start: Optional[int] = None,
                end: Optional[int] = None, anc_allele_file: Optional[str] = None, n_threads: Optional[int] = None,
                buffer_bytes: Optional[int] = None):  # fmt: skip
    """(pos int32 [n], dosage int8 [n][len(samples)], n_matched, n_anc_entries) for one region, decoded on
    the host (``sai_eigenstrat_decode_host``): the ``SAI_AMD_INGEST=host`` route and the yardstick of the kernels."""
    lib = _ffi_eigenstrat.load_host()
    n_threads = n_threads or default_threads()
    idx = _Index(lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads)
    n = idx.n_slots
    dos = np.empty((idx.n_rows, n), dtype=np.int8)
    if n == 0 or idx.n_rows == 0:
        return idx.pos, dos, idx.n_matched, idx.n_anc
    status = np.empty(idx.n_rows, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def decode(buf, bt):
        if bt.k1 > bt.k0:
            check_io(lib, lib.sai_eigenstrat_decode_host(
                idx.encoding, ptr(buf), bt.n_batch, bt.stride, bt.first_code, bt.k1 - bt.k0, ptr(bt.row_in_batch),
                ptr(idx.flip[bt.k0 : bt.k1]), idx.n_cols, n, ptr(idx.cols), ptr(idx.ploidies), ptr(dos[bt.k0 : bt.k1]),
                ptr(status[bt.k0 : bt.k1]), n_threads,
            ))  # fmt: skip

    read_batches(idx.geno, idx.staged(_cap(buffer_bytes)), decode)
    idx.raise_flagged(status)
    return idx.pos, dos, idx.n_matched, idx.n_anc


def release_buffers(eng) -> None:
    """Drop the staging ``load_dosage_device`` keeps between calls."""
    st = eng.__dict__.pop("_eigenstrat_state", None)
    if st:
        st["stream"].synchronize()
        st.clear()


def load_dosage_device(eng, path, chr_name: str, samples: Sequence[str], ploidies: Sequence[int],
                       start: Optional[int] = None, end: Optional[int] = None, anc_allele_file: Optional[str] = None,
                       n_threads: Optional[int] = None, buffer_bytes: Optional[int] = None, trace: Optional[dict] = None):  # fmt: skip
    """(pos int32 host array [n], dosage int8 DEVICE tensor [n][len(samples)], n_matched, n_anc_entries):
    ``load_dosage`` with the result left in HBM.  The bytes of a batch are ``pread`` into two pinned buffers in
    turn, copied on a side stream and decoded behind the copy (``_ingest.staged_copy``), so the file read of batch
    k + 1 runs under the copy and the kernel of batch k.  ``trace`` (a dict) collects host-clock seconds per phase:
    always ``index`` and ``file_read``; with ``trace["serial"]`` set the side stream is synchronised behind every copy
    and every kernel, so ``h2d`` and ``decode`` are timed on their own (and nothing overlaps)."""
    import time

    import torch

    _ffi_eigenstrat.load()
    lib = eng.lib
    t0 = time.perf_counter()
    idx = _Index(lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads)
    if trace is not None:
        trace["index"] = trace.get("index", 0.0) + time.perf_counter() - t0
        trace["geno_bytes"] = 0
        trace["encoding"] = idx.encoding
    n = idx.n_slots
    dos = torch.empty((idx.n_rows, n), dtype=torch.int8, device=eng.device)
    if n == 0 or idx.n_rows == 0:
        return idx.pos, dos, idx.n_matched, idx.n_anc
    cap = _cap(buffer_bytes)
    status = torch.empty((idx.n_rows,), dtype=torch.int32, device=eng.device)
    cols_dev = None if idx.first_col >= 0 else torch.from_numpy(idx.cols).to(eng.device)
    ploidy_dev = None if idx.uniform_ploidy > 0 else torch.from_numpy(idx.ploidies).to(eng.device)

    def launch(rows, bt, side):
        if bt.k1 == bt.k0:
            return None
        d_rib = torch.from_numpy(bt.row_in_batch).to(eng.device, non_blocking=True)
        d_flip = torch.from_numpy(idx.flip[bt.k0 : bt.k1]).to(eng.device, non_blocking=True)
        out_ptr, status_ptr = C.c_void_p(dos.data_ptr()), C.c_void_p(status.data_ptr() + 4 * bt.k0)
        stream_ptr, rows_ptr = C.c_void_p(side.cuda_stream), C.c_void_p(rows)
        if idx.transposed:
            _ffi.check(
                lib.sai_eigenstrat_decode_transposed(eng.ctx, rows_ptr, idx.n_cols, bt.stride, bt.first_code, bt.n_batch, bt.k1 - bt.k0,
                                                     eng._ptr(d_rib), eng._ptr(d_flip), n, eng._ptr(cols_dev), eng._ptr(ploidy_dev),
                                                     out_ptr, bt.k0, status_ptr, stream_ptr)
            )  # fmt: skip
        else:
            _ffi.check(
                lib.sai_eigenstrat_decode(eng.ctx, idx.encoding, rows_ptr, bt.n_batch, bt.stride, bt.k1 - bt.k0, eng._ptr(d_rib),
                                          eng._ptr(d_flip), idx.n_cols, n, eng._ptr(cols_dev), idx.first_col, eng._ptr(ploidy_dev),
                                          idx.uniform_ploidy, out_ptr, bt.k0, status_ptr, stream_ptr)
            )  # fmt: skip
        return d_rib, d_flip

    side = staged_copy(eng, "_eigenstrat_state", idx.staging_bytes(cap), idx.geno, idx.staged(cap), launch, trace, "geno_bytes")
    if bool(status.any()):
        idx.raise_flagged(status.cpu().numpy())
    torch.cuda.current_stream(eng.device).wait_stream(side)
    return idx.pos, dos, idx.n_matched, idx.n_anc
