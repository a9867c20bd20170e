"""PLINK 1 binary filesets (PREFIX.bed + PREFIX.bim + PREFIX.fam) as an input of ``score``.

A ``.bed`` holds a genotype in 2 bits -- 16 times fewer bytes than VCF text -- in rows of fixed length, so
the rows of a region are byte ranges that follow from the ``.bim`` alone.  The host index
(``sai_plink_open``, sai_amd/csrc/plink/plink_index.cpp) resolves the samples and selects the rows; the
``.bed`` bytes cross PCIe as they are and ``sai_plink_decode`` turns them into the int8
[record][sample] block ``sai_tokenize_gt`` writes for VCF text, so everything behind the readers is
shared with the VCF route.  A2 plays REF and A1 plays ALT; the dosage table, and what is refused, are
in DESIGN_INGEST.md ("PLINK 1 filesets").

``load_dosage`` / ``load_dosage_device`` return what ``native_vcf.load_dosage`` /
``device_vcf.load_dosage_device`` return.  Unlike a VCF pass, one pass serves a sample that is asked
for more than once (a sample that sits in populations of different ploidy): every request is a slot.

``load_packed`` / ``load_packed_device`` take the populations of a run and decode the same rows straight
into one packed2 block per population (``sai_bed_pack2``, include/saihip_packed_ingest.h): two bits per
call from the file to the site pass, no int8 block in between (DESIGN_INGEST.md, "PLINK 1 filesets in
the 2-bit layout").
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from .. import _ffi, _ffi_packed_ingest, _ffi_plink
from ._ingest import check_io, default_threads, read_batches, region_args, row_batches, staged_copy
from ._packed import _PackedPlan, _packed_bytes

BUFFER_BYTES = 32 << 20  # as the VCF route (device_vcf.BUFFER_BYTES); SAI_AMD_INGEST_BUFFER overrides it
_MAGIC = b"\x6c\x1b"
_EXTENSIONS = (".bed", ".bim", ".fam")
_READ_THROUGH_BYTES = 64 << 10  # unselected rows between two selected ones are read along up to this many bytes


def fileset_prefix(path) -> Optional[str]:
    """PREFIX when ``path`` (``PREFIX.bed`` or the bare ``PREFIX``) names a PLINK 1 fileset: the three
    files exist and the ``.bed`` starts with PLINK's magic bytes.  By content, never by the extension
    alone -- ``.bed`` is also what ancestral-allele files are called."""
    if path is None:
        return None
    text = os.fspath(path)
    candidates = ([text[: -len(".bed")]] if text.endswith(".bed") else []) + [text]
    for prefix in candidates:
        if prefix and all(os.path.isfile(prefix + ext) for ext in _EXTENSIONS):
            try:
                with open(prefix + ".bed", "rb") as f:
                    if f.read(2) == _MAGIC:
                        return prefix
            except OSError:
                pass
    return None


def is_fileset(path) -> bool:
    return fileset_prefix(path) is not None


def _prefix_of(path) -> str:
    """The prefix a reader hands to the library: the detected one, else the path as a prefix (the library
    then says which file is missing or what is wrong with the ``.bed``)."""
    found = fileset_prefix(path)
    if found is not None:
        return found
    text = os.fspath(path)
    return text[: -len(".bed")] if text.endswith(".bed") else text


def scan_first_last(path, chr_name: str):
    """First and last position of the first contiguous run of ``chr_name`` in the ``.bim`` (None, None if
    absent): ``native_vcf.scan_first_last`` for a fileset."""
    lib = _ffi_plink.load_host()
    first, last = C.c_int64(-1), C.c_int64(-1)
    check_io(lib, lib.sai_plink_scan(os.fsencode(_prefix_of(path)), str(chr_name).encode(), C.byref(first), C.byref(last)))
    return (None, None) if first.value < 0 else (int(first.value), int(last.value))


class _Index:
    """The host index of one region: positions, the ``.bed`` row and the flip flag of every selected row,
    the ``.fam`` column of every slot."""

    def __init__(self, lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads):
        self.prefix = _prefix_of(path)
        n, handle = len(samples), C.c_void_p()
        args = region_args(self.prefix, chr_name, start, end, samples, ploidies, anc_allele_file, n_threads)
        check_io(lib, lib.sai_plink_open(*args, C.byref(handle)))
        try:
            v = [C.c_int64() for _ in range(8)]
            check_io(lib, lib.sai_plink_index_info(handle, *[C.byref(x) for x in v]))
            n_rows, self.n_matched, self.n_anc, self.row_bytes, self.n_fam, self.n_bim, self.first, self.last = (int(x.value) for x in v)
            self.pos = np.empty(n_rows, dtype=np.int32)
            self.file_row = np.empty(n_rows, dtype=np.int64)
            self.flip = np.empty(n_rows, dtype=np.uint8)
            self.col_of_slot = np.empty(n, dtype=np.int32)
            arrays = (self.pos, self.file_row, self.flip, self.col_of_slot)
            check_io(lib, lib.sai_plink_index_copy(handle, *(a.ctypes.data_as(C.c_void_p) for a in arrays)))
        finally:
            lib.sai_plink_index_close(handle)
        self.samples = list(samples)
        self.ploidies = np.asarray([int(p) for p in ploidies], dtype=np.int32)
        self.n_rows, self.n_slots = n_rows, n
        cols = self.col_of_slot
        # the two promises that select the kernel's fast path
        self.first_col = int(cols[0]) if n and np.array_equal(cols, np.arange(cols[0], cols[0] + n, dtype=np.int32)) else -1
        self.uniform_ploidy = int(self.ploidies[0]) if n and bool((self.ploidies == self.ploidies[0]).all()) else 0

    def batches(self, cap: int):
        """Cut the selected rows into batches of at most ``cap`` bytes of whole rows.  Selected rows that are
        close in the file are read as one range, the few rows between them included (a ``pread`` per row
        would cost more than their bytes); the ranges of a batch lie back to back in its buffer.  Yields
        ``(k0, k1, row_in_batch int32 [k1 - k0], n_batch_rows, reads)`` with ``reads`` = [(buffer offset,
        file offset, bytes)]."""
        return row_batches(self.file_row, self.row_bytes, 3, cap, _READ_THROUGH_BYTES, f"{self.prefix}.bed", f"{self.prefix}.bim")

    def staged(self, cap: int):
        """``batches`` as the shared loops take them: ``(reads, bytes staged, batch)``."""
        return ((bt[4], bt[3] * self.row_bytes, bt) for bt in self.batches(cap))

    def raise_flagged(self, status: np.ndarray, row0: int = 0) -> None:
        """The first flagged row of ``status`` (rows ``row0 ..`` of the index) as the reader's ValueError."""
        bad = np.flatnonzero(status)
        if bad.size == 0:
            return
        k, st = row0 + int(bad[0]), int(status[bad[0]])
        if st == _ffi_plink.SAI_PLINK_STATUS_BAD_INDEX:
            raise ValueError(f"{self.prefix}.bed: row {int(self.file_row[k])} was decoded with an index outside its range")
        slot = self.n_slots - st
        raise ValueError(
            f"{self.prefix}.bed: heterozygous call of sample {self.samples[slot]} at variant {_variant_id(self.prefix, int(self.file_row[k]))} "
            f"(position {int(self.pos[k])}), but the sample is configured with ploidy 1: a fileset has no phase to pick an allele by"
        )


def _variant_id(prefix: str, file_row: int) -> str:
    """Column 2 of record line ``file_row`` of the ``.bim`` (error path only)."""
    try:
        with open(prefix + ".bim", "rb") as f:
            k = -1
            for line in f:
                fields = line.split()
                if fields:
                    k += 1
                    if k == file_row:
                        return fields[1].decode("utf-8", "replace")
    except (OSError, IndexError):
        pass
    return f"#{file_row + 1}"


def _cap(buffer_bytes) -> int:
    return int(buffer_bytes or os.environ.get("SAI_AMD_INGEST_BUFFER", BUFFER_BYTES))


def load_dosage(path, chr_name: str, samples: Sequence[str], ploidies: Sequence[int], start: Optional[int] = None,
                end: Optional[int] = None, anc_allele_file: Optional[str] = None, n_threads: Optional[int] = None,
                buffer_bytes: Optional[int] = None):  # fmt: skip
    """(pos int32 [n], dosage int8 [n][len(samples)], n_matched, n_anc_entries) for one region, decoded on
    the host (``sai_plink_decode_host``): the ``SAI_AMD_INGEST=host`` route and the yardstick of the kernel."""
    lib = _ffi_plink.load_host()
    n_threads = n_threads or default_threads()
    idx = _Index(lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads)
    n = idx.n_slots
    dos = np.empty((idx.n_rows, n), dtype=np.int8)
    if n == 0 or idx.n_rows == 0:
        return idx.pos, dos, idx.n_matched, idx.n_anc
    status = np.empty(idx.n_rows, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def decode(buf, batch):
        k0, k1, rib, n_batch_rows, _ = batch
        if k1 > k0:
            check_io(lib, lib.sai_plink_decode_host(
                ptr(buf), n_batch_rows, idx.row_bytes, k1 - k0, ptr(rib), ptr(idx.flip[k0:k1]), idx.n_fam, n, ptr(idx.col_of_slot),
                ptr(idx.ploidies), ptr(dos[k0:k1]), ptr(status[k0:k1]), n_threads,
            ))  # fmt: skip

    read_batches(idx.prefix + ".bed", idx.staged(_cap(buffer_bytes)), decode)
    idx.raise_flagged(status)
    return idx.pos, dos, idx.n_matched, idx.n_anc


def release_buffers(eng) -> None:
    """Drop the staging ``load_dosage_device`` keeps between calls."""
    st = eng.__dict__.pop("_plink_state", None)
    if st:
        st["stream"].synchronize()
        st.clear()


def load_dosage_device(eng, path, chr_name: str, samples: Sequence[str], ploidies: Sequence[int],
                       start: Optional[int] = None, end: Optional[int] = None, anc_allele_file: Optional[str] = None,
                       n_threads: Optional[int] = None, buffer_bytes: Optional[int] = None, trace: Optional[dict] = None):  # fmt: skip
    """(pos int32 host array [n], dosage int8 DEVICE tensor [n][len(samples)], n_matched, n_anc_entries):
    ``load_dosage`` with the result left in HBM.  The selected rows are ``pread`` into two pinned buffers in
    turn, copied on a side stream and decoded behind the copy (``_ingest.staged_copy``), so the file read of
    batch k + 1 runs under the copy and the kernel of batch k.  ``trace`` (a dict) collects host-clock seconds per
    phase: always ``index`` and ``file_read``; with ``trace["serial"]`` set the side stream is synchronised behind
    every copy and every kernel, so ``h2d`` and ``decode`` are timed on their own (and nothing overlaps)."""
    import time

    import torch

    _ffi_plink.load()
    lib = eng.lib
    t0 = time.perf_counter()
    idx = _Index(lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads)
    if trace is not None:
        trace["index"] = trace.get("index", 0.0) + time.perf_counter() - t0
        trace["bed_bytes"] = 0
    n = idx.n_slots
    dos = torch.empty((idx.n_rows, n), dtype=torch.int8, device=eng.device)
    if n == 0 or idx.n_rows == 0:
        return idx.pos, dos, idx.n_matched, idx.n_anc
    cap = _cap(buffer_bytes)
    status = torch.empty((idx.n_rows,), dtype=torch.int32, device=eng.device)
    cols_dev = None if idx.first_col >= 0 else torch.from_numpy(idx.col_of_slot).to(eng.device)
    ploidy_dev = None if idx.uniform_ploidy else torch.from_numpy(idx.ploidies).to(eng.device)

    def launch(rows_ptr, batch, side):
        k0, k1, rib, n_batch_rows, _ = batch
        if k1 == k0:
            return None
        d_rib = torch.from_numpy(rib).to(eng.device, non_blocking=True)
        d_flip = torch.from_numpy(idx.flip[k0:k1]).to(eng.device, non_blocking=True)
        _ffi.check(
            lib.sai_plink_decode(eng.ctx, C.c_void_p(rows_ptr), n_batch_rows, idx.row_bytes, k1 - k0, eng._ptr(d_rib), eng._ptr(d_flip),
                                 idx.n_fam, n, eng._ptr(cols_dev), idx.first_col, eng._ptr(ploidy_dev), idx.uniform_ploidy,
                                 C.c_void_p(dos.data_ptr()), k0, C.c_void_p(status.data_ptr() + 4 * k0), C.c_void_p(side.cuda_stream))
        )  # fmt: skip
        return d_rib, d_flip

    side = staged_copy(eng, "_plink_state", cap, idx.prefix + ".bed", idx.staged(cap), launch, trace, "bed_bytes")
    if bool(status.any()):
        idx.raise_flagged(status.cpu().numpy())
    torch.cuda.current_stream(eng.device).wait_stream(side)
    return idx.pos, dos, idx.n_matched, idx.n_anc


_WHOLE_ROW = (_ffi_plink.SAI_PLINK_STATUS_BAD_INDEX,)  # the status codes that stand for a row, not for one of its slots


def _packed_plan(lib, path, chr_name, populations, start, end, anc_allele_file, n_threads) -> _PackedPlan:
    return _PackedPlan(lambda samples, ploidies: _Index(lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads),
                       populations, _WHOLE_ROW, ".bed", _variant_id)  # fmt: skip


def load_packed(path, chr_name: str, populations, start: Optional[int] = None, end: Optional[int] = None,
                anc_allele_file: Optional[str] = None, n_threads: Optional[int] = None, buffer_bytes: Optional[int] = None):  # fmt: skip
    """(pos int32 [n], [uint8 array of ``sai_packed2_bytes(n, len(names))`` bytes per population], n_matched,
    n_anc_entries) for one region, decoded on the host (``sai_bed_pack2_host``): the yardstick of
    ``load_packed_device``.  ``populations`` = [(sample names, ploidy)]."""
    lib = _ffi_packed_ingest.load_host()
    _ffi_plink.load_host()
    n_threads = n_threads or default_threads()
    plan = _packed_plan(lib, path, chr_name, populations, start, end, anc_allele_file, n_threads)
    idx = plan.idx
    blocks = [np.zeros(_packed_bytes(idx.n_rows, pop["n_ind"]), dtype=np.uint8) for pop in plan.pops]
    if idx.n_slots == 0 or idx.n_rows == 0:
        return idx.pos, blocks, idx.n_matched, idx.n_anc
    status = [np.zeros(idx.n_rows, dtype=np.int32) for _ in plan.pops]
    unfit = [np.zeros(idx.n_rows, dtype=np.int32) for _ in plan.pops]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def decode(buf, batch):
        k0, k1, rib, n_batch_rows, _ = batch
        for p, pop in enumerate(plan.pops):
            if k1 > k0 and pop["n_ind"]:
                check_io(lib, lib.sai_bed_pack2_host(
                    ptr(buf), n_batch_rows, idx.row_bytes, k1 - k0, ptr(rib), ptr(idx.flip[k0:k1]), idx.n_fam, pop["n_ind"],
                    ptr(pop["cols"]), pop["first_col"], pop["ploidy"], ptr(blocks[p]), idx.n_rows, k0, ptr(status[p][k0:k1]),
                    ptr(unfit[p][k0:k1]), n_threads,
                ))  # fmt: skip

    read_batches(idx.prefix + ".bed", idx.staged(_cap(buffer_bytes)), decode)
    plan.raise_flagged(status, unfit)
    return idx.pos, blocks, idx.n_matched, idx.n_anc


def load_packed_device(eng, path, chr_name: str, populations, start: Optional[int] = None, end: Optional[int] = None,
                       anc_allele_file: Optional[str] = None, n_threads: Optional[int] = None, buffer_bytes: Optional[int] = None,
                       trace: Optional[dict] = None):  # fmt: skip
    """(pos int32 host array [n], [PackedPop per population], n_matched, n_anc_entries): the rows of the region
    decoded straight into one packed2 block per population, left in HBM.  The index, the batches, the staging and
    the side stream are those of ``load_dosage_device``; behind each copy one ``sai_bed_pack2`` call per population
    writes the batch's sites of that population's block.  No int8 [record][slot] tensor exists on this route.
    ``trace`` as in ``load_dosage_device``."""
    import time

    import torch

    _ffi_plink.load()
    _ffi_packed_ingest.load()
    lib = eng.lib
    t0 = time.perf_counter()
    plan = _packed_plan(lib, path, chr_name, populations, start, end, anc_allele_file, n_threads)
    idx = plan.idx
    if trace is not None:
        trace["index"] = trace.get("index", 0.0) + time.perf_counter() - t0
        trace["bed_bytes"] = 0
    packed = plan.device_blocks(eng)
    if idx.n_slots == 0 or idx.n_rows == 0:
        return idx.pos, packed, idx.n_matched, idx.n_anc
    cap = _cap(buffer_bytes)
    # per population: status and unfit of every row, side by side in one tensor
    flags = torch.empty((len(plan.pops), 2, idx.n_rows), dtype=torch.int32, device=eng.device)
    cols_dev = [None if pop["first_col"] >= 0 else torch.from_numpy(pop["cols"]).to(eng.device) for pop in plan.pops]

    def launch(rows_ptr, batch, side):
        k0, k1, rib, n_batch_rows, _ = batch
        if k1 == k0:
            return None
        d_rib = torch.from_numpy(rib).to(eng.device, non_blocking=True)
        d_flip = torch.from_numpy(idx.flip[k0:k1]).to(eng.device, non_blocking=True)
        for p, pop in enumerate(plan.pops):
            if pop["n_ind"]:
                _ffi.check(
                    lib.sai_bed_pack2(eng.ctx, C.c_void_p(rows_ptr), n_batch_rows, idx.row_bytes, k1 - k0, eng._ptr(d_rib), eng._ptr(d_flip),
                                      idx.n_fam, pop["n_ind"], eng._ptr(cols_dev[p]), pop["first_col"], pop["ploidy"],
                                      C.c_void_p(packed[p].data.data_ptr()), idx.n_rows, k0, C.c_void_p(flags[p, 0].data_ptr() + 4 * k0),
                                      C.c_void_p(flags[p, 1].data_ptr() + 4 * k0), C.c_void_p(side.cuda_stream))
                )  # fmt: skip
        return d_rib, d_flip

    side = staged_copy(eng, "_plink_state", cap, idx.prefix + ".bed", idx.staged(cap), launch, trace, "bed_bytes")
    plan.raise_flagged_device(flags)
    torch.cuda.current_stream(eng.device).wait_stream(side)
    return idx.pos, packed, idx.n_matched, idx.n_anc
