"""The steps the ingest readers share (``native_vcf``, ``device_vcf``, ``plink``, ``eigenstrat``, ``pgen``): the region /
sample arguments of the C ABI, its errors as ValueError, the staging kept on the engine, the batches and the
``pread`` of fixed-length rows (the PLINK 1 and EIGENSOFT readers) and of variable-length records (the PLINK 2
reader), the loop of the fileset readers over those batches -- ``read_batches`` on the host, ``staged_copy`` through
two pinned buffers and a side stream to the device -- and, ``Records``, what the two GPU-tokenising VCF routes do with
the record lines of a batch."""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .. import _ffi

# torch is imported where it is used: native_vcf imports this module, and the host-only library of the sanitizer
# build is loaded without torch.  device_vcf, which only ever runs with a GPU, imports it at the top.


def default_threads() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def check_io(lib, status: int) -> None:
    """I/O and format problems of the ingest surface as ValueError, like the reference's readers."""
    if status != 0:
        raise ValueError(lib.sai_last_error().decode("utf-8", "replace"))


def region_args(path, chr_name, start, end, samples, ploidies, anc_allele_file, n_threads) -> tuple:
    """``(path, chrom, start, end, n, names, ploidies, anc file, threads)`` as the ``*_open`` / ``sai_vcf_load``
    calls take them; the caller holds the tuple for as long as the call runs."""
    n = len(samples)
    return (os.fsencode(path), str(chr_name).encode(), -1 if start is None else int(start), -1 if end is None else int(end), n,
            (C.c_char_p * n)(*[s.encode() for s in samples]), (C.c_int32 * n)(*[int(p) for p in ploidies]),
            os.fsencode(anc_allele_file) if anc_allele_file else None, n_threads or default_threads())  # fmt: skip


def staging(eng, key: str, cap: int, make) -> dict:
    """The buffers and streams a reader keeps on the engine under ``key`` for its next call: a plain dict
    (``Engine.release_ingest_buffers`` pops and synchronises it), filled from ``make()`` whenever ``cap`` changes."""
    st = eng.__dict__.setdefault(key, {})
    if st.get("cap") != cap:
        st.clear()
        st["cap"] = cap
        st.update(make())
    return st


def pair(n: int, dtype=None, device=None) -> list:
    """Two buffers of ``n`` elements (bytes unless ``dtype`` says otherwise): on ``device``, else page-locked on the host."""
    import torch

    bufs = [torch.empty((n,), dtype=dtype or torch.uint8, device=device) for _ in range(2)]
    return bufs if device is not None else [t.pin_memory() for t in bufs]


def row_batches(file_row, row_bytes: int, data_offset: int, cap: int, read_through: int, data_path: str, index_path: str):
    """Cut the selected rows ``file_row`` (ascending 0-based rows of ``row_bytes`` bytes that start at
    ``data_offset`` of the file) into batches of at most ``cap`` bytes of whole rows.  Selected rows that are close
    in the file are read as one range, the rows between them included when they come to at most ``read_through``
    bytes (a ``pread`` per row would cost more than their bytes); the ranges of a batch lie back to back in its
    buffer.  Yields ``(k0, k1, row_in_batch int32 [k1 - k0], n_batch_rows, reads)`` with ``reads`` = [(buffer
    offset, file offset, bytes)]."""
    rb, n_rows = row_bytes, len(file_row)
    if n_rows == 0 or rb == 0:
        return
    per_batch = cap // rb
    if per_batch < 1:
        raise ValueError(f"SAI_AMD_INGEST_BUFFER of {cap} bytes is smaller than one row of {data_path} ({rb} bytes)")
    rows = file_row
    new_range = np.empty(n_rows, dtype=bool)
    new_range[0] = True
    new_range[1:] = np.diff(rows) > 1 + read_through // rb
    if n_rows > 1 and bool((np.diff(rows) <= 0).any()):
        raise ValueError(f"{index_path}: the index is not in file order")
    starts = np.flatnonzero(new_range)
    range_first = rows[starts]  # first file row of every range
    range_last = rows[np.append(starts[1:] - 1, n_rows - 1)]
    range_base = np.concatenate(([0], np.cumsum(range_last - range_first + 1)))  # ... its place in the stream of all ranges
    range_of = np.cumsum(new_range) - 1
    stream_row = rows - range_first[range_of] + range_base[range_of]  # ascending
    total = int(range_base[-1])
    for lo in range(0, total, per_batch):
        hi = min(lo + per_batch, total)
        k0, k1 = (int(x) for x in np.searchsorted(stream_row, (lo, hi)))
        reads = []
        j = int(np.searchsorted(range_base, lo, side="right")) - 1
        at = lo
        while at < hi:
            stop = min(hi, int(range_base[j + 1]))
            reads.append(((at - lo) * rb, data_offset + (int(range_first[j]) + at - int(range_base[j])) * rb, (stop - at) * rb))
            at = stop
            j += 1
        yield k0, k1, (stream_row[k0:k1] - lo).astype(np.int32), hi - lo, reads


def span_batches(rec, base, cap: int, read_through: int, data_path: str):
    """``row_batches`` for records of variable length.  ``rec`` = int64 [n][3], the (file offset, length, type) of
    every selected row's record in file order; ``base`` = the same of the record it differs from, or -1.  The wanted
    records -- rows and bases -- are laid out as one stream in file order, records between two wanted ones read along
    when they come to at most ``read_through`` bytes; a batch is a piece of that stream that ends behind a row, at
    most ``cap`` bytes.  A base that lies before the piece can only be the base of the batch's first row (every
    record between a base and its row differs from the same base): it is read to the front of the buffer, even when
    its own row went out with the previous batch.  Yields ``(k0, k1, rec [k1 - k0][3], base [k1 - k0][3], n_bytes,
    reads)``, the offsets of the two tables counted from the start of the buffer, ``reads`` = [(buffer offset, file
    offset, bytes)]."""
    n_rows = len(rec)
    if n_rows == 0:
        return
    rec_off, rec_len = rec[:, 0], rec[:, 1]
    if n_rows > 1 and bool((np.diff(rec_off) <= 0).any()):
        raise ValueError(f"{data_path}: the index is not in file order")
    has_base = base[:, 0] >= 0
    if bool((base[has_base, 0] >= rec_off[has_base]).any()):
        raise ValueError(f"{data_path}: a record's base does not lie before it")
    offs, where = np.unique(np.concatenate((rec_off, base[has_base, 0])), return_index=True)
    lens = np.concatenate((rec_len, base[has_base, 1]))[where]
    gap = offs[1:] - (offs[:-1] + lens[:-1])
    if bool((gap < 0).any()):
        raise ValueError(f"{data_path}: records overlap")
    new_range = np.ones(len(offs), dtype=bool)
    new_range[1:] = gap > read_through
    skipped = np.concatenate(([0], np.cumsum(np.where(new_range[1:], gap, 0))))
    at_stream = offs - offs[0] - skipped  # where every wanted record starts in the stream
    starts = np.flatnonzero(new_range)
    range_stream, range_file = at_stream[starts], offs[starts]
    range_end = np.append(range_stream[1:], at_stream[-1] + lens[-1])
    rec_at = at_stream[np.searchsorted(offs, rec_off)]
    rec_end = rec_at + rec_len
    base_at = np.where(has_base, at_stream[np.searchsorted(offs, np.where(has_base, base[:, 0], offs[0]))], -1)
    def too_small(k: int) -> ValueError:
        front = int(base[k, 1]) if has_base[k] else 0
        return ValueError(f"SAI_AMD_INGEST_BUFFER of {cap} bytes is smaller than one record of {data_path} "
                          f"({int(rec_len[k])} bytes{f' and its base of {front}' if front else ''})")  # fmt: skip

    # A row and its base never fit a smaller buffer, whichever batch the row falls into: with the base inside the
    # batch both are staged, with the base before it the base is read to the front.  So the first row that is too
    # long is refused here, before the first batch is yielded, and not after the rows before it have been decoded.
    short = np.flatnonzero(rec_len + np.where(has_base, base[:, 1], 0) > cap)
    if short.size:
        raise too_small(int(short[0]))
    k0 = 0
    while k0 < n_rows:
        lo = int(rec_at[k0])
        front = int(base[k0, 1]) if has_base[k0] else 0  # the first row's base, read on its own
        k1 = int(np.searchsorted(rec_end, lo + cap - front, side="right"))
        if k1 <= k0:  # cannot be, after the check above: but a batch without a row would never end the loop
            raise too_small(k0)
        hi = int(rec_end[k1 - 1])
        reads = [(0, int(base[k0, 0]), front)] if front else []
        j = int(np.searchsorted(range_stream, lo, side="right")) - 1
        at = lo
        while at < hi:
            stop = min(hi, int(range_end[j]))
            reads.append((front + at - lo, int(range_file[j]) + at - int(range_stream[j]), stop - at))
            at = stop
            j += 1
        rows, bases = rec[k0:k1].copy(), base[k0:k1].copy()
        rows[:, 0] = rec_at[k0:k1] - lo + front
        inside = base_at[k0:k1] >= lo
        before = has_base[k0:k1] & ~inside
        if bool((base[k0:k1, 0][before] != base[k0, 0]).any()):
            raise ValueError(f"{data_path}: rows of one batch differ from several records before it")
        bases[:, 0] = np.where(has_base[k0:k1], np.where(inside, base_at[k0:k1] - lo + front, 0), -1)
        yield k0, k1, rows, bases, front + hi - lo, reads
        k0 = k1


_PREAD_PIECE = 4 << 20  # a batch is read by several threads in pieces of this size
_pool = None


def _read_pool():
    from concurrent.futures import ThreadPoolExecutor

    global _pool
    if _pool is None or getattr(_pool, "_owner", None) != os.getpid():  # threads do not survive a fork
        _pool = ThreadPoolExecutor(max(1, min(default_threads(), 8)), thread_name_prefix="sai-fileset-read")
        _pool._owner = os.getpid()
    return _pool


def pread_into(fd: int, view: memoryview, reads, path: str) -> None:
    """Fill ``view`` from the file: ``reads`` = [(buffer offset, file offset, bytes)], large ones in pieces on
    several threads (``preadv`` releases the GIL; one thread copies the page cache at a fraction of what PCIe takes)."""
    pieces = []
    for at, off, n in reads:
        for d in range(0, n, _PREAD_PIECE):
            pieces.append((at + d, off + d, min(_PREAD_PIECE, n - d)))

    def one(piece):
        at, off, n = piece
        done = 0
        while done < n:
            got = os.preadv(fd, [view[at + done : at + n]], off + done)
            if got <= 0:
                raise ValueError(f"{path}: read error or unexpected end of file at byte {off + done}")
            done += got

    if len(pieces) > 1:
        pool = _read_pool()
        workers = pool._max_workers
        if len(pieces) > 2 * workers:  # many small reads (one per individual of a transposed .geno): a share per thread, not a task each
            share = -(-len(pieces) // workers)
            list(pool.map(lambda lo: [one(piece) for piece in pieces[lo : lo + share]], range(0, len(pieces), share)))
        else:
            list(pool.map(one, pieces))
    else:
        for piece in pieces:
            one(piece)


def read_batches(path: str, batches, decode) -> None:
    """The host readers' loop: every batch ``(reads, nbytes, item)`` of ``batches`` is ``pread`` from ``path`` into
    one buffer that grows to the largest of them, and ``decode(buf, item)`` takes it from there."""
    buf = None
    fd = os.open(path, os.O_RDONLY)
    try:
        for reads, nbytes, item in batches:
            if buf is None or buf.size < nbytes:
                buf = np.empty(nbytes, dtype=np.uint8)
            pread_into(fd, memoryview(buf), reads, path)
            decode(buf, item)
    finally:
        os.close(fd)


def staged_copy(eng, key: str, size: int, path: str, batches, launch, trace=None, counter: str = ""):
    """The device readers' loop.  Every batch ``(reads, nbytes, item)`` of ``batches`` is ``pread`` from ``path`` into
    two pinned buffers of ``size`` bytes in turn and copied to their device twins on a side stream; behind the copy
    ``launch(device pointer of the batch's bytes, item, side stream)`` enqueues the batch's tables and kernels, inside
    the side-stream context, so the file read of batch k + 1 runs under the copy and the kernels of batch k.  The
    buffers and the stream are kept on the engine under ``key`` for the next call.  Returns the side stream, drained:
    the caller looks at its flags and lets the current stream wait for it.

    ``launch`` returns the device tensors that must outlive it (the batch's tables).  They are held per buffer and
    those of two batches back go: they are allocated and used on the side stream alone, so the caching allocator
    hands their memory to nothing that could run before the kernels that read them.

    ``trace`` (a dict) collects host-clock seconds per phase: always ``file_read``, and under ``counter`` the bytes
    read; with ``trace["serial"]`` set the side stream is synchronised behind every copy and every ``launch``, so
    ``h2d`` and ``decode`` are timed on their own (and nothing overlaps)."""
    import itertools
    import time

    import torch

    batches = iter(batches)
    head = list(itertools.islice(batches, 1))  # a buffer that is too small is refused here, before anything is page-locked
    st = staging(eng, key, size, lambda: {"pinned": pair(size), "rows": pair(size, device=eng.device),
                                          "stream": torch.cuda.Stream(device=eng.device)})  # fmt: skip
    pinned, dev_rows, side = st["pinned"], st["rows"], st["stream"]
    copied = [None, None]  # per buffer: the event behind its last H2D copy
    tables = [None, None]  # per buffer: what the ``launch`` of its last batch returned
    fd = os.open(path, os.O_RDONLY)
    try:
        side.wait_stream(torch.cuda.current_stream(eng.device))  # the caller's outputs were allocated on the current stream
        b = 0
        for reads, nbytes, item in itertools.chain(head, batches):
            if copied[b] is not None:
                copied[b].synchronize()  # the copy two batches back has left this pinned buffer
            t1 = time.perf_counter()
            pread_into(fd, memoryview(pinned[b].numpy()), reads, path)
            if trace is not None:
                trace["file_read"] = trace.get("file_read", 0.0) + time.perf_counter() - t1
                # the bytes read, not the bytes staged: the same for row_batches ((hi - lo) rows, in ranges back to back)
                # and span_batches (front + hi - lo), fewer where the reads lie apart in the buffer (a padded stride)
                trace[counter] += sum(r[2] for r in reads)
            serial = trace is not None and trace.get("serial")
            with torch.cuda.stream(side):
                t1 = time.perf_counter()
                dev_rows[b][:nbytes].copy_(pinned[b][:nbytes], non_blocking=True)
                copied[b] = torch.cuda.Event()
                copied[b].record(side)
                if serial:
                    side.synchronize()
                    trace["h2d"] = trace.get("h2d", 0.0) + time.perf_counter() - t1
                    t1 = time.perf_counter()
                tables[b] = launch(dev_rows[b].data_ptr(), item, side)
                if serial:
                    side.synchronize()
                    trace["decode"] = trace.get("decode", 0.0) + time.perf_counter() - t1
            b ^= 1
    finally:
        os.close(fd)
        side.synchronize()  # also on an error: the staging buffers are reused by the next call
    return side


class Records:
    """The record lines of one read: the out-parameters an index call fills with the line table of a batch
    (``refs``, in the order the C ABI takes them), and the positions, dosage blocks and tokenizer statuses
    collected batch by batch."""

    def __init__(self, eng, selection, handle, samples, ploidies):
        import torch

        self.eng, self.selection, self.handle, self.n = eng, selection, handle, len(samples)
        self.n_lines, self.done = C.c_int64(), C.c_int32()
        self.p_off, self.p_len, self.p_pos, self.p_flip, self.p_gi = (C.c_void_p() for _ in range(5))
        self.refs = tuple(C.byref(x) for x in (self.n_lines, self.p_off, self.p_len, self.p_pos, self.p_flip, self.p_gi, self.done))
        self.ploidy_dev = torch.tensor([int(p) for p in ploidies], dtype=torch.int32, device=eng.device)
        self.n_cols, self.slot_dev = 0, None
        self.outs, self.stats, self.pos_parts = [], [], []

    def select(self) -> None:
        """Fetch the column count and the column -> slot map of the stream handle, once the header is read."""
        import torch

        if self.slot_dev is not None:
            return
        lib, cols = self.eng.lib, C.c_int32()
        check_io(lib, self.selection(self.handle, None, 0, C.byref(cols), None, None))
        self.n_cols = int(cols.value)
        slots = np.empty(max(self.n_cols, 1), dtype=np.int32)
        check_io(lib, self.selection(self.handle, slots.ctypes.data_as(C.c_void_p), self.n_cols, C.byref(cols), None, None))
        self.slot_dev = torch.from_numpy(slots[: self.n_cols].copy()).to(self.eng.device)

    def _column(self, ptr, ctype, dtype):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(int(self.n_lines.value),)).astype(dtype, copy=True)

    def take_positions(self) -> None:
        self.pos_parts.append(self._column(self.p_pos, C.c_int32, np.int32))

    def launch(self, text_ptr: int, base: int, n_bytes: int, stream) -> None:
        """The batch step: the line table the index call just reported (offsets relative to ``text_ptr + base``)
        goes to the device and ``sai_tokenize_gt`` reads its lines, all on ``stream``."""
        import torch

        eng, nl = self.eng, int(self.n_lines.value)
        self.take_positions()
        with torch.cuda.stream(stream):
            d_off = torch.from_numpy(self._column(self.p_off, C.c_int64, np.int64) + base).to(eng.device, non_blocking=True)
            d_len = torch.from_numpy(self._column(self.p_len, C.c_int32, np.int32)).to(eng.device, non_blocking=True)
            d_flip = torch.from_numpy(self._column(self.p_flip, C.c_uint8, np.uint8)).to(eng.device, non_blocking=True)
            d_gi = torch.from_numpy(self._column(self.p_gi, C.c_uint8, np.uint8)).to(eng.device, non_blocking=True)
            out = torch.empty((nl, self.n), dtype=torch.int8, device=eng.device)
            status = torch.empty((nl,), dtype=torch.int32, device=eng.device)
            _ffi.check(
                eng.lib.sai_tokenize_gt(eng.ctx, C.c_void_p(text_ptr), (base + n_bytes + 3) & ~3, nl, eng._ptr(d_off), eng._ptr(d_len),
                                        eng._ptr(d_flip), eng._ptr(d_gi), self.n_cols, eng._ptr(self.slot_dev), self.n,
                                        eng._ptr(self.ploidy_dev), eng._ptr(out), eng._ptr(status), C.c_void_p(stream.cuda_stream))
            )  # fmt: skip
            self.outs.append(out)
            self.stats.append(status)

    def counts(self) -> tuple[int, int]:
        """(records matched, ancestral-allele entries) of the finished read; zeros when no header was seen."""
        n_match, n_anc, cols = C.c_int64(), C.c_int64(), C.c_int32()
        if self.selection(self.handle, None, 0, C.byref(cols), C.byref(n_match), C.byref(n_anc)):
            return 0, 0
        return int(n_match.value), int(n_anc.value)

    def finish(self, streams, vcf_file, *host_args):
        """(pos, dos) of the whole read once ``streams`` have been drained.  A line the tokenizer flagged is one
        the host reader refuses: it is asked to say why, in the reference's words."""
        import torch

        from .native_vcf import load_dosage

        if self.stats and bool(torch.cat(self.stats).any()):
            load_dosage(vcf_file, *host_args)
            raise ValueError(f"{vcf_file}: the GPU tokenizer flagged a line the host reader accepts")
        for stream in streams:
            torch.cuda.current_stream(self.eng.device).wait_stream(stream)
        pos = np.concatenate(self.pos_parts) if self.pos_parts else np.zeros(0, dtype=np.int32)
        if not self.outs:
            return pos, torch.empty((0, self.n), dtype=torch.int8, device=self.eng.device)
        return pos, torch.cat(self.outs) if len(self.outs) > 1 else self.outs[0]
