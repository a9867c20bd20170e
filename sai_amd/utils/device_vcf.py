"""VCF region -> dosages resident in HBM, tokenised on the GPU.

The host side (libsaihip's ``sai_vcf_stream_*``) reads / inflates the file and indexes its record
lines while the genotype text crosses PCIe as it is; ``sai_tokenize_gt`` turns the text into int8
dosages on the GPU.  The producer thread fills one pinned buffer while the other one is being copied
and tokenised, so reading, PCIe and the kernel overlap.  Same rules and same bytes as the host
tokenizer (``native_vcf.load_dosage``); a line the GPU flags is handed to the host reader, which
produces the reference's error text.
"""

from __future__ import annotations

import ctypes as C
import os
import time
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _ffi
from ._ingest import Records, check_io, pair, region_args, staging

BUFFER_BYTES = 32 << 20
INFLATE_BATCH_BYTES = 3968 << 16  # 248 MiB: at most 3 968 full members, under the 4 096 the chip holds at a time
_MEMBER_BYTES = 32  # sizeof(sai_bgzf_member)


def _inflate_batch_for(vcf_file) -> int:
    """Text bytes per GPU-inflate batch: the full 248 MiB for files that can fill it, a quarter-step
    size class for small ones (the staging buffers are pinned and kept per size: a 100 kB file should
    not page-lock 400 MB).  Only a ceiling: a file that inflates to more simply takes more batches."""
    try:
        guess = os.path.getsize(vcf_file) * 16  # genotype text compresses 10-20x
    except OSError:
        return INFLATE_BATCH_BYTES
    cap = 1 << 20
    while cap < guess and cap < INFLATE_BATCH_BYTES:
        cap <<= 2
    return min(cap, INFLATE_BATCH_BYTES)


class _Fallback(Exception):
    """The bgzip-on-the-GPU route cannot serve this read; the host-inflating stream takes it."""


class _TextIndex(Exception):
    """The line heads would be most of the text (short lines) or do not reach the ninth tab: index
    this file from the whole text instead."""


def load_dosage_device(eng, vcf_file: str, chr_name: str, samples: Sequence[str], ploidies: Sequence[int],
                       start: Optional[int] = None, end: Optional[int] = None, anc_allele_file: Optional[str] = None,
                       n_threads: Optional[int] = None, buffer_bytes: Optional[int] = None):  # fmt: skip
    """(pos int32 host array [n], dosage int8 DEVICE tensor [n][len(samples)], n_matched,
    n_anc_entries) for one region -- ``load_dosage`` with the result left in HBM."""
    lib = eng.lib
    cap = int(buffer_bytes or os.environ.get("SAI_AMD_INGEST_BUFFER", BUFFER_BYTES))
    if os.environ.get("SAI_AMD_GPU_INFLATE", "1") != "0":
        try:
            # 4 096 members are in flight on the chip at a time: a batch of 248 MiB of text fills it in one round
            icap = int(buffer_bytes or os.environ.get("SAI_AMD_INFLATE_BATCH", 0)) or _inflate_batch_for(vcf_file)
            try:
                got = _load_bgzf_device(eng, vcf_file, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, icap)
            except _TextIndex:
                got = _load_bgzf_device(eng, vcf_file, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, icap,
                                        index_from="text")  # fmt: skip
            if got is not None:
                return got
        except _Fallback:
            pass
    # pinned staging + device text buffers, kept for the next call
    st = staging(eng, "_ingest_state", cap, lambda: {"pinned": pair(cap), "text": pair(cap + 16, device=eng.device),
                                                     "stream": torch.cuda.Stream(device=eng.device)})  # fmt: skip
    pinned, text, side = st["pinned"], st["text"], st["stream"]
    args = region_args(vcf_file, chr_name, start, end, samples, ploidies, anc_allele_file, n_threads)
    handle = C.c_void_p()
    check_io(lib, lib.sai_vcf_stream_open(*args, C.c_void_p(pinned[0].data_ptr()), C.c_void_p(pinned[1].data_ptr()), cap, C.byref(handle)))
    try:
        rec = Records(eng, lib.sai_vcf_stream_selection, handle, samples, ploidies)
        buf, n_text, copied = C.c_int32(), C.c_int64(), None
        while True:
            if copied is not None:
                copied.synchronize()  # the H2D copy of the previous batch has left its pinned buffer
            check_io(lib, lib.sai_vcf_stream_next(handle, C.byref(buf), C.byref(n_text), *rec.refs))
            if rec.done.value:
                break
            nb, b = int(n_text.value), int(buf.value)
            rec.select()
            with torch.cuda.stream(side):
                text[b][:nb].copy_(pinned[b][:nb], non_blocking=True)
                copied = torch.cuda.Event()
                copied.record(side)
                if rec.n_lines.value:
                    rec.launch(text[b].data_ptr(), 0, nb, side)
        counts = rec.counts()
    finally:
        lib.sai_vcf_stream_close(handle)
        side.synchronize()  # also on an error: the staging buffers are reused by the next call
    pos, dos = rec.finish([side], vcf_file, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads)
    return pos, dos, *counts


class _BgzfRead:
    """One read on the GPU-inflate route: the reader's handle, the staging ring of two slots, and what the steps
    of neighbouring batches hand each other.  A batch is a namespace: ``b`` (its ring slot), ``n_comp``,
    ``n_members``, ``n_text``, ``table``, ``carry`` (bytes in front of its own text that belong to it: the
    incomplete last line of the batch before; negative for the first batch of a region: that many bytes of its
    text are not its own), the events ``h2d`` / ``inflated`` / ``scanned`` / ``back``, and ``at`` / ``left``
    (where its own incomplete last line lies in ``text_dev[b]``, and its length)."""

    def __init__(self, eng, vcf_file, cap, index_from, positions_only):
        self.eng, self.lib, self.vcf_file, self.cap = eng, eng.lib, vcf_file, cap
        self.index_from, self.heads, self.positions_only = index_from, index_from != "text", positions_only
        # the incomplete last line of a batch is carried in front of the next one
        room = self.room = max(1 << 20, min(cap // 4, 8 << 20))
        comp_cap = self.comp_cap = cap // 4 + (1 << 20)
        line_cap = self.line_cap = (room + cap) // 48 + 16
        self.heads_cap = (room + cap) // 4
        st = self.st = staging(eng, "_inflate_state", cap, lambda: {
            "comp_host": pair(comp_cap), "comp_dev": pair(comp_cap, device=eng.device),
            "text_dev": pair(room + cap + 32, device=eng.device),
            "flag_host": [torch.zeros((4,), dtype=torch.int32).pin_memory() for _ in range(2)],
            **{name: torch.cuda.Stream(device=eng.device) for name in ("side", "copy", "d2h", "tok")}})  # fmt: skip
        if not self.heads and "text_host" not in st:
            st["text_host"] = pair(room + cap + 32)
        if self.heads and "starts_dev" not in st:
            st["starts_dev"] = pair(line_cap + 1, torch.int64, eng.device)
            st["info_dev"] = pair(line_cap, torch.int32, eng.device)
            st["heads_dev"] = pair(self.heads_cap, device=eng.device)
            st["scratch_dev"] = torch.empty(((room + cap + 32) // 4096 + 4,), dtype=torch.int32, device=eng.device)
            st["info4_dev"] = [torch.zeros((4,), dtype=torch.int32, device=eng.device) for _ in range(2)]
            # the pinned mirrors grow with the line counts actually seen (a 2 002-sample file has 31 000 lines
            # in a 248 MiB batch: 2 MB of table; page-locking for the worst case would cost 270 MB and 0.2 s)
            st["starts_host"], st["info_host"], st["heads_host"] = pair(1, torch.int64), pair(1, torch.int32), pair(1)
            st["tail_host"] = torch.empty((1,), dtype=torch.uint8).pin_memory()
        self.comp_host, self.comp_dev, self.text_dev, self.flag_host = st["comp_host"], st["comp_dev"], st["text_dev"], st["flag_host"]
        self.side, self.copy, self.d2h, self.tok = st["side"], st["copy"], st["d2h"], st["tok"]
        self.tok_done = [None, None]  # per ring slot: the tokenizer that read text_dev[slot] last
        self.last_inflate = [None, None]  # per ring slot: the event behind the inflate that read comp_dev[slot] last
        self.ahead, self.reader_done = None, False  # the batch fetched ahead, whether the reader has said "done"
        self.usable = C.c_int64()
        self.trace = {} if os.environ.get("SAI_AMD_INGEST_TRACE") else None

    def open(self, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads) -> bool:
        """Start the reader; False when the file is not bgzip."""
        lib, handle = self.lib, C.c_void_p()
        args = region_args(self.vcf_file, chr_name, start, end, samples, ploidies, anc_allele_file, n_threads)
        rc = lib.sai_bgzf_stream_open(*args, C.c_void_p(self.comp_host[0].data_ptr()), C.c_void_p(self.comp_host[1].data_ptr()),
                                      self.comp_cap, self.cap, C.byref(handle))  # fmt: skip
        if rc == _ffi.SAI_ERR_UNSUPPORTED:
            return False
        check_io(lib, rc)
        self.handle = handle
        try:
            self.rec = Records(self.eng, lib.sai_bgzf_stream_selection, handle, samples, ploidies)
            f_begin, f_stop, f_skip = C.c_int64(), C.c_int64(), C.c_int64()
            check_io(lib, lib.sai_bgzf_stream_region(handle, C.byref(f_begin), C.byref(f_stop), C.byref(f_skip)))
        except BaseException:
            lib.sai_bgzf_stream_close(handle)
            raise
        # text of the first member that belongs to records before the region (a tabix seek lands inside a member)
        self.skip = int(f_skip.value)
        # what the last read took from the file (tests and tools/bgzf_rate.py look at it)
        self.last = self.st["last"] = {"file_begin": int(f_begin.value), "file_stop": int(f_stop.value), "first_text_skip": self.skip,
                                       "members": 0, "comp_bytes": 0, "text_bytes": 0}  # fmt: skip
        self.t_mark = time.perf_counter()
        return True

    def lap(self, name):
        if self.trace is not None:
            now = time.perf_counter()
            self.trace[name] = self.trace.get(name, 0.0) + now - self.t_mark
            self.t_mark = now

    def span(self, batch):
        """(ring slot, where the batch's text starts in text_dev[slot] with what is carried in front, its length)"""
        return batch.b, self.room - batch.carry, batch.carry + batch.n_text

    def fetch(self):
        """The next batch of members from the reader; its compressed bytes start for HBM (copy stream)."""
        buf, n_comp, n_mem, n_text, done = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64(), C.c_int32()
        table_p = C.c_void_p()
        check_io(self.lib, self.lib.sai_bgzf_stream_next(self.handle, C.byref(buf), C.byref(n_comp), C.byref(n_mem), C.byref(table_p),
                                                         C.byref(n_text), C.byref(done)))  # fmt: skip
        self.lap("wait_reader")
        if done.value:
            return None
        b, nc, nm, nt = int(buf.value), int(n_comp.value), int(n_mem.value), int(n_text.value)
        self.last["members"] += nm
        self.last["comp_bytes"] += nc
        self.last["text_bytes"] += nt
        table = np.ctypeslib.as_array(C.cast(table_p, C.POINTER(C.c_uint8)), shape=(nm * _MEMBER_BYTES,)).copy()
        with torch.cuda.stream(self.copy):
            if self.last_inflate[b] is not None:
                self.copy.wait_event(self.last_inflate[b])  # the inflate two batches back may still be reading comp_dev[b]
            self.comp_dev[b][:nc].copy_(self.comp_host[b][:nc], non_blocking=True)
            h2d = torch.cuda.Event()
            h2d.record(self.copy)
        self.lap("copy_table")
        carry, self.skip = -self.skip, 0
        if -carry > nt:
            raise ValueError(f"{self.vcf_file}: the tabix index points behind the end of a BGZF block")
        return SimpleNamespace(b=b, n_comp=nc, n_members=nm, n_text=nt, table=table, h2d=h2d, carry=carry)

    def launch(self, batch):
        """Inflate + CRC of a fetched batch.  Its H2D copy was started one batch earlier -- a copy issued
        while the inflate kernel holds the chip waits for it (measured: 2 ms instead of 0.2) -- so the
        wait here is short, and the reader gets its pinned buffer back."""
        eng, side, b, nm = self.eng, self.side, batch.b, batch.n_members
        batch.h2d.synchronize()
        self.lib.sai_bgzf_stream_release(self.handle)
        self.lap("h2d_sync")
        with torch.cuda.stream(side):
            if self.tok_done[b] is not None:
                side.wait_event(self.tok_done[b])  # the tokenizer two batches back read text_dev[b]
            d_tab = torch.from_numpy(batch.table).to(eng.device, non_blocking=True)
            d_stat = torch.empty((nm,), dtype=torch.int32, device=eng.device)
            _ffi.check(
                self.lib.sai_inflate_bgzf(eng.ctx, C.c_void_p(self.comp_dev[b].data_ptr()), batch.n_comp, C.c_void_p(d_tab.data_ptr()), nm,
                                          C.c_void_p(self.text_dev[b].data_ptr() + self.room), batch.n_text, C.c_void_p(d_stat.data_ptr()),
                                          C.c_void_p(side.cuda_stream))
            )  # fmt: skip
            batch.bad = (d_stat != 0).sum(dtype=torch.int32).reshape(1)
            batch.inflated = self.last_inflate[b] = torch.cuda.Event()
            batch.inflated.record(side)
            batch.keep = (d_tab, d_stat)
        self.lap("enqueue_inflate")

    def fetch_ahead(self):
        if not self.reader_done and self.ahead is None:
            self.ahead = self.fetch()
            self.reader_done = self.ahead is None

    def next_batch(self):
        """The next batch with its inflate enqueued (None at the end); the H2D copy of the one after it runs
        under that inflate."""
        self.fetch_ahead()
        batch, self.ahead = self.ahead, None
        if batch is not None:
            self.launch(batch)
            self.fetch_ahead()
        return batch

    def move_carry(self, prev, batch):
        """The incomplete last line of ``prev`` goes in front of ``batch`` on the device (and, when the host indexes
        from the whole text, in its copy there)."""
        at, left, room = prev.at, prev.left, self.room
        if left and batch is not None and not self.heads:
            text_host = self.st["text_host"]
            text_host[batch.b][room - left : room].copy_(text_host[prev.b][at : at + left])
        if left > room:
            raise _Fallback  # a record line longer than the carry room
        if left and batch is not None:
            with torch.cuda.stream(self.side):
                self.text_dev[batch.b][room - left : room].copy_(self.text_dev[prev.b][at : at + left], non_blocking=True)
            batch.carry = left

    def tokenize(self, b, base, n_bytes, ready=None):
        """The record lines the index call just reported (offsets relative to text_dev[b][base]).  With
        ``ready`` (the event behind the batch's text) the kernel runs on its own stream, beside the
        inflate of the next batch -- that one occupies a fifth of the wavefront slots."""
        rec = self.rec
        if rec.n_lines.value == 0:
            return
        if self.positions_only:
            rec.take_positions()
            return
        rec.select()
        if ready is None:
            rec.launch(self.text_dev[b].data_ptr(), base, n_bytes, self.side)
        else:
            self.tok.wait_event(ready)
            rec.launch(self.text_dev[b].data_ptr(), base, n_bytes, self.tok)
            self.tok_done[b] = torch.cuda.Event()
            self.tok_done[b].record(self.tok)

    def index_text(self, host_ptr, b, base, n_bytes, n_carry, is_last):
        """Index ``n_bytes`` of text on the host (they lie at text_dev[b][base] on the device) and tokenise them."""
        check_io(self.lib, self.lib.sai_vcf_index_text(self.handle, C.c_void_p(host_ptr), n_bytes, n_carry, None, 0, 1 if is_last else 0,
                                                       C.byref(self.usable), *self.rec.refs))  # fmt: skip
        self.tokenize(b, base, n_bytes)

    def index_tail(self, prev):
        """The file ends without a newline: the last line of ``prev`` is indexed as text (a few bytes: the heads
        mode brings them to the host for it)."""
        at, left = prev.at, prev.left
        if self.heads:
            if self.st["tail_host"].numel() < left:
                self.st["tail_host"] = torch.empty((1 << (left - 1).bit_length(),), dtype=torch.uint8).pin_memory()
            tail_host = self.st["tail_host"]
            with torch.cuda.stream(self.side):
                tail_host[:left].copy_(self.text_dev[prev.b][at : at + left], non_blocking=True)
            self.side.synchronize()
            host_ptr = tail_host.data_ptr()
        else:
            host_ptr = self.st["text_host"][prev.b].data_ptr() + at
        self.index_text(host_ptr, prev.b, at, left, left, True)

    # -- index_from="text": the whole text comes back once (d2h stream) and sai_vcf_index_text reads it

    def copy_back(self, batch):
        b, nt, room, d2h = batch.b, batch.n_text, self.room, self.d2h
        with torch.cuda.stream(d2h):
            d2h.wait_event(batch.inflated)
            self.st["text_host"][b][room : room + nt].copy_(self.text_dev[b][room : room + nt], non_blocking=True)
            self.flag_host[b][:1].copy_(batch.bad, non_blocking=True)
            batch.back = torch.cuda.Event()
            batch.back.record(d2h)

    def index_copied_text(self, prev):
        b, base, total = self.span(prev)
        prev.back.synchronize()
        self.lap("wait_d2h")
        if int(self.flag_host[b][0]):
            raise ValueError(f"{self.vcf_file}: BGZF block fails to inflate or its CRC")
        self.index_text(self.st["text_host"][b].data_ptr() + base, b, base, total, max(prev.carry, 0), False)
        self.lap("index_and_tokenize")
        used = int(self.usable.value)
        prev.at, prev.left = base + used, total - used

    # -- index_from="heads": the GPU finds the lines; the host indexes from their heads

    def scan_lines(self, batch):
        st, side, (b, base, total) = self.st, self.side, self.span(batch)
        with torch.cuda.stream(side):
            _ffi.check(
                self.lib.sai_text_line_starts(self.eng.ctx, C.c_void_p(self.text_dev[b].data_ptr() + base), total, self.line_cap,
                                              C.c_void_p(st["starts_dev"][b].data_ptr()), C.c_void_p(st["info_dev"][b].data_ptr()),
                                              C.c_void_p(st["scratch_dev"].data_ptr()), C.c_void_p(st["info4_dev"][b].data_ptr()),
                                              C.c_void_p(side.cuda_stream))
            )  # fmt: skip
            self.flag_host[b][:3].copy_(st["info4_dev"][b][:3], non_blocking=True)
            self.flag_host[b][3:].copy_(batch.bad, non_blocking=True)
            batch.scanned = torch.cuda.Event()
            batch.scanned.record(side)

    def fetch_table(self, batch):
        """Wait for the scan, gather the heads and bring them to the host with the line table; its last offset says
        where the batch's incomplete last line lies."""
        st, d2h, (b, base, total) = self.st, self.d2h, self.span(batch)
        batch.scanned.synchronize()
        self.lap("wait_scan")
        n_l, fixed, overflow, bad = (int(v) for v in self.flag_host[b].tolist())
        if bad:
            raise ValueError(f"{self.vcf_file}: BGZF block fails to inflate or its CRC")
        hb = max(16, (fixed + 3) & ~3)
        if overflow or fixed > 4096 or n_l * hb > self.heads_cap:
            raise _TextIndex  # short lines / far fixed columns: the whole-text index serves this file
        batch.n_lines, batch.hb = n_l, hb
        moves = [(st["starts_host"], st["starts_dev"], n_l + 1), (st["info_host"], st["info_dev"], max(n_l, 1)),
                 (st["heads_host"], st["heads_dev"], max(n_l * hb, 1))]  # fmt: skip
        for host, dev, need in moves:
            if host[b].numel() < need:
                host[b] = torch.empty((1 << (need - 1).bit_length(),), dtype=dev[b].dtype).pin_memory()
        with torch.cuda.stream(d2h):  # its own stream: the next batch's inflate is already queued on `side`
            _ffi.check(
                self.lib.sai_text_line_heads(self.eng.ctx, C.c_void_p(self.text_dev[b].data_ptr() + base), total,
                                             C.c_void_p(st["starts_dev"][b].data_ptr()), n_l, hb, C.c_void_p(st["heads_dev"][b].data_ptr()),
                                             C.c_void_p(d2h.cuda_stream))
            )  # fmt: skip
            for host, dev, need in moves:
                host[b][:need].copy_(dev[b][:need], non_blocking=True)
            tabled = torch.cuda.Event()
            tabled.record(d2h)
        tabled.synchronize()
        used = int(st["starts_host"][b][n_l]) if n_l else 0
        batch.at, batch.left = base + used, total - used

    def index_heads(self, prev):
        st, (b, base, total) = self.st, self.span(prev)
        self.lap("wait_table")
        heads, starts, info = (C.c_void_p(st[name][b].data_ptr()) for name in ("heads_host", "starts_host", "info_host"))
        check_io(self.lib, self.lib.sai_vcf_index_heads(self.handle, heads, prev.hb, starts, info, prev.n_lines, *self.rec.refs))
        self.tokenize(b, base, total, ready=prev.scanned)
        self.lap("index_and_tokenize")

    def stage(self, prev, batch):
        """What is enqueued for `batch` (and, heads mode, fetched of `prev`) before the host indexes `prev`."""
        if not self.heads:
            if batch is not None:
                self.copy_back(batch)
            return
        if prev is not None:
            self.fetch_table(prev)
            self.move_carry(prev, batch)
        if batch is not None:
            self.scan_lines(batch)  # runs behind the inflate of `batch`, while the host indexes `prev`

    def index(self, prev, batch):
        """Index and tokenise `prev`; False when nothing follows it (the region is passed, or the file ends)."""
        if self.heads:
            self.index_heads(prev)
        else:
            self.index_copied_text(prev)
        if self.rec.done.value:
            return False
        if batch is None:
            if prev.left:
                self.index_tail(prev)
            return False
        if not self.heads:  # known only now: the heads mode read it off the line table in `stage`
            self.move_carry(prev, batch)
        return True

    def run(self):
        """Batch after batch: `batch` is inflated (and, heads mode, scanned) while the host indexes `prev`."""
        prev, batch = None, self.next_batch()
        self.stage(None, batch)
        while batch is not None:
            prev, batch = batch, self.next_batch()
            self.stage(prev, batch)
            if not self.index(prev, batch):
                break

    def close(self):
        self.lap("other")
        self.lib.sai_bgzf_stream_close(self.handle)
        for stream in (self.side, self.copy, self.d2h, self.tok):
            stream.synchronize()  # also on an error: the staging buffers are reused by the next call
        self.lap("close_and_drain")


def _load_bgzf_device(eng, vcf_file, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, cap, index_from=None,
                      positions_only=False):  # fmt: skip
    """``load_dosage_device`` for a bgzip file.  A region of a file with a usable ``.tbi`` is a seek: the
    reader hands over only the members that hold the region (``sai_bgzf_stream_region``), and the line
    table of the first batch starts behind the text that precedes the region's first record.  The compressed members cross
    PCIe and are inflated by ``sai_inflate_bgzf`` (one wavefront per member; a second launch checks
    every member's CRC-32).  The record index -- chromosome / region filter, POS, the ancestral-allele
    decision, where the sample columns start: the host's ``index_lines`` rules -- is made from the
    line table the GPU extracts (``sai_text_line_starts`` / ``_heads``: line offsets + the fixed
    columns of every line, a few MB) or, ``index_from="text"``, from the whole text copied back once;
    the text is tokenised where it lies in HBM either way.  Batch k+1 is inflated and scanned while
    the host indexes batch k.  Returns None when the file is not bgzip: the caller falls back to the
    host-inflating stream.  ``positions_only`` (no samples):
    the record index alone, nothing is tokenised."""
    read = _BgzfRead(eng, vcf_file, cap, index_from or os.environ.get("SAI_AMD_BGZF_INDEX", "heads"), positions_only)
    if not read.open(chr_name, samples, ploidies, start, end, anc_allele_file, n_threads):
        return None
    try:
        read.run()
        counts = read.rec.counts()
    finally:
        read.close()
    pos, dos = read.rec.finish([read.side, read.tok], vcf_file, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads)
    read.lap("status_and_concat")
    if read.trace is not None:
        print(f"bgzf route ({read.index_from}), ms:", " ".join(f"{k}={1e3 * v:.1f}" for k, v in read.trace.items()), flush=True)
    return pos, dos, *counts


def scan_first_last_device(eng, vcf_file: str, chr_name: str):
    """First and last POS of the first contiguous run of ``chr_name`` in a bgzip file, found with the
    GPU-inflate pass (no sample column is tokenised): what ``ChunkGenerator`` needs before the windows
    can be laid out.  None when this route does not serve the file (not bgzip, lines it cannot index
    from their heads and would have to copy back whole, ...): the host scan does it then."""
    if os.environ.get("SAI_AMD_GPU_INFLATE", "1") == "0":
        return None
    cap = int(os.environ.get("SAI_AMD_INFLATE_BATCH", 0)) or _inflate_batch_for(vcf_file)
    try:
        got = _load_bgzf_device(eng, vcf_file, chr_name, [], [], None, None, None, None, cap, positions_only=True)
    except (_Fallback, _TextIndex):
        return None
    if got is None:
        return None
    pos = got[0]
    return (None, None) if pos.size == 0 else (int(pos[0]), int(pos[-1]))
