"""BCF 2.x files (BGZF-compressed, as ``bcftools view -Ob`` writes them) as an input of ``score``.

A BCF record holds its genotypes as a dense typed integer array, normally one byte per allele.  ``sai_bcf_decode``
(bcf/bcf_decode.hip) recodes the arrays of the selected rows into the int8 [record][sample] block ``sai_tokenize_gt``
writes for the same calls as VCF text, so everything behind the reader is shared with the VCF route.  Two routes
bring the arrays to it:

* the GPU route (``_load_device_walk``; the default of ``load_dosage_device`` unless ``SAI_AMD_GPU_INFLATE=0``): the
  compressed members cross PCIe as they are (``sai_bcf_feed_*``), ``sai_inflate_bgzf``
  inflates them, ``sai_bcf_chain_segments`` / ``sai_bcf_stitch`` / ``sai_bcf_record_heads`` (bcf/bcf_walk.hip,
  bcf/bcf_feed.cpp) find the records, 64 bytes per record come back for the row selection, and the GT arrays are
  decoded where the inflater left them.  Anything unusual -- a member the inflater refuses, a chain the stitch cannot
  follow, a selected row with an error flag, a row the decoder flags -- throws the partial result away and runs
* the host route from the start (``sai_bcf_stream_*``, bcf/bcf_index.cpp): the host inflates the members with several
  threads, walks the record chain, selects the rows and copies the GT array of every selected row -- nothing else of
  the record -- into two staging buffers in turn.  It words every error about the file (profiles/bcf_ingest.txt,
  profiles/bcf_gpu_walk.txt).

A read of a region with a current ``<path>.csi`` beside the file begins, on both routes, at the virtual offset that
index names (``_index_for``; ``sai_bcf_stream_open_at`` / ``sai_bcf_feed_open_at``, bcf/csi_index.cpp); whatever is
unusual about the index only means that the read walks from the start of the file, as it does without one
(DESIGN_INGEST.md, "BCF files: a region is a seek"; ``SAI_AMD_BCF_INDEX=0`` switches it off).

The format rules as they are implemented, what of them has not been checked against ``bcftools``, and what is refused
are in DESIGN_INGEST.md ("BCF files" and "BCF files: members inflated and records found on the GPU").

The surface is that of the fileset readers: ``fileset_prefix`` (the path itself when it is a BCF: detection is by
content), ``scan_first_last``, ``load_dosage`` / ``load_dosage_device`` (what ``native_vcf.load_dosage`` /
``device_vcf.load_dosage_device`` return) and ``release_buffers``.  Every request of a (sample, ploidy) is a slot.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from .. import _ffi, _ffi_bcf, _ffi_bcf_device, _ffi_bcf_index
from ._ingest import check_io, default_threads, pair, region_args, staging

BUFFER_BYTES = 32 << 20  # as the other routes; SAI_AMD_INGEST_BUFFER overrides it

SEG_BYTES = 16384  # SAI_AMD_BCF_SEG_BYTES overrides it for tools/bcf_rate.py (a power of two in 256 .. 65536)
CARRY_ROOM = 64 << 20  # at most this much of a batch's tail is carried in front of the next one

_probed: dict = {}  # (path, size, mtime) -> is a BCF
_scanned: dict = {}  # (path, size, mtime, chromosome) -> (first, last, n_records_total, n_samples)
_indexes: dict = {}  # (path, size, mtime, index size, index mtime) -> the sai_bcf_index handle, or None: not usable


def _file_key(path):
    text = os.fspath(path)
    st = os.stat(text)
    return (os.path.abspath(text), st.st_size, st.st_mtime_ns)


def fileset_prefix(path) -> Optional[str]:
    """The path itself when it names a BGZF file whose inflated stream starts as a BCF (``sai_bcf_probe``), else
    None.  The name does not matter; the answer is remembered per (path, size, mtime)."""
    if path is None:
        return None
    text = os.fspath(path)
    try:
        if not os.path.isfile(text):
            return None
        key = _file_key(text)
        if key not in _probed:
            with open(text, "rb") as f:
                gz = f.read(2) == b"\x1f\x8b"  # only a gzip member is worth inflating
            _probed[key] = bool(gz and _ffi_bcf.load_host().sai_bcf_probe(os.fsencode(text)))
        return text if _probed[key] else None
    except OSError:
        return None


def is_fileset(path) -> bool:
    return fileset_prefix(path) is not None


def _index_for(path, start, end):
    """The handle of ``<path>.csi`` for a read with ``start`` or ``end`` given, or None: no region, no index beside
    the file, ``SAI_AMD_BCF_INDEX=0``, an index older than the file (whole seconds, as for a ``.tbi``) or one that does
    not parse or fails a check.  None is never an error: the read walks from the start of the file.  Opened once per
    (path, size, mtime, index size, index mtime) and kept for the life of the process, like the scan results."""
    if (start is None and end is None) or os.environ.get("SAI_AMD_BCF_INDEX", "1") == "0":
        return None
    try:
        text = os.fspath(path)
        ist = os.stat(text + ".csi")
        key = (*_file_key(text), ist.st_size, ist.st_mtime_ns)
    except OSError:
        return None
    if key not in _indexes:
        handle = None
        if ist.st_mtime_ns // 10**9 >= key[2] // 10**9:
            lib, opened = _ffi_bcf_index.load_host(), C.c_void_p()
            if lib.sai_bcf_index_open(os.fsencode(text + ".csi"), key[1], C.byref(opened)) == 0:
                handle = opened
        _indexes[key] = handle
    return _indexes[key]


def _gpu_walk_wanted() -> bool:
    return os.environ.get("SAI_AMD_GPU_INFLATE", "1") != "0" and os.environ.get("SAI_AMD_INGEST", "device") != "host"


def _scan_on_device(path, chr_name: str):
    """The scan through the GPU route -- no samples, nothing decoded, every record of the file counted -- or None
    where there is no GPU, the knob says no or the route hands the file over: the host scan says what is wrong."""
    if not _gpu_walk_wanted():
        return None
    try:
        import torch

        if not torch.cuda.is_available():
            return None
        from ..engine import Engine

        eng = Engine.get()
        icap = int(os.environ.get("SAI_AMD_INFLATE_BATCH", 0)) or _inflate_batch(path)
        return _load_device_walk(eng, path, chr_name, [], [], None, None, None, icap, None, whole_file=True)[4]
    except (ImportError, ValueError, _HostRoute):
        return None


def _scan(path, chr_name: str):
    key = (*_file_key(path), str(chr_name))
    if key not in _scanned:
        got = _scan_on_device(path, chr_name)
        if got is None:
            lib = _ffi_bcf.load_host()
            v = [C.c_int64(-1) for _ in range(4)]
            check_io(lib, lib.sai_bcf_scan(os.fsencode(path), str(chr_name).encode(), *[C.byref(x) for x in v]))
            got = tuple(int(x.value) for x in v)
        _scanned[key] = got
    return _scanned[key]


def scan_first_last(path, chr_name: str):
    """First and last position of the first contiguous run of ``chr_name`` (None, None if absent):
    ``native_vcf.scan_first_last`` for a BCF.  One walk of the whole file, remembered per (path, size, mtime,
    chromosome) for the life of the process."""
    first, last, _, _ = _scan(path, chr_name)
    return (None, None) if first < 0 else (first, last)


def header_counts(path) -> tuple:
    """(records of the file, samples of its header): what stays resident is their product.  A BCF has no record
    count in its header, so this is a walk of the whole file -- ``sai_bcf_scan`` counts while it looks for a
    chromosome, and any chromosome's remembered scan answers; where there is none yet, the scan is asked for the
    empty name, which no contig has: it selects nothing and counts everything (and is remembered like the others)."""
    for key, got in _scanned.items():
        if key[:3] == _file_key(path):
            return got[2], got[3]
    _, _, n_records, n_samples = _scan(path, "")
    return n_records, n_samples


def _cap(buffer_bytes) -> int:
    return int(buffer_bytes or os.environ.get("SAI_AMD_INGEST_BUFFER", BUFFER_BYTES))


class _Stream:
    """One ``sai_bcf_stream``: the batches of a region and, once the first has come, the selection."""

    def __init__(self, lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, buffers, cap, index=None):
        self.lib, self.path, self.chr_name = lib, os.fspath(path), str(chr_name)
        self.samples = list(samples)
        self.ploidies = np.asarray([int(p) for p in ploidies], dtype=np.int32)
        self.handle = C.c_void_p()
        args = region_args(path, chr_name, start, end, samples, ploidies, anc_allele_file, n_threads)
        if index is None:
            check_io(lib, lib.sai_bcf_stream_open(*args, C.c_void_p(buffers[0]), C.c_void_p(buffers[1]), cap, C.byref(self.handle)))
        else:
            check_io(lib, lib.sai_bcf_stream_open_at(*args, C.c_void_p(buffers[0]), C.c_void_p(buffers[1]), cap, index, C.byref(self.handle)))
        self.cols = None  # int32 [n slots]: the sample column of every slot
        self.n_cols = 0
        self.first_col = self.uniform_ploidy = -1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.sai_bcf_stream_close(self.handle)
        self.handle = None

    def next(self):
        """(buffer, bytes, pos, flip, off, width, L) of the next batch -- copies of the tables -- or None at the end."""
        buf, n_bytes, n_rows, done = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
        ptrs = [C.c_void_p() for _ in range(5)]
        check_io(self.lib, self.lib.sai_bcf_stream_next(self.handle, C.byref(buf), C.byref(n_bytes), C.byref(n_rows),
                                                        *[C.byref(p) for p in ptrs], C.byref(done)))  # fmt: skip
        if done.value:
            return None
        n = int(n_rows.value)
        kinds = ((C.c_int32, np.int32), (C.c_uint8, np.uint8), (C.c_int64, np.int64), (C.c_uint8, np.uint8), (C.c_int32, np.int32))
        tables = [np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)
                  for p, (ct, dt) in zip(ptrs, kinds)]  # fmt: skip
        if self.cols is None:
            self._select()
        return (int(buf.value), int(n_bytes.value), *tables)

    def _select(self) -> None:
        n = len(self.samples)
        cols, n_file = np.empty(max(n, 1), dtype=np.int32), C.c_int32()
        check_io(self.lib, self.lib.sai_bcf_stream_selection(self.handle, cols.ctypes.data_as(C.c_void_p), n, C.byref(n_file), None, None))
        self.cols, self.n_cols = cols[:n].copy(), int(n_file.value)
        # the two promises that select the kernel's fast path
        self.first_col = int(cols[0]) if n and np.array_equal(self.cols, np.arange(cols[0], cols[0] + n, dtype=np.int32)) else -1
        self.uniform_ploidy = int(self.ploidies[0]) if n and bool((self.ploidies == self.ploidies[0]).all()) else 0

    def stats(self) -> dict:
        """The producer's seconds by phase and its byte counts (``sai_bcf_stream_stats``), once the stream is read to its end."""
        t = [C.c_double() for _ in range(5)]
        n = [C.c_int64() for _ in range(2)]
        check_io(self.lib, self.lib.sai_bcf_stream_stats(self.handle, *[C.byref(x) for x in t], *[C.byref(x) for x in n]))
        names = ("file_read", "inflate", "walk", "copy_to_staging", "wait_for_buffer")
        return {**{k: float(x.value) for k, x in zip(names, t)}, "inflated_bytes": int(n[0].value), "staged_bytes": int(n[1].value),
                "seek": self.seek()}  # fmt: skip

    def seek(self) -> dict:
        """Whether the producer began at a virtual offset of the index, which one, and the bytes of the file and the
        members it inflated (``sai_bcf_stream_seek_stats``), once the stream is read to its end."""
        lib = _ffi_bcf_index.load_host()
        made, v, n_bytes, n_members = C.c_int32(), C.c_uint64(), C.c_int64(), C.c_int64()
        check_io(lib, lib.sai_bcf_stream_seek_stats(self.handle, C.byref(made), C.byref(v), C.byref(n_bytes), C.byref(n_members)))
        return {"made": bool(made.value), "voffset": int(v.value), "file_bytes": int(n_bytes.value), "members": int(n_members.value)}

    def counts(self) -> tuple:
        """(rows matched before polarisation, entries of the ancestral-allele table) of the finished walk."""
        n_matched, n_anc = C.c_int64(), C.c_int64()
        if self.lib.sai_bcf_stream_selection(self.handle, None, 0, None, C.byref(n_matched), C.byref(n_anc)):
            return 0, 0
        return int(n_matched.value), int(n_anc.value)

    def raise_flagged(self, buf, n_bytes, pos, flip, off, width, length, status) -> None:
        """The first flagged row of a batch as the reader's ValueError, naming the record and the sample."""
        bad = np.flatnonzero(status)
        if bad.size == 0:
            return
        r, st = int(bad[0]), int(status[bad[0]])
        where, name = f"{self.chr_name}:{int(pos[r])}", None
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        one, one_status = np.zeros(1, dtype=np.int8), np.zeros(1, dtype=np.int32)
        for s in range(len(self.samples)):  # the error path: slot by slot until one says it
            check_io(self.lib, self.lib.sai_bcf_decode_host(ptr(buf), n_bytes, 1, ptr(off[r : r + 1]), ptr(width[r : r + 1]), ptr(length[r : r + 1]),
                                                            ptr(flip[r : r + 1]), self.n_cols, 1, ptr(self.cols[s : s + 1]),
                                                            ptr(self.ploidies[s : s + 1]), ptr(one), ptr(one_status), 1))  # fmt: skip
            if int(one_status[0]) == st:
                name = self.samples[s]
                break
        if st == _ffi_bcf.SAI_BCF_STATUS_RANGE:
            raise ValueError(f"{self.path}: dosage outside the int8 range at {where} (sample {name})")
        if st == _ffi_bcf.SAI_BCF_STATUS_BAD_VALUE:
            raise ValueError(f"{self.path}: record {where}: the GT vector of sample {name} holds a reserved value: the record is damaged")
        raise ValueError(f"{self.path}: record {where} was decoded with an index outside its range")


def load_dosage(path, chr_name: str, samples: Sequence[str], ploidies: Sequence[int], start: Optional[int] = None,
                end: Optional[int] = None, anc_allele_file: Optional[str] = None, n_threads: Optional[int] = None,
                buffer_bytes: Optional[int] = None, trace: Optional[dict] = None):  # fmt: skip
    """(pos int32 [n], dosage int8 [n][len(samples)], n_matched, n_anc_entries) for one region, decoded on the
    host (``sai_bcf_decode_host``): the ``SAI_AMD_INGEST=host`` route and the yardstick of the kernel.  With a region
    and a current ``<path>.csi`` the stream begins where the index says (``_index_for``); a read that began there and
    fails is read again from the start of the file, so the index never words an error.  ``trace`` (a dict) gets the
    stream's stats, ``seek`` among them."""
    index = _index_for(path, start, end)
    if index is not None:
        try:
            return _load_dosage(path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, buffer_bytes, trace, index)
        except ValueError:
            pass
    return _load_dosage(path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, buffer_bytes, trace, None)


def _load_dosage(path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, buffer_bytes, trace, index):
    lib = _ffi_bcf.load_host()
    n_threads = n_threads or default_threads()
    cap, n = _cap(buffer_bytes), len(samples)
    bufs = [np.empty(cap, dtype=np.uint8) for _ in range(2)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pos_parts, dos_parts = [], []
    with _Stream(lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, [b.ctypes.data for b in bufs], cap, index) as stream:
        while True:
            got = stream.next()
            if got is None:
                break
            b, n_bytes, pos, flip, off, width, length = got
            pos_parts.append(pos)
            dos = np.empty((len(pos), n), dtype=np.int8)
            if n and len(pos):
                status = np.empty(len(pos), dtype=np.int32)
                check_io(lib, lib.sai_bcf_decode_host(ptr(bufs[b]), n_bytes, len(pos), ptr(off), ptr(width), ptr(length), ptr(flip), stream.n_cols, n,
                                                      ptr(stream.cols), ptr(stream.ploidies), ptr(dos), ptr(status), n_threads))  # fmt: skip
                stream.raise_flagged(bufs[b], n_bytes, pos, flip, off, width, length, status)
            dos_parts.append(dos)
        n_matched, n_anc = stream.counts()
        if trace is not None:
            trace.update(stream.stats())
    pos = np.concatenate(pos_parts) if pos_parts else np.zeros(0, dtype=np.int32)
    dos = np.concatenate(dos_parts) if dos_parts else np.zeros((0, n), dtype=np.int8)
    return pos, dos, n_matched, n_anc


def release_buffers(eng) -> None:
    """Drop the staging ``load_dosage_device`` keeps between calls."""
    for key in ("_bcf_state", "_bcf_walk_state"):
        st = eng.__dict__.pop(key, None)
        if st:
            st["stream"].synchronize()
            st.clear()


class _HostRoute(Exception):
    """The GPU route does not serve this read: the host route takes it from the start."""


def _inflate_batch(path) -> int:
    from .device_vcf import _inflate_batch_for

    return _inflate_batch_for(path)


def load_dosage_device(eng, path, chr_name: str, samples: Sequence[str], ploidies: Sequence[int],
                       start: Optional[int] = None, end: Optional[int] = None, anc_allele_file: Optional[str] = None,
                       n_threads: Optional[int] = None, buffer_bytes: Optional[int] = None, trace: Optional[dict] = None):  # fmt: skip
    """(pos int32 host array [n], dosage int8 DEVICE tensor [n][len(samples)], n_matched, n_anc_entries):
    ``load_dosage`` with the result left in HBM.  The GPU route (``_load_device_walk``) unless ``SAI_AMD_GPU_INFLATE=0``,
    in batches of ``SAI_AMD_INFLATE_BATCH`` inflated bytes (default: by the file's size,
    as for a bgzip VCF); where that route hands the read over, and otherwise, the host route (``_load_host_inflate``).
    ``trace`` (a dict) gets ``route`` = ``"device"`` / ``"host"``, the route's seconds per phase and ``seek``: whether
    the read began at a virtual offset of ``<path>.csi`` (``_index_for``), which one, and the bytes of the file read.
    A read that began there and does not come through -- on either route -- is made again from the start of the file
    on the same route, exactly as without an index."""
    index = _index_for(path, start, end)
    attempts = [index, None] if index is not None else [None]
    if _gpu_walk_wanted():
        icap = int(os.environ.get("SAI_AMD_INFLATE_BATCH", 0)) or _inflate_batch(path)
        for ix in attempts:
            try:
                got = _load_device_walk(eng, path, chr_name, samples, ploidies, start, end, anc_allele_file, icap, trace, index=ix)
                if trace is not None:
                    trace["route"] = "device"
                return got[:4]
            except _HostRoute:
                pass
            except ValueError:
                if ix is None:
                    raise
    if trace is not None:
        trace["route"] = "host"
    if index is not None:
        try:
            return _load_host_inflate(eng, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, buffer_bytes, trace, index)
        except ValueError:
            pass
    return _load_host_inflate(eng, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, buffer_bytes, trace)


def _load_device_walk(eng, path, chr_name, samples, ploidies, start, end, anc_allele_file, icap, trace, whole_file=False, index=None):
    """(pos, dosage, n_matched, n_anc, (first, last, records seen, samples of the file)) through the GPU route, or
    ``_HostRoute``.  Per batch, on a side stream: the compressed members and their table go to the device; ``sai_inflate_bgzf`` writes their
    text behind the carry of the batch before; ``sai_bcf_chain_segments`` summarises every segment and the summaries
    come back for ``sai_bcf_stitch``; ``sai_bcf_record_heads`` writes a head per record and the heads come back for
    ``sai_bcf_feed_select``; the row tables go up and ``sai_bcf_decode`` reads the GT arrays out of the text.  The
    bytes from the first incomplete record on are copied, device to device, to the front of the other text buffer.
    The feed's thread reads batch k + 1 from the file meanwhile.  With ``trace["serial"]`` the stream is synchronised
    behind every step, so ``h2d``, ``inflate_gpu``, ``walk_gpu`` and ``decode`` are timed on their own.

    With ``index`` (``sai_bcf_feed_open_at``) the first batch's members start at the ``coffset`` the index names and
    the stitch's known entry is its ``uoffset``.  The text in front of it holds the end of earlier records, whose
    chains run into ``uoffset``, so it is cleared first: the stitch wants its entry to be the head of a chain.  An
    entry that is no record start, a first record of another contig or a broken chain is ``_HostRoute("seek")`` or the
    stitch's own verdict, and the caller reads from the start of the file."""
    import time

    import torch

    _ffi_bcf.load()
    lib = _ffi_bcf_device.load()
    n, text_path = len(samples), os.fspath(path)
    seg_bytes, max_heads = int(os.environ.get("SAI_AMD_BCF_SEG_BYTES", SEG_BYTES)), _ffi_bcf_device.SAI_BCF_MAX_HEADS
    room = min(icap, CARRY_ROOM)
    text_cap = room + max(icap, 65536)
    comp_cap = max(icap // 2, 1 << 17) + 65540  # a batch is closed early when its members fill this first
    st = staging(eng, "_bcf_walk_state", icap, lambda: {"pinned": pair(comp_cap), "comp": pair(comp_cap, device=eng.device),
                                                        "text": pair(text_cap + 16, device=eng.device),
                                                        "stream": torch.cuda.Stream(device=eng.device)})  # fmt: skip
    pinned, comp_dev, text_dev, side = st["pinned"], st["comp"], st["text"], st["stream"]
    current = torch.cuda.current_stream(eng.device)
    side.wait_stream(current)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    names = (C.c_char_p * n)(*[s.encode() for s in samples])
    feed = C.c_void_p()
    ilib = _ffi_bcf_index.load()
    rc = ilib.sai_bcf_feed_open_at(os.fsencode(text_path), str(chr_name).encode(), -1 if start is None else int(start), -1 if end is None else int(end),
                                   n, names, os.fsencode(anc_allele_file) if anc_allele_file else None, C.c_void_p(pinned[0].data_ptr()),
                                   C.c_void_p(pinned[1].data_ptr()), comp_cap, icap, int(whole_file), index, C.byref(feed))  # fmt: skip
    if rc:
        raise _HostRoute("open")

    def seek_stats():
        made, v, contig, n_file_bytes, n_members = C.c_int32(), C.c_uint64(), C.c_int32(), C.c_int64(), C.c_int64()
        ilib.sai_bcf_feed_seek_stats(feed, C.byref(made), C.byref(v), C.byref(contig), C.byref(n_file_bytes), C.byref(n_members))
        return {"made": bool(made.value), "voffset": int(v.value), "file_bytes": int(n_file_bytes.value), "members": int(n_members.value)}, int(contig.value)

    serial = trace is not None and trace.get("serial")
    laps = {}

    def lap(name, t1):
        if serial:
            side.synchronize()
            laps[name] = laps.get(name, 0.0) + time.perf_counter() - t1
        return time.perf_counter()

    pos_parts, outs, stats = [], [], []
    try:
        n_contigs, n_file, gt_key = C.c_int32(), C.c_int32(), C.c_int64()
        lib.sai_bcf_feed_selection(feed, None, 0, None, 0, C.byref(n_contigs), C.byref(n_file), C.byref(gt_key), *[None] * 5)
        contigs, cols = np.zeros(max(n_contigs.value, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32)
        check_io(lib, lib.sai_bcf_feed_selection(feed, ptr(cols), n, ptr(contigs), n_contigs.value, *[None] * 8))
        cols, n_cols = cols[:n].copy(), int(n_file.value)
        pl = np.asarray([int(p) for p in ploidies], dtype=np.int32)
        first_col = int(cols[0]) if n and np.array_equal(cols, np.arange(cols[0], cols[0] + n, dtype=np.int32)) else -1
        uniform = int(pl[0]) if n and bool((pl == pl[0]).all()) and 1 <= int(pl[0]) <= 64 else 0
        if n and (int(pl.min()) < 1 or int(pl.max()) > 64):
            raise _HostRoute("ploidy")  # the host route words it
        with torch.cuda.stream(side):
            d_contigs = torch.from_numpy(contigs).to(eng.device)
            d_cols = torch.from_numpy(cols).to(eng.device) if n and first_col < 0 else None
            d_pl = torch.from_numpy(pl).to(eng.device) if n and uniform == 0 else None
        carry, done = 0, False
        seek, contig = seek_stats()
        unchecked = seek["made"]  # the first record from the seek on has to be one of the chromosome's
        first_batch = True
        while not done:
            b, n_comp, n_members, n_text, e0, end_of_file = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
            members = C.c_void_p()
            if lib.sai_bcf_feed_next(feed, C.byref(b), C.byref(n_comp), C.byref(n_members), C.byref(members), C.byref(n_text), C.byref(e0),
                                     C.byref(end_of_file)):  # fmt: skip
                raise _HostRoute("reader")
            if end_of_file.value:
                break
            b, n_comp, nm, n_text = int(b.value), int(n_comp.value), int(n_members.value), int(n_text.value)
            n_bytes = carry + n_text  # at most text_cap: carry <= room, and a batch is icap bytes or one member
            entry = 0 if carry else int(e0.value)
            clear = entry if seek["made"] and first_batch else 0
            first_batch = False
            if clear > n_text:
                raise _HostRoute("seek")  # uoffset lies behind its member
            table = np.ctypeslib.as_array(C.cast(members, C.POINTER(C.c_uint8)), shape=(nm * 32,)).copy()
            n_seg = -(-n_bytes // seg_bytes)
            text = text_dev[b]
            with torch.cuda.stream(side):
                t1 = time.perf_counter()
                comp_dev[b][:n_comp].copy_(pinned[b][:n_comp], non_blocking=True)
                d_table = torch.from_numpy(table).to(eng.device, non_blocking=True)
                t1 = lap("h2d", t1)
                d_member_status = torch.empty((nm,), dtype=torch.int32, device=eng.device)
                _ffi.check(lib.sai_inflate_bgzf(eng.ctx, C.c_void_p(comp_dev[b].data_ptr()), n_comp, C.c_void_p(d_table.data_ptr()), nm,
                                                C.c_void_p(text.data_ptr() + carry), n_text, C.c_void_p(d_member_status.data_ptr()),
                                                C.c_void_p(side.cuda_stream)))  # fmt: skip
                if clear:
                    text[:clear].zero_()
                t1 = lap("inflate_gpu", t1)
                d_chains = torch.empty((n_seg * max_heads * 16,), dtype=torch.uint8, device=eng.device)
                d_info = torch.empty((n_seg,), dtype=torch.int32, device=eng.device)
                _ffi.check(lib.sai_bcf_chain_segments(eng.ctx, C.c_void_p(text.data_ptr()), n_bytes, seg_bytes, max_heads, C.c_void_p(d_contigs.data_ptr()),
                                                      int(n_contigs.value), n_cols, C.c_void_p(d_chains.data_ptr()), C.c_void_p(d_info.data_ptr()),
                                                      C.c_void_p(side.cuda_stream)))  # fmt: skip
                bad_members = int(d_member_status.count_nonzero())  # waits for the stream
                chains, info = d_chains.cpu().numpy(), d_info.cpu().numpy()
                lib.sai_bcf_feed_release(feed)  # the compressed bytes and the table have left their buffer
                if bad_members:
                    raise _HostRoute("member")
                seg_entry, seg_first = np.empty(n_seg, dtype=np.int64), np.empty(n_seg, dtype=np.int64)
                n_records, carry_from, verdict = C.c_int64(), C.c_int64(), C.c_int32()
                check_io(lib, lib.sai_bcf_stitch(ptr(chains), ptr(info), n_bytes, seg_bytes, max_heads, entry, ptr(seg_entry), ptr(seg_first),
                                                 C.byref(n_records), C.byref(carry_from), C.byref(verdict)))  # fmt: skip
                if verdict.value:
                    raise _HostRoute("stitch")
                n_records, carry_from = int(n_records.value), int(carry_from.value)
                heads = np.zeros(0, dtype=_ffi_bcf_device.HEAD)
                if n_records:
                    d_entry, d_first = torch.from_numpy(seg_entry).to(eng.device, non_blocking=True), torch.from_numpy(seg_first).to(eng.device, non_blocking=True)
                    d_heads = torch.empty((n_records * 64,), dtype=torch.uint8, device=eng.device)
                    _ffi.check(lib.sai_bcf_record_heads(eng.ctx, C.c_void_p(text.data_ptr()), n_bytes, seg_bytes, C.c_void_p(d_entry.data_ptr()),
                                                        C.c_void_p(d_first.data_ptr()), carry_from, n_records, int(gt_key.value), int(n > 0),
                                                        C.c_void_p(d_heads.data_ptr()), C.c_void_p(side.cuda_stream)))  # fmt: skip
                    heads = d_heads.cpu().numpy().view(_ffi_bcf_device.HEAD)
                t1 = lap("walk_gpu", t1)
            if unchecked and n_records:
                if int(heads[0]["chrom"]) != contig:
                    raise _HostRoute("seek")
                unchecked = False
            n_rows, sel_done, verdict = C.c_int64(), C.c_int32(), C.c_int32()
            tabs = [C.c_void_p() for _ in range(5)]
            check_io(lib, lib.sai_bcf_feed_select(feed, ptr(heads), n_records, C.byref(n_rows), *[C.byref(t) for t in tabs], C.byref(sel_done),
                                                  C.byref(verdict)))  # fmt: skip
            if verdict.value:
                raise _HostRoute("select")
            done, nr = bool(sel_done.value), int(n_rows.value)
            kinds = ((C.c_int32, np.int32), (C.c_uint8, np.uint8), (C.c_int64, np.int64), (C.c_uint8, np.uint8), (C.c_int32, np.int32))
            pos, flip, off, width, length = (np.ctypeslib.as_array(C.cast(t, C.POINTER(ct)), shape=(nr,)).astype(dt, copy=True) if nr
                                             else np.zeros(0, dtype=dt) for t, (ct, dt) in zip(tabs, kinds))  # fmt: skip
            pos_parts.append(pos)
            if n and nr:
                out = torch.empty((nr, n), dtype=torch.int8, device=eng.device)
                status = torch.empty((nr,), dtype=torch.int32, device=eng.device)
                side.wait_stream(current)
                with torch.cuda.stream(side):
                    t1 = time.perf_counter()
                    d_off, d_width, d_len, d_flip = (torch.from_numpy(a).to(eng.device, non_blocking=True) for a in (off, width, length, flip))
                    _ffi.check(lib.sai_bcf_decode(eng.ctx, C.c_void_p(text.data_ptr()), n_bytes, nr, eng._ptr(d_off), eng._ptr(d_width), eng._ptr(d_len),
                                                  eng._ptr(d_flip), n_cols, n, eng._ptr(d_cols), first_col, eng._ptr(d_pl), uniform,
                                                  C.c_void_p(out.data_ptr()), 0, eng._ptr(status), C.c_void_p(side.cuda_stream)))  # fmt: skip
                    t1 = lap("decode", t1)
                outs.append(out)
                stats.append(status)
            carry = n_bytes - carry_from
            if done:  # the selection has stopped: what lies behind the region is not looked at, as on the host
                break
            if carry > room:
                raise ValueError(f"{text_path}: a record does not fit a batch of {icap} inflated bytes: raise SAI_AMD_INFLATE_BATCH")
            if carry:
                with torch.cuda.stream(side):
                    text_dev[b ^ 1][:carry].copy_(text[carry_from:n_bytes], non_blocking=True)
        if not done and carry:
            raise _HostRoute("trailing bytes")  # the stream ends inside a record: the host route words it
        v = [C.c_int64() for _ in range(5)]
        check_io(lib, lib.sai_bcf_feed_selection(feed, None, 0, None, 0, None, None, None, *[C.byref(x) for x in v]))
        n_matched, n_anc, n_seen, first, last = (int(x.value) for x in v)
        if trace is not None:
            t = [C.c_double() for _ in range(4)]
            comp_bytes = C.c_int64()
            lib.sai_bcf_feed_stats(feed, *[C.byref(x) for x in t], C.byref(comp_bytes))
            trace.update({k: float(x.value) for k, x in zip(("file_read", "header_inflate", "select", "wait_for_buffer"), t)})
            trace.update(laps, comp_bytes=int(comp_bytes.value), seek=seek_stats()[0])
    finally:
        lib.sai_bcf_feed_close(feed)
        side.synchronize()  # also on an error: the staging buffers are reused by the next call
    if stats and bool(torch.cat(stats).any()):
        raise _HostRoute("a flagged row")
    current.wait_stream(side)
    pos = np.concatenate(pos_parts) if pos_parts else np.zeros(0, dtype=np.int32)
    dos = torch.cat(outs) if len(outs) > 1 else outs[0] if outs else torch.empty((len(pos), n), dtype=torch.int8, device=eng.device)
    return pos, dos, n_matched, n_anc, (first, last, n_seen, n_cols)


def _load_host_inflate(eng, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, buffer_bytes, trace, index=None):
    """The host route of ``load_dosage_device``.  The loop of ``device_vcf.load_dosage_device``: the producer thread
    fills one pinned buffer while the other one is copied on a side stream and decoded behind the copy; the producer
    may refill a buffer once its copy has left it.  A row the kernel flags is handed to the host route, which raises
    the error that names the record and the sample.  ``trace`` (a dict) collects the producer's seconds per phase
    (``_Stream.stats``: file_read, inflate, walk, copy_to_staging, wait_for_buffer, and the bytes inflated and staged);
    with ``trace["serial"]`` set the side stream is synchronised behind every copy and every kernel, so ``h2d`` and
    ``decode`` are timed on their own, by the host clock (and nothing overlaps)."""
    import time

    import torch

    _ffi_bcf.load()
    lib = eng.lib
    cap, n = _cap(buffer_bytes), len(samples)
    st = staging(eng, "_bcf_state", cap, lambda: {"pinned": pair(cap), "rows": pair(cap, device=eng.device),
                                                  "stream": torch.cuda.Stream(device=eng.device)})  # fmt: skip
    pinned, dev_rows, side = st["pinned"], st["rows"], st["stream"]
    current = torch.cuda.current_stream(eng.device)
    side.wait_stream(current)  # the outputs are allocated on the current stream: what used their memory before is done first
    pos_parts, outs, stats, tables = [], [], [], [None, None]
    cols_dev = ploidy_dev = None  # only where the promises of the fast path do not hold
    try:
        with _Stream(lib, path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, [t.data_ptr() for t in pinned], cap, index) as stream:
            copied = None
            while True:
                if copied is not None:
                    copied.synchronize()  # the H2D copy of the previous batch has left its pinned buffer
                got = stream.next()
                if got is None:
                    break
                b, n_bytes, pos, flip, off, width, length = got
                pos_parts.append(pos)
                if n == 0 or len(pos) == 0:
                    continue
                out = torch.empty((len(pos), n), dtype=torch.int8, device=eng.device)
                status = torch.empty((len(pos),), dtype=torch.int32, device=eng.device)
                serial = trace is not None and trace.get("serial")
                with torch.cuda.stream(side):
                    t1 = time.perf_counter()
                    dev_rows[b][:n_bytes].copy_(pinned[b][:n_bytes], non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(side)
                    if serial:
                        side.synchronize()
                        trace["h2d"] = trace.get("h2d", 0.0) + time.perf_counter() - t1
                        t1 = time.perf_counter()
                    if cols_dev is None and stream.first_col < 0:
                        cols_dev = torch.from_numpy(stream.cols).to(eng.device)
                    if ploidy_dev is None and stream.uniform_ploidy <= 0:
                        ploidy_dev = torch.from_numpy(stream.ploidies).to(eng.device)
                    d_off, d_width, d_len, d_flip = (torch.from_numpy(a).to(eng.device, non_blocking=True) for a in (off, width, length, flip))
                    tables[b] = (d_off, d_width, d_len, d_flip)  # those of two batches back go: allocated and used on this stream alone
                    _ffi.check(
                        lib.sai_bcf_decode(eng.ctx, C.c_void_p(dev_rows[b].data_ptr()), n_bytes, len(pos), eng._ptr(d_off), eng._ptr(d_width),
                                           eng._ptr(d_len), eng._ptr(d_flip), stream.n_cols, n,
                                           eng._ptr(cols_dev), stream.first_col, eng._ptr(ploidy_dev), max(stream.uniform_ploidy, 0),
                                           C.c_void_p(out.data_ptr()), 0, eng._ptr(status), C.c_void_p(side.cuda_stream))
                    )  # fmt: skip
                    if serial:
                        side.synchronize()
                        trace["decode"] = trace.get("decode", 0.0) + time.perf_counter() - t1
                outs.append(out)
                stats.append(status)
            n_matched, n_anc = stream.counts()
            if trace is not None:
                trace.update(stream.stats())
    finally:
        side.synchronize()  # also on an error: the staging buffers are reused by the next call
    if stats and bool(torch.cat(stats).any()):
        _load_dosage(path, chr_name, samples, ploidies, start, end, anc_allele_file, n_threads, buffer_bytes, None, None)
        raise ValueError(f"{os.fspath(path)}: the GPU decoder flagged a row the host reader accepts")
    current.wait_stream(side)
    pos = np.concatenate(pos_parts) if pos_parts else np.zeros(0, dtype=np.int32)
    if not outs:
        return pos, torch.empty((len(pos), n), dtype=torch.int8, device=eng.device), n_matched, n_anc
    return pos, torch.cat(outs) if len(outs) > 1 else outs[0], n_matched, n_anc
