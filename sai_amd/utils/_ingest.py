"""The steps the ingest readers share (``native_vcf``, ``device_vcf``, ``plink``): the region / sample
arguments of the C ABI, its errors as ValueError, the staging kept on the engine, and -- ``Records`` --
what the two GPU-tokenising VCF routes do with the record lines of a batch."""

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
