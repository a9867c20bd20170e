#!/usr/bin/env python3
"""Rate of `sai convert --out-eigenstrat`, the two kernels behind it and `sai_bed_encode` beside them, in one process.

Writes, from a seed, a matrix of --rows records x --samples phased diploid calls on chromosome 1 as plain VCF text
(``tools/bed_export_rate.py``'s generator; writing is not timed).  Then, with the file in the page cache:

  (a) the kernels over the whole block, timed with device events after a warm-up round, in turn:
      ``sai_bed_encode`` (the yardstick of the packed kernel: the same 16 bytes read and 4 bytes written per lane),
      ``sai_geno_encode``, and ``sai_geno_encode_transposed`` -- every slot group of the converter's batch budget, the
      calls summed.  The order of the three is reversed every other round, so that no kernel always starts on what
      the same predecessor left in the last-level cache; every run's predecessor is printed.  Medians with min - max over --repeats; GB/s of block bytes;
  (b) ``convert`` end to end with its phase table for ``--out-bfile``, ``--out-eigenstrat`` packed and
      ``--out-eigenstrat`` transposed, alternating, and the phase that bounds each.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for entry_dir in (ROOT, ROOT / "tests", ROOT / "tools"):
    if str(entry_dir) not in sys.path:
        sys.path.insert(0, str(entry_dir))


def fmt(values, unit="ms"):
    ordered = sorted(values)
    return f"median {ordered[len(ordered) // 2]:.3f} {unit} (min {ordered[0]:.3f} - max {ordered[-1]:.3f}; " + " ".join(f"{v:.3f}" for v in values) + ")"


def median(values):
    return sorted(values)[len(values) // 2]


def kernel_figures(eng, dos, repeats):
    """(a): {name: [ms per repeat]}, alternating; and the slot groups of the transposed form."""
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import bed_writer, geno_writer

    lib = geno_writer.load()
    bed_writer.load()
    n_rows, n_slots = dos.shape
    groups, rlen_t = geno_writer._batches(True, n_rows, n_slots)
    rlen = geno_writer.record_bytes(n_slots)
    out = torch.empty((max(n_rows * rlen, n_slots * rlen_t),), dtype=torch.uint8, device=eng.device)
    status = torch.zeros((n_rows,), dtype=torch.int32, device=eng.device)
    stream = torch.cuda.current_stream(eng.device)
    st, ptr = C.c_void_p(stream.cuda_stream), lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def bed():
        _ffi.check(lib.sai_bed_encode(eng.ctx, ptr(dos), n_rows, n_slots, None, 2, ptr(out), ptr(status), st))

    def packed():
        _ffi.check(lib.sai_geno_encode(eng.ctx, ptr(dos), n_rows, n_slots, None, 2, ptr(out), ptr(status), st))

    def transposed():
        for k0, k1 in groups:  # each group at the front of the buffer, as the converter's two buffers take them
            _ffi.check(lib.sai_geno_encode_transposed(eng.ctx, ptr(dos), n_rows, n_slots, None, 2, k0, k1 - k0, ptr(out), ptr(status), st))

    steps = {"sai_bed_encode": bed, "sai_geno_encode": packed, "sai_geno_encode_transposed": transposed}
    times, behind = {name: [] for name in steps}, {name: [] for name in steps}
    names, last = list(steps), None
    for rep in range(repeats + 1):  # the first round is the warm-up
        # The order is reversed every other round: the block is larger than the last-level cache, and what a kernel
        # finds there is what its predecessor left -- no kernel always runs behind the same one.
        for name in names[::-1] if rep % 2 else names:
            step = steps[name]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            step()
            b.record(stream)
            b.synchronize()
            if rep:
                times[name].append(a.elapsed_time(b))
                behind[name].append(last)
            last = name
    assert not bool(status.any()), "the seeded block holds a call that does not fit"
    return times, behind, groups


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=6, help="kernel rounds after the warm-up")
    ap.add_argument("--convert-repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20263)
    ap.add_argument("--dir", default=None, help="where the input and the filesets are written (kept when given; default: a temporary directory)")
    args = ap.parse_args()

    import tempfile

    import torch

    import __graft_entry__ as entry

    entry.build()
    from bed_export_rate import write_inputs
    from sai_amd.engine import Engine
    from sai_amd.sai import convert
    from sai_amd.utils import device_vcf

    holder = None if args.dir else tempfile.TemporaryDirectory(prefix="geno_export_rate_")
    directory = Path(args.dir or holder.name)
    directory.mkdir(parents=True, exist_ok=True)
    eng = Engine.get(0)
    t0 = time.perf_counter()
    plain, _, names = write_inputs(directory, args.rows, args.samples, args.seed, 1)  # only the plain text is read here
    print(f"== {args.rows} rows x {args.samples} samples: {os.path.getsize(plain)} bytes of plain VCF text, written or found in "
          f"{time.perf_counter() - t0:.1f} s (not part of any figure)")  # fmt: skip
    result = {"rows": args.rows, "samples": args.samples}

    # (a)
    pos, dos, _, _ = device_vcf.load_dosage_device(eng, plain, "1", names, [2] * args.samples)
    torch.cuda.synchronize()
    assert len(pos) == args.rows
    times, behind, groups = kernel_figures(eng, dos, args.repeats)
    block_bytes = args.rows * args.samples
    del dos
    print(f"(a) kernels over the block of {block_bytes} bytes, device events, {args.repeats} repeats after a warm-up, the order reversed every other round:")
    short = {"sai_bed_encode": "bed", "sai_geno_encode": "packed", "sai_geno_encode_transposed": "transposed"}
    for name, ms in times.items():
        print(f"  {name:28s} {fmt(ms)} = {block_bytes / median(ms) / 1e6:.1f} GB/s of block bytes")
        print(f"  {'':28s} each run behind: " + " ".join(short[b] for b in behind[name]))
    bed_ms, geno_ms = times["sai_bed_encode"], times["sai_geno_encode"]
    inside = min(bed_ms) <= median(geno_ms) <= max(bed_ms)
    print(f"  sai_geno_encode against sai_bed_encode: median {median(geno_ms):.3f} ms against {median(bed_ms):.3f} ms "
          f"({(median(geno_ms) / median(bed_ms) - 1) * 100:+.1f} %); inside the min - max of sai_bed_encode's own repeats: {'yes' if inside else 'NO'}")  # fmt: skip
    print(f"  sai_geno_encode_transposed: {len(groups)} calls of up to {groups[0][1] - groups[0][0]} individuals over all {args.rows} rows, summed")
    result["kernel_ms"] = {k: [round(v, 4) for v in vs] for k, vs in times.items()}

    # (b)
    outputs = {"out-bfile": (dict(out_prefix=None), (".bed", ".bim", ".fam")), "out-eigenstrat packed": (dict(geno_format="packed"), (".geno", ".snp", ".ind")),
               "out-eigenstrat transposed": (dict(geno_format="transposed"), (".geno", ".snp", ".ind"))}  # fmt: skip
    runs = {label: ([], []) for label in outputs}
    for rep in range(args.convert_repeats + 1):  # the first round is the warm-up
        for label, (kw, exts) in outputs.items():
            prefix = str(directory / ("out_" + label.replace(" ", "_")))
            for ext in exts:
                if os.path.exists(prefix + ext):
                    os.remove(prefix + ext)
            kw = dict(out_prefix=prefix) if "out_prefix" in kw else dict(out_eigenstrat=prefix, **kw)
            torch.cuda.synchronize()
            t = time.perf_counter()
            summary = convert(plain, "1", **kw)
            dt = (time.perf_counter() - t) * 1e3
            if rep:
                runs[label][0].append(dt), runs[label][1].append(summary["ms"])
    phases = ("read", "site_scan", "encode", "d2h", "write")
    for label, (totals, summaries) in runs.items():
        print(f"(b) convert --{label}, end to end, ms: {fmt(totals)}")
        for phase in phases:
            print(f"      {phase:10s} {fmt([s[phase] for s in summaries])}")
        bound = max(phases, key=lambda ph: median([s[ph] for s in summaries]))
        print(f"      the phase that bounds it: {bound} (read and site_scan run side by side; encode, d2h and write are pipelined behind them)")
        result[label] = {"convert_ms": totals, "phases_ms": summaries, "bounded_by": bound}
    print(json.dumps(result))
    if holder is not None:
        holder.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
