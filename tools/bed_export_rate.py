#!/usr/bin/env python3
"""Rate of `sai convert`, the kernel behind it and the fileset it writes, in one call.

Writes, from a seed, a matrix of --rows records x --samples phased diploid calls on chromosome 1 as plain VCF text and as
bgzip VCF text (``tools/bcf_rate.py``'s ``BgzfWriter``: the tests' ``bcf_builder.bgzf_members``; writing is not timed),
once per width of --samples.  Then, per width, with the files in the page cache:

  (a) the kernel: ``sai_bed_encode`` over the whole block in one call, timed with device events after a warm-up,
      alternating with its two yardsticks -- the D2H copy of its own output into pinned memory, which it must hide
      under, and a device-to-device copy of its input, for information.  The condition: the kernel is not slower
      than that D2H copy.  The kernel is timed twice: with one ploidy for every slot, and with the same ploidies
      handed over slot by slot (``per_slot``: what a conversion with ``--haploid`` launches);
  (b) ``convert`` end to end against ``load_dosage_device`` alone on the same file, alternating, for the plain and the
      bgzip file: every phase of the summary, the phase that bounds it, and the site scanner alone on both files;
  (c) the files' sizes, and ``score`` from the fileset (both layouts) against ``score`` from the plain VCF.

Every figure is a median with its spread (max - min) over --repeats.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for entry_dir in (ROOT, ROOT / "tests", ROOT / "tools"):
    if str(entry_dir) not in sys.path:
        sys.path.insert(0, str(entry_dir))

CHUNK_ROWS = 4096


def write_inputs(directory: Path, rows: int, samples: int, seed: int, level: int):
    """(plain path, bgzip path, names): the same seeded calls, found again when they exist."""
    from bcf_rate import BgzfWriter

    plain, bgz = directory / f"export_{rows}x{samples}_{seed}.vcf", directory / f"export_{rows}x{samples}_{seed}.vcf.gz"
    names = [f"s{k}" for k in range(samples)]
    if plain.exists() and bgz.exists():
        return str(plain), str(bgz), names
    rng = np.random.default_rng(seed)
    header = "##fileformat=VCFv4.2\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    text_of = np.array([b"0|0\t", b"0|1\t", b"1|0\t", b"1|1\t"], dtype="S4")
    out_bgz = BgzfWriter(bgz, level)
    with open(plain, "wb") as out_plain:
        out_plain.write(header.encode())
        out_bgz.write(header.encode())
        pos = 0
        for lo in range(0, rows, CHUNK_ROWS):
            n = min(rows, lo + CHUNK_ROWS) - lo
            p = rng.random((n, 1)) ** 3
            codes = (rng.random((n, samples)) < p).astype(np.uint8) * 2 + (rng.random((n, samples)) < p).astype(np.uint8)
            steps = rng.integers(1, 50, n)
            text = []
            for k in range(n):
                pos += int(steps[k])
                text.append(f"1\t{pos}\tv{lo + k}\tG\tT\t.\tPASS\t.\tGT\t".encode() + text_of[codes[k]].tobytes()[:-1] + b"\n")
            chunk = b"".join(text)
            out_plain.write(chunk)
            out_bgz.write(chunk)
    out_bgz.close()
    return str(plain), str(bgz), names


def stats(values):
    values = sorted(values)
    return values[len(values) // 2], values[-1] - values[0]


def fmt(values, unit="ms"):
    med, spread = stats(values)
    return f"median {med:.3f} {unit} (spread {spread:.3f}; " + " ".join(f"{v:.3f}" for v in values) + ")"


def kernel_figures(eng, dos, repeats):
    """(a): {kernel, d2h, d2d} -> ms per repeat, alternating."""
    import ctypes as C

    import torch

    from sai_amd import _ffi
    from sai_amd.utils import bed_writer

    lib = bed_writer.load()
    n_rows, n_slots = dos.shape
    row_bytes = (n_slots + 3) // 4
    out = torch.empty((n_rows * row_bytes,), dtype=torch.uint8, device=eng.device)
    status = torch.empty((n_rows,), dtype=torch.int32, device=eng.device)
    twin = torch.empty_like(dos)
    pinned = torch.empty((n_rows * row_bytes,), dtype=torch.uint8).pin_memory()
    stream = torch.cuda.current_stream(eng.device)

    per_slot = torch.full((n_slots,), 2, dtype=torch.int32, device=eng.device)  # the same ploidies, said slot by slot

    def kernel(ploidies=None):
        _ffi.check(lib.sai_bed_encode(eng.ctx, C.c_void_p(dos.data_ptr()), n_rows, n_slots, None if ploidies is None else C.c_void_p(ploidies.data_ptr()),
                                      2 if ploidies is None else 0, C.c_void_p(out.data_ptr()), C.c_void_p(status.data_ptr()),
                                      C.c_void_p(stream.cuda_stream)))  # fmt: skip

    steps = {"kernel": kernel, "per_slot": lambda: kernel(per_slot), "d2h": lambda: pinned.copy_(out, non_blocking=True), "d2d": lambda: twin.copy_(dos)}
    times = {name: [] for name in steps}
    for rep in range(repeats + 1):  # the first round is the warm-up
        for name, step in steps.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            step()
            b.record(stream)
            b.synchronize()
            if rep:
                times[name].append(a.elapsed_time(b))
    assert not bool(status.any()), "the seeded block holds a call that does not fit"
    return times, n_rows * row_bytes, n_rows * n_slots


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--samples", default="2000,2002", help="widths, comma-separated")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20263)
    ap.add_argument("--bgzf-level", type=int, default=1, help="zlib level of the bgzip input (its size depends on it, the inflated text does not)")
    ap.add_argument("--dir", default=None, help="where the inputs and the filesets are written (kept when given; default: a temporary directory)")
    ap.add_argument("--no-score", action="store_true", help="leave (c)'s `score` runs out")
    args = ap.parse_args()

    import tempfile

    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine
    from sai_amd.sai import convert, score
    from sai_amd.utils import bed_writer, device_vcf

    holder = None if args.dir else tempfile.TemporaryDirectory(prefix="bed_export_rate_")
    directory = Path(args.dir or holder.name)
    directory.mkdir(parents=True, exist_ok=True)
    eng = Engine.get(0)
    result = {"rows": args.rows, "widths": {}}
    for samples in (int(s) for s in args.samples.split(",")):
        t0 = time.perf_counter()
        plain, bgz, names = write_inputs(directory, args.rows, samples, args.seed, args.bgzf_level)
        print(f"== {args.rows} rows x {samples} samples: {plain} ({os.path.getsize(plain)} bytes) and {bgz} ({os.path.getsize(bgz)} bytes, zlib level "
              f"{args.bgzf_level}), written or found in {time.perf_counter() - t0:.1f} s (not part of any figure)")  # fmt: skip
        ploidies = [2] * samples
        here = result["widths"][samples] = {}

        def read(path):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = device_vcf.load_dosage_device(eng, path, "1", names, ploidies)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3, got

        # (a)
        _, (pos, dos, _, _) = read(plain)
        assert len(pos) == args.rows
        times, out_bytes, in_bytes = kernel_figures(eng, dos, args.repeats)
        del dos
        print(f"(a) sai_bed_encode, {in_bytes} bytes in, {out_bytes} bytes out, one call, device events, alternating, ms:")
        for name, moved in (("kernel", in_bytes + out_bytes), ("per_slot", in_bytes + out_bytes), ("d2h", out_bytes), ("d2d", 2 * in_bytes)):
            med, _ = stats(times[name])
            print(f"  {name:8s} {fmt(times[name])} = {moved / med / 1e6:.1f} GB/s of the bytes it moves")
        k_med, h_med = max(stats(times["kernel"])[0], stats(times["per_slot"])[0]), stats(times["d2h"])[0]
        verdict = "holds" if k_med <= h_med else "DOES NOT HOLD"
        print(f"  condition (kernel, in its slower form, not slower than the D2H copy of its output): {verdict}: {k_med:.3f} ms against {h_med:.3f} ms, "
              f"D2H / kernel = {h_med / k_med:.2f}")  # fmt: skip
        here["kernel_ms"] = {k: [round(v, 4) for v in vs] for k, vs in times.items()}
        here["condition_holds"] = bool(k_med <= h_med)

        # (b)
        for label, path in (("plain", plain), ("bgzip", bgz)):
            prefix = str(directory / f"out_{samples}_{label}")
            reads, converts, summaries = [], [], []
            for rep in range(args.repeats + 1):  # the first round is the warm-up
                for ext in (".bed", ".bim", ".fam"):
                    if os.path.exists(prefix + ext):
                        os.remove(prefix + ext)
                ms, got = read(path)
                del got
                torch.cuda.synchronize()
                t = time.perf_counter()
                summary = convert(path, "1", prefix)
                dt = (time.perf_counter() - t) * 1e3
                if rep:
                    reads.append(ms), converts.append(dt), summaries.append(summary["ms"])
            print(f"(b) {label}: load_dosage_device alone, ms: {fmt(reads)}")
            print(f"    {label}: convert end to end, ms:        {fmt(converts)}")
            phases = ("read", "site_scan", "encode", "d2h", "write")
            for phase in phases:
                print(f"      {phase:10s} {fmt([s[phase] for s in summaries])}")
            bound = max(phases, key=lambda ph: stats([s[ph] for s in summaries])[0])
            print(f"      the phase that bounds it: {bound} (read and site_scan run side by side; encode, d2h and write are pipelined behind them)")
            scans = []
            for rep in range(args.repeats + 1):
                t = time.perf_counter()
                bed_writer.SiteColumns(path, "1").close()
                if rep:
                    scans.append((time.perf_counter() - t) * 1e3)
            text_bytes = os.path.getsize(plain)
            print(f"    {label}: site scanner alone, ms: {fmt(scans)} = {text_bytes / stats(scans)[0] / 1e6:.2f} GB/s of text"
                  + (" (one thread through zlib)" if label == "bgzip" else " (mapped, threads split at line starts)"))  # fmt: skip
            here[label] = {"read_ms": reads, "convert_ms": converts, "phases_ms": summaries, "bounded_by": bound, "site_scan_alone_ms": scans}

        # (c)
        prefix = str(directory / f"out_{samples}_plain")
        sizes = {ext: os.path.getsize(prefix + ext) for ext in (".bed", ".bim", ".fam")}
        print(f"(c) files: .bed {sizes['.bed']} bytes, .bim {sizes['.bim']}, .fam {sizes['.fam']}; the plain VCF {os.path.getsize(plain)} "
              f"({os.path.getsize(plain) / sizes['.bed']:.1f} times the .bed), the bgzip VCF {os.path.getsize(bgz)}")  # fmt: skip
        here["sizes"] = sizes
        if not args.no_score:
            half = (samples - 2) // 2
            groups = (("ref", "R", names[:half]), ("tgt", "T", names[half : 2 * half]), ("src", "S", names[2 * half : 2 * half + 2]))
            for group, pop, members in groups:
                (directory / f"{group}_{samples}.list").write_text("".join(f"{pop}\t{s}\n" for s in members))
            uq = "    ref:\n      R: 0.3\n    tgt:\n      T: {x}\n    src:\n      S: \"=1\"\n"
            cfg = directory / f"cfg_{samples}.yaml"
            cfg.write_text("statistics:\n  U:\n" + uq.format(x=0.2) + "  Q:\n" + uq.format(x=0.95) + "ploidies:\n  ref:\n    R: 2\n  tgt:\n    T: 2\n  src:\n    S: 2\n"
                           "populations:\n" + "".join(f"  {g}: \"{directory}/{g}_{samples}.list\"\n" for g, _, _ in groups))  # fmt: skip
            outputs = {}
            for label, source, layout in (("vcf", plain, None), ("bed_int8", prefix + ".bed", "int8"), ("bed_packed2", prefix + ".bed", "packed2")):
                runs = []
                for rep in range(min(args.repeats, 3) + 1):
                    out = directory / f"score_{samples}_{label}.tsv"
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    score(vcf_file=source, chr_name="1", win_len=50000, win_step=10000, anc_allele_file=None, output_file=str(out), config=str(cfg),
                          num_workers=1, layout=layout)  # fmt: skip
                    torch.cuda.synchronize()
                    if rep:
                        runs.append((time.perf_counter() - t) * 1e3)
                outputs[label] = out.read_bytes()
                print(f"    score from {label:12s} ms: {fmt(runs)}")
                here[f"score_{label}_ms"] = runs
            same = outputs["vcf"] == outputs["bed_int8"] == outputs["bed_packed2"]
            print(f"    the three score tables are {'byte-identical' if same else 'DIFFERENT'}; score from the VCF / from the .bed = "
                  f"{stats(here['score_vcf_ms'])[0] / stats(here['score_bed_int8_ms'])[0]:.2f} (int8), "
                  f"{stats(here['score_vcf_ms'])[0] / stats(here['score_bed_packed2_ms'])[0]:.2f} (packed2)")  # fmt: skip
        if holder is not None:  # a temporary directory holds one width at a time
            for path in directory.iterdir():
                path.unlink()
    print(json.dumps(result))
    if holder is not None:
        holder.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
