#!/usr/bin/env python3
"""Rate of the PLINK 1 fileset route, phase by phase, next to the plain-text VCF route on the same box.

Writes, from a seed, a fileset of --rows x --samples genotypes on chromosome 1 (random bytes are valid
.bed rows; writing is not timed) and a plain-text VCF of its first --vcf-rows rows, then

  * reads chromosome 1 with ``plink.load_dosage_device`` --repeats times after one warm-up, overlapped as
    `score` reads it (host clock around a device synchronise);
  * reads it once more with every phase synchronised on its own: index, file read, H2D, decode, and the
    re-tiling of the block into three populations (``Engine.tile_columns``);
  * reads the VCF with ``device_vcf.load_dosage_device`` (the route a user has without a fileset) for a
    genotypes-per-second figure from the same call.

Ceilings to read the figures against: the H2D copy crosses PCIe Gen5 x16 (63 GB/s by specification); the
decode kernel writes 4 bytes of HBM per .bed byte.  ``--trace-summary DIR --staged-bytes N`` reads the CSVs a
``rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -- python tools/plink_rate.py ...``
run left behind (N: that run's "staged" line) and prints the kernel's and the copies' own rates.
"""

from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

PCIE_GBS = 63.0


def write_inputs(directory: Path, rows: int, samples: int, vcf_rows: int, seed: int):
    rng = np.random.default_rng(seed)
    prefix = directory / f"rate_{rows}x{samples}_{seed}"
    row_bytes = (samples + 3) // 4
    names = [f"s{i}" for i in range(samples)]
    vcf = directory / f"rate_{vcf_rows}x{samples}_{seed}.vcf"
    if all(Path(f"{prefix}{e}").exists() for e in (".bed", ".bim", ".fam")) and (vcf_rows == 0 or vcf.exists()):
        return str(prefix), str(vcf), names
    positions = np.cumsum(rng.integers(1, 200, size=rows))
    with open(f"{prefix}.fam", "w") as f:
        f.writelines(f"f{i} {n} 0 0 0 -9\n" for i, n in enumerate(names))
    with open(f"{prefix}.bim", "w") as f:
        for lo in range(0, rows, 1 << 18):
            f.write("".join(f"1\tv{k}\t0\t{positions[k]}\tA\tC\n" for k in range(lo, min(rows, lo + (1 << 18)))))
    head = None
    with open(f"{prefix}.bed", "wb") as f:
        f.write(b"\x6c\x1b\x01")
        for lo in range(0, rows, 1 << 17):
            n = min(rows, lo + (1 << 17)) - lo
            block = rng.bytes(n * row_bytes)
            if head is None:
                head = np.frombuffer(block, dtype=np.uint8).reshape(n, row_bytes)[:vcf_rows].copy()
            f.write(block)
    if vcf_rows:
        if vcf_rows > len(head):
            raise SystemExit("--vcf-rows must not exceed 131072 or --rows")
        text = np.array([b"1|1\t", b".|.\t", b"0|1\t", b"0|0\t"], dtype="S4")  # by PLINK code: A1 = ALT
        shifts = np.array([0, 2, 4, 6], dtype=np.uint8)
        with open(vcf, "wb") as f:
            f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names).encode() + b"\n")
            for k in range(vcf_rows):
                codes = ((head[k][:, None] >> shifts) & 3).reshape(-1)[:samples]
                f.write(f"1\t{positions[k]}\tv{k}\tC\tA\t.\tPASS\t.\tGT\t".encode() + text[codes].tobytes()[:-1] + b"\n")
    return str(prefix), str(vcf), names


def trace_summary(directory: str, staged_bytes: int) -> int:
    """Rates from the profiler's own clocks: .bed bytes per second of ``bed_decode_kernel`` and of the H2D
    copies of the staged rows.  The copy trace carries no byte counts, so the rows' copies are told from
    the per-batch index arrays (a few kB, microseconds) by their duration, and the bytes are what the
    profiled run says it staged (``--staged-bytes``: its "staged" line)."""

    def rows_of(pattern):
        out = []
        for path in glob.glob(os.path.join(directory, "**", pattern), recursive=True):
            with open(path, newline="") as f:
                out += list(csv.DictReader(f))
        return out

    def ns(r):
        return int(r["End_Timestamp"]) - int(r["Start_Timestamp"])

    kernels = [r for r in rows_of("*kernel_trace.csv") if "bed_decode" in r.get("Kernel_Name", "")]
    copies = [r for r in rows_of("*memory_copy_trace.csv") if "HOST_TO_DEVICE" in r.get("Direction", "").upper()]
    if not kernels or not copies:
        print(f"trace summary: no bed_decode kernel or H2D copy found under {directory}")
        return 1
    k_ns = sum(ns(r) for r in kernels)
    big = [r for r in copies if ns(r) >= 100_000]  # 100 us: 4 MB at the link's rate; the index arrays take ~10 us
    c_ns, small_ns = sum(ns(r) for r in big), sum(ns(r) for r in copies if ns(r) < 100_000)
    print(f"trace summary: {len(kernels)} bed_decode_kernel launches, {k_ns / 1e6:.3f} ms in all; {len(big)} H2D copies of .bed rows, "
          f"{c_ns / 1e6:.3f} ms in all (+ {len(copies) - len(big)} small copies of index arrays, {small_ns / 1e6:.3f} ms)")  # fmt: skip
    if staged_bytes <= 0:
        return 0
    print(f"trace summary: H2D of {staged_bytes} .bed bytes: {staged_bytes / c_ns:.1f} GB/s (ceiling: PCIe Gen5 x16, {PCIE_GBS:.0f} GB/s by specification)")
    print(f"trace summary: bed_decode_kernel over the same bytes: {staged_bytes / k_ns:.1f} GB/s of .bed = {4 * staged_bytes / k_ns:.1f} GB/s of "
          "HBM writes (ceiling: the HBM write rate, 4 bytes per .bed byte)")  # fmt: skip
    print(f"trace summary: decode rate / H2D rate = {c_ns / k_ns:.2f} (the kernel must not be the bound: >= 1)")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--samples", type=int, default=2002)
    ap.add_argument("--vcf-rows", type=int, default=100_000, help="rows of the plain-text VCF (0: skip the VCF route)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261)
    ap.add_argument("--dir", default=None, help="where the inputs are written (kept and reused when given; default: a temporary directory)")
    ap.add_argument("--trace-summary", default=None, metavar="DIR")
    ap.add_argument("--staged-bytes", type=int, default=0, help="with --trace-summary: the .bed bytes the profiled run staged")
    args = ap.parse_args()
    if args.trace_summary:
        return trace_summary(args.trace_summary, args.staged_bytes)

    import tempfile

    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine
    from sai_amd.utils import device_vcf, plink

    holder = None if args.dir else tempfile.TemporaryDirectory(prefix="plink_rate_")
    directory = Path(args.dir or holder.name)
    directory.mkdir(parents=True, exist_ok=True)
    t0 = time.perf_counter()
    prefix, vcf, names = write_inputs(directory, args.rows, args.samples, min(args.vcf_rows, args.rows), args.seed)
    bed_bytes = os.path.getsize(prefix + ".bed")
    print(f"inputs: {prefix}.bed {bed_bytes} bytes ({args.rows} rows x {args.samples} samples), written or found in "
          f"{time.perf_counter() - t0:.1f} s (not part of any figure)")  # fmt: skip
    eng = Engine.get(0)
    ploidies = [2] * len(names)
    genotypes = args.rows * args.samples

    reads = [0]

    def read(trace=None):
        reads[0] += 1
        torch.cuda.synchronize()
        t = time.perf_counter()
        pos, dos, n_matched, _ = plink.load_dosage_device(eng, prefix, "1", names, ploidies, trace=trace)
        torch.cuda.synchronize()
        return time.perf_counter() - t, pos, dos

    read()  # warm-up: page-locks the staging buffers, loads the code object
    whole = []
    for _ in range(args.repeats):
        dt, pos, dos = read()
        assert len(pos) == args.rows and tuple(dos.shape) == (args.rows, args.samples)
        whole.append(dt)
        del dos
    best, median = min(whole), sorted(whole)[len(whole) // 2]
    print("fileset read, overlapped (as `score` reads it), ms per read: " + " ".join(f"{1e3 * t:.1f}" for t in whole))
    print(f"  median {1e3 * median:.1f} ms = {bed_bytes / median / 1e9:.2f} GB/s of .bed, {genotypes / median / 1e9:.2f} G genotypes/s "
          f"(best {1e3 * best:.1f} ms)")  # fmt: skip
    trace = {"serial": True}
    dt, pos, dos = read(trace)
    torch.cuda.synchronize()
    t = time.perf_counter()
    third = args.samples // 2
    tiled = [eng.tile_columns(dos, list(range(lo, hi))) for lo, hi in ((0, third), (third, 2 * third), (2 * third, args.samples))]
    torch.cuda.synchronize()
    trace["re-tile"] = time.perf_counter() - t
    n_bytes = trace["bed_bytes"]
    print(f"fileset read, every phase synchronised on its own ({1e3 * dt:.1f} ms in all), ms per phase:")
    notes = {"index": "host: .fam + .bim, one pass over an mmap",
             "file_read": f"pread into pinned memory, {n_bytes / trace['file_read'] / 1e9:.1f} GB/s of .bed",
             "h2d": f"{n_bytes / trace['h2d'] / 1e9:.1f} GB/s of .bed; ceiling PCIe Gen5 x16, {PCIE_GBS:.0f} GB/s by specification",
             "decode": f"{n_bytes / trace['decode'] / 1e9:.1f} GB/s of .bed = {4 * n_bytes / trace['decode'] / 1e9:.1f} GB/s of HBM writes "
                       "(includes a launch and a synchronise per batch)",
             "re-tile": f"three populations, {2 * genotypes / trace['re-tile'] / 1e9:.1f} GB/s of HBM read + write"}  # fmt: skip
    for name in ("index", "file_read", "h2d", "decode", "re-tile"):
        print(f"  {name:9s} {1e3 * trace[name]:9.1f}   {notes[name]}")
    del dos, tiled
    result = {"rows": args.rows, "samples": args.samples, "bed_bytes": bed_bytes, "fileset_ms": [round(1e3 * t, 2) for t in whole],
              "fileset_genotypes_per_s": genotypes / median, "fileset_bed_gb_per_s": bed_bytes / median / 1e9,
              "phases_ms": {k: round(1e3 * v, 2) for k, v in trace.items() if k not in ("serial", "bed_bytes")}}  # fmt: skip
    if args.vcf_rows:
        n_vcf = min(args.vcf_rows, args.rows)
        text_bytes = os.path.getsize(vcf)

        def read_vcf():
            torch.cuda.synchronize()
            t = time.perf_counter()
            pos, dos, _, _ = device_vcf.load_dosage_device(eng, vcf, "1", names, ploidies)
            torch.cuda.synchronize()
            assert len(pos) == n_vcf
            return time.perf_counter() - t

        read_vcf()
        runs = [read_vcf() for _ in range(max(3, min(args.repeats, 5)))]
        v_med = sorted(runs)[len(runs) // 2]
        print(f"plain-text VCF of the first {n_vcf} rows ({text_bytes} bytes), GPU tokenizer route, ms per read: "
              + " ".join(f"{1e3 * t:.1f}" for t in runs))  # fmt: skip
        print(f"  median {1e3 * v_med:.1f} ms = {text_bytes / v_med / 1e9:.2f} GB/s of text, {n_vcf * args.samples / v_med / 1e9:.3f} G genotypes/s")
        ratio = (genotypes / median) / (n_vcf * args.samples / v_med)
        print(f"fileset / VCF, genotypes per second: {ratio:.1f}x (the byte ratio, 16, is the ceiling)")
        result.update(vcf_rows=n_vcf, vcf_text_bytes=text_bytes, vcf_ms=[round(1e3 * t, 2) for t in runs],
                      vcf_genotypes_per_s=n_vcf * args.samples / v_med, fileset_over_vcf=ratio)  # fmt: skip
    print(f"staged: {reads[0]} reads x {bed_bytes - 3} bytes = {reads[0] * (bed_bytes - 3)} .bed bytes over PCIe (warm-up and the serial read included)")
    print(json.dumps(result))
    if holder is not None:
        holder.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
