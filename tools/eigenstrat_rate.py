#!/usr/bin/env python3
"""Rate of the EIGENSOFT fileset routes, phase by phase, next to the PLINK route on the same genotype matrix in
the same call.

Writes, from a seed, ONE matrix of --rows x --samples genotypes on chromosome 1 three ways (writing is not timed):
the ``.bed`` of ``plink_rate.py``, the packed ``.geno`` that holds the same calls (a byte-for-byte recode: the same
bytes cross PCIe), and the transposed packed ``.geno`` (turned on the GPU with torch, chunk by chunk).  Then, per
route -- ``plink.load_dosage_device`` as the yardstick, ``eigenstrat.load_dosage_device`` on the two ``.geno`` --

  * reads chromosome 1 --repeats times after one warm-up, overlapped as `score` reads it (host clock around a
    device synchronise), and checks once that the three routes give the same dosage block;
  * reads it once more with every phase synchronised on its own: index, file read, H2D, decode.

``--trace-summary DIR --staged-bytes N`` reads the CSVs a ``rocprofv3 --kernel-trace --memory-copy-trace --stats
--output-format csv -d DIR -- python tools/eigenstrat_rate.py ...`` run left behind (N: that run's "staged" line,
the bytes of ONE route) and prints the three kernels' rates and the H2D copies' rate from the profiler's clocks.
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
for entry_dir in (ROOT, ROOT / "tools"):
    if str(entry_dir) not in sys.path:
        sys.path.insert(0, str(entry_dir))

from plink_rate import PCIE_GBS, write_inputs  # noqa: E402

KERNELS = {"bed": "bed_decode_kernel", "packed": "geno_decode_kernel", "transposed": "geno_transpose_kernel"}
G_OF_PLINK = np.array([0, 3, 1, 2], dtype=np.uint8)  # PLINK code (A1 A1, missing, het, A2 A2) -> copies of A2, 3 = missing


def write_geno(bed_prefix: str, rows: int, samples: int):
    """PREFIX_packed / PREFIX_transposed (.geno, .snp, .ind) of the fileset ``bed_prefix``: A2 is the first allele."""
    import torch

    row_bytes = (samples + 3) // 4
    assert row_bytes >= 48 and rows % 4 == 0, "the tool's shapes: at least 189 samples, rows a multiple of 4"
    packed, turned = bed_prefix + "_packed", bed_prefix + "_transposed"
    if all(os.path.exists(p + e) for p in (packed, turned) for e in (".geno", ".snp", ".ind")):
        return packed, turned
    with open(bed_prefix + ".bim") as f, open(packed + ".snp", "w") as out:
        for line in f:
            chrom, name, gpos, pos, a1, a2 = line.split()
            out.write(f"{name:>20} {chrom:>3} {0.0:>12.6f} {pos:>15} {a2} {a1}\n")
    with open(bed_prefix + ".fam") as f, open(packed + ".ind", "w") as out:
        out.writelines(f"{line.split()[1]:>20} U {'Pop':>10}\n" for line in f)
    for ext in (".snp", ".ind"):
        with open(packed + ext, "rb") as src, open(turned + ext, "wb") as dst:
            dst.write(src.read())
    # a .bed byte holds the codes of four samples, the first in bits 1:0; a .geno byte the first in bits 7:6
    b = np.arange(256, dtype=np.uint16)
    recode = sum(G_OF_PLINK[(b >> (2 * k)) & 3].astype(np.uint16) << (6 - 2 * k) for k in range(4)).astype(np.uint8)
    rlen_t = max(48, rows // 4)
    with open(turned + ".geno", "wb") as f:
        f.write(("TGENO %7d %7d 0 0" % (samples, rows)).encode().ljust(rlen_t, b"\0"))
        f.truncate(rlen_t * (1 + samples))
    out_t = np.memmap(turned + ".geno", dtype=np.uint8, mode="r+", offset=rlen_t, shape=(samples, rlen_t))
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    shifts = torch.tensor([0, 2, 4, 6], dtype=torch.int32, device=dev)
    g_of = torch.from_numpy(G_OF_PLINK).to(dev)
    chunk = 1 << 17
    with open(bed_prefix + ".bed", "rb") as src, open(packed + ".geno", "wb") as dst:
        src.seek(3)
        dst.write(("GENO %7d %7d 0 0" % (samples, rows)).encode().ljust(row_bytes, b"\0"))
        for lo in range(0, rows, chunk):
            n = min(rows, lo + chunk) - lo
            block = np.frombuffer(src.read(n * row_bytes), dtype=np.uint8).reshape(n, row_bytes)
            dst.write(recode[block].tobytes())
            codes = (torch.from_numpy(block.copy()).to(dev).int()[:, :, None] >> shifts) & 3  # [n][row_bytes][4]
            g = g_of[codes.reshape(n, -1)[:, :samples].long()].T.contiguous().reshape(samples, n // 4, 4).int()  # [sample][byte][code]
            turned_bytes = (g[:, :, 0] << 6) | (g[:, :, 1] << 4) | (g[:, :, 2] << 2) | g[:, :, 3]
            out_t[:, lo // 4 : (lo + n) // 4] = turned_bytes.to(torch.uint8).cpu().numpy()
    out_t.flush()
    del out_t
    return packed, turned


def trace_summary(directory: str, staged_bytes: int) -> int:
    """Rates from the profiler's own clocks: file bytes per second of each decode kernel and of the H2D copies of the
    staged bytes (all three routes together: the copy trace does not say whose a copy is)."""
    import csv
    import glob

    def rows_of(pattern):
        out = []
        for path in glob.glob(os.path.join(directory, "**", pattern), recursive=True):
            with open(path, newline="") as f:
                out += list(csv.DictReader(f))
        return out

    def ns(r):
        return int(r["End_Timestamp"]) - int(r["Start_Timestamp"])

    kernels = rows_of("*kernel_trace.csv")
    copies = [r for r in rows_of("*memory_copy_trace.csv") if "HOST_TO_DEVICE" in r.get("Direction", "").upper()]
    big = [r for r in copies if ns(r) >= 100_000]  # 100 us: 4 MB at the link's rate; the index arrays take ~10 us
    if not kernels or not big:
        print(f"trace summary: no kernel or H2D copy found under {directory}")
        return 1
    c_ns = sum(ns(r) for r in big)
    print(f"trace summary: {len(big)} H2D copies of staged bytes, {c_ns / 1e6:.3f} ms in all (+ {len(copies) - len(big)} small copies of index arrays)")
    h2d = 3 * staged_bytes / c_ns if staged_bytes > 0 else 0.0
    if staged_bytes > 0:
        print(f"trace summary: H2D of 3 x {staged_bytes} bytes: {h2d:.1f} GB/s (ceiling: PCIe Gen5 x16, {PCIE_GBS:.0f} GB/s by specification)")
    for route, name in KERNELS.items():
        mine = [r for r in kernels if name in r.get("Kernel_Name", "")]
        k_ns = sum(ns(r) for r in mine)
        if not mine:
            print(f"trace summary: {route}: no {name} launch found")
            continue
        line = f"trace summary: {route}: {len(mine)} {name} launches, {k_ns / 1e6:.3f} ms in all"
        if staged_bytes > 0:
            line += (f" = {staged_bytes / k_ns:.1f} GB/s of file bytes = {4 * staged_bytes / k_ns:.1f} GB/s of HBM writes; "
                     f"kernel rate / H2D rate = {staged_bytes / k_ns / h2d:.2f}")  # fmt: skip
        print(line)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--samples", type=int, default=2002)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261)
    ap.add_argument("--dir", default=None, help="where the inputs are written (kept and reused when given; default: a temporary directory)")
    ap.add_argument("--trace-summary", default=None, metavar="DIR")
    ap.add_argument("--staged-bytes", type=int, default=0, help="with --trace-summary: the file bytes ONE route of the profiled run staged")
    args = ap.parse_args()
    if args.trace_summary:
        return trace_summary(args.trace_summary, args.staged_bytes)

    import tempfile

    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine
    from sai_amd.utils import eigenstrat, plink

    holder = None if args.dir else tempfile.TemporaryDirectory(prefix="eigenstrat_rate_")
    directory = Path(args.dir or holder.name)
    directory.mkdir(parents=True, exist_ok=True)
    t0 = time.perf_counter()
    bed, _, names = write_inputs(directory, args.rows, args.samples, 0, args.seed)
    packed, turned = write_geno(bed, args.rows, args.samples)
    data_bytes = args.rows * ((args.samples + 3) // 4)
    print(f"inputs: {args.rows} rows x {args.samples} samples as {bed}.bed ({os.path.getsize(bed + '.bed')} bytes), _packed.geno "
          f"({os.path.getsize(packed + '.geno')}) and _transposed.geno ({os.path.getsize(turned + '.geno')}), written or found in "
          f"{time.perf_counter() - t0:.1f} s (not part of any figure)")  # fmt: skip
    eng = Engine.get(0)
    ploidies = [2] * len(names)
    genotypes = args.rows * args.samples
    routes = {"bed": (plink, bed, "bed_bytes"), "packed": (eigenstrat, packed, "geno_bytes"), "transposed": (eigenstrat, turned, "geno_bytes")}
    result = {"rows": args.rows, "samples": args.samples, "data_bytes": data_bytes, "routes": {}}
    reads = 0
    reference = None
    for route, (reader, prefix, counter) in routes.items():

        def read(trace=None):
            torch.cuda.synchronize()
            t = time.perf_counter()
            pos, dos, _, _ = reader.load_dosage_device(eng, prefix, "1", names, ploidies, trace=trace)
            torch.cuda.synchronize()
            return time.perf_counter() - t, pos, dos

        _, pos, dos = read()  # warm-up: page-locks the staging buffers, loads the code object
        assert len(pos) == args.rows and tuple(dos.shape) == (args.rows, args.samples)
        if reference is None:
            reference = dos  # the .bed route's block: the two .geno routes must give the same bytes
        else:
            assert torch.equal(dos, reference), f"{route}: the dosage block differs from the .bed route's"
        del dos
        whole = [read()[0] for _ in range(args.repeats)]
        median, spread = sorted(whole)[len(whole) // 2], max(whole) - min(whole)
        print(f"{route}: read overlapped (as `score` reads it), ms per read: " + " ".join(f"{1e3 * t:.1f}" for t in whole))
        print(f"  median {1e3 * median:.1f} ms (spread {1e3 * spread:.1f}) = {data_bytes / median / 1e9:.2f} GB/s of file bytes, "
              f"{genotypes / median / 1e9:.2f} G genotypes/s")  # fmt: skip
        trace = {"serial": True}
        dt = read(trace)[0]
        n_bytes = trace[counter]
        print(f"{route}: every phase synchronised on its own ({1e3 * dt:.1f} ms in all), ms per phase:")
        for name in ("index", "file_read", "h2d", "decode"):
            rate = "" if name == "index" else f"{n_bytes / trace[name] / 1e9:.1f} GB/s of file bytes"
            print(f"  {name:9s} {1e3 * trace[name]:9.1f}   {rate}")
        slowest = max(("file_read", "h2d", "decode"), key=lambda k: trace[k])
        print(f"  slowest phase: {slowest}; decode rate / H2D rate = {trace['h2d'] / trace['decode']:.2f}")
        result["routes"][route] = {"ms": [round(1e3 * t, 2) for t in whole], "median_ms": round(1e3 * median, 2), "spread_ms": round(1e3 * spread, 2),
                                   "phases_ms": {k: round(1e3 * trace[k], 2) for k in ("index", "file_read", "h2d", "decode")}}  # fmt: skip
        reads = args.repeats + 2
        reader.release_buffers(eng)
    del reference
    print(f"staged: {reads} reads x {data_bytes} bytes = {reads * data_bytes} file bytes over PCIe per route (warm-up and the serial read included)")
    print(json.dumps(result))
    if holder is not None:
        holder.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
