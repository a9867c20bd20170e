#!/usr/bin/env python3
"""Rate of the BCF route, phase by phase, next to the two bgzip-VCF routes on the same calls in the same call.

Writes, from a seed, ONE matrix of --rows x --samples phased diploid calls on chromosome 1 two ways (writing is not
timed): as bgzip VCF text and as BCF, the latter with the tests' writer (tests/bcf_builder.py: its header, its
``encode_record`` and its ``bgzf_members`` at zlib level 6; the GT payload of a record comes from numpy).  Then, in
ONE call,

  * reads chromosome 1 through ``bcf.load_dosage_device`` on its host route (``SAI_AMD_GPU_INFLATE=0``), through
    ``device_vcf.load_dosage_device`` with the host inflating (``SAI_AMD_GPU_INFLATE=0``) and through the same with the
    GPU inflating, and through ``bcf.load_dosage_device`` on its GPU route (``bcf_gpu_walk``: members inflated and
    records found on the GPU) -- each --repeats times after one warm-up, with the files in the page cache, overlapped
    as `score` reads them (host clock around a device synchronise) -- reports the median, and checks that the four
    dosage blocks are equal;
  * reads the BCF once more on its host route with every phase on its own: the producer's file read, inflate, walk
    and copy into staging (``sai_bcf_stream_stats``), and H2D and kernel with the side stream synchronised behind each;
  * reads it on the GPU route with every phase on its own, once per segment size of --seg-bytes;
  * says which phase bounds the host route.

``--trace-summary DIR --staged-bytes N`` reads the CSVs a ``rocprofv3 --kernel-trace --memory-copy-trace --stats
--output-format csv -d DIR -- python tools/bcf_rate.py ...`` run left behind (N: that run's "staged" line) and prints
the kernel's rate against the H2D copies' from the profiler's clocks, as ``tools/plink_rate.py`` does for the `.bed`.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for entry_dir in (ROOT, ROOT / "tests"):
    if str(entry_dir) not in sys.path:
        sys.path.insert(0, str(entry_dir))

KERNEL = "bcf_decode_kernel"
PCIE_GBS = 63.0  # PCIe Gen5 x16 by specification
MEMBER = 65280
CHUNK_ROWS = 4096


class BgzfWriter:
    """Bytes in, BGZF members of MEMBER inflated bytes out (``bcf_builder.bgzf_members``, zlib level 6), the EOF member at the end."""

    def __init__(self, path, level=6):
        import bcf_builder as B

        self.B, self.f, self.level, self.pending = B, open(path, "wb"), level, bytearray()

    def write(self, data: bytes) -> None:
        self.pending += data
        whole = len(self.pending) // MEMBER * MEMBER
        if whole:
            self.f.write(b"".join(self.B.bgzf_members(bytes(self.pending[:whole]), MEMBER, self.level, eof=False)))
            del self.pending[:whole]

    def close(self) -> None:
        self.f.write(b"".join(self.B.bgzf_members(bytes(self.pending), MEMBER, self.level, eof=True)))
        self.f.close()


def write_inputs(directory: Path, rows: int, samples: int, seed: int):
    """(path of the .vcf.gz, path of the .bcf, sample names): the same seeded calls, found again when they exist."""
    import bcf_builder as B

    vcf, bcf = directory / f"rate_{rows}x{samples}_{seed}.vcf.gz", directory / f"rate_{rows}x{samples}_{seed}.bcf"
    names = [f"s{k}" for k in range(samples)]
    if vcf.exists() and bcf.exists():
        return str(vcf), str(bcf), names
    rng = np.random.default_rng(seed)
    header = ["##fileformat=VCFv4.2", "##contig=<ID=1>", '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names)]  # fmt: skip
    htext, contigs, strings, _ = B.build_header(header, ["1"], False, False, False)
    text_of = np.array([b"0|0\t", b"0|1\t", b"1|0\t", b"1|1\t"], dtype="S4")
    # (allele + 1) << 1 | phased: 0|0 = 02 03, 0|1 = 02 05, 1|0 = 04 03, 1|1 = 04 05
    gt_of = np.array([[2, 3], [2, 5], [4, 3], [4, 5]], dtype=np.uint8)
    out_vcf, out_bcf = BgzfWriter(vcf), BgzfWriter(bcf)
    out_vcf.write(("\n".join(header) + "\n").encode())
    out_bcf.write(B.MAGIC + len(htext).to_bytes(4, "little") + htext)
    pos = 0
    for lo in range(0, rows, CHUNK_ROWS):
        n = min(rows, lo + CHUNK_ROWS) - lo
        p = rng.random((n, 1)) ** 3
        codes = (rng.random((n, samples)) < p).astype(np.uint8) * 2 + (rng.random((n, samples)) < p).astype(np.uint8)
        steps = rng.integers(1, 50, n)
        text, records = [], []
        for k in range(n):
            pos += int(steps[k])
            cells = text_of[codes[k]].tobytes()
            text.append(f"1\t{pos}\tv{lo + k}\tG\tT\t.\tPASS\t.\tGT\t".encode() + cells[:-1] + b"\n")
            records.append(B.encode_record({"chrom": contigs["1"], "pos0": pos - 1, "rlen": 1, "n_allele": 2, "n_info": 0, "n_sample": samples,
                                            "id": f"v{lo + k}", "alleles": ["G", "T"], "filter": [0],
                                            "fmt": [{"key": strings["GT"], "type": B.INT8, "L": 2, "payload": gt_of[codes[k]].tobytes()}]}))  # fmt: skip
        out_vcf.write(b"".join(text))
        out_bcf.write(b"".join(records))
    out_vcf.close()
    out_bcf.close()
    return str(vcf), str(bcf), names


def trace_summary(directory: str, staged_bytes: int) -> int:
    """The kernel's rate against the H2D copies' of the staged GT bytes, from the profiler's own clocks."""
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

    mine = [r for r in rows_of("*kernel_trace.csv") if KERNEL in r.get("Kernel_Name", "")]
    big = [r for r in rows_of("*memory_copy_trace.csv") if "HOST_TO_DEVICE" in r.get("Direction", "").upper() and ns(r) >= 100_000]
    if not mine or not big:
        print(f"trace summary: no {KERNEL} launch or no H2D copy found under {directory}")
        return 1
    k_ns, c_ns = sum(ns(r) for r in mine), sum(ns(r) for r in big)
    print(f"trace summary: {len(mine)} {KERNEL} launches, {k_ns / 1e6:.3f} ms in all; {len(big)} H2D copies of 100 us or more, {c_ns / 1e6:.3f} ms in all "
          "(the copies of the VCF routes of the same run are among them: profile a run with --routes bcf for this line)")  # fmt: skip
    if staged_bytes > 0:
        print(f"trace summary: kernel {staged_bytes / k_ns:.1f} GB/s of GT bytes, H2D {staged_bytes / c_ns:.1f} GB/s (ceiling: PCIe Gen5 x16, "
              f"{PCIE_GBS:.0f} GB/s by specification); kernel rate / H2D rate = {c_ns / k_ns:.2f}")  # fmt: skip
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=2002)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20262)
    ap.add_argument("--routes", default="bcf,vcf_host_inflate,vcf_gpu_inflate,bcf_gpu_walk", help="comma-separated; the default is all four")
    ap.add_argument("--seg-bytes", default="4096,16384,65536", help="segment sizes of the GPU route's serial readings, comma-separated")
    ap.add_argument("--dir", default=None, help="where the inputs are written (kept and reused when given; default: a temporary directory)")
    ap.add_argument("--trace-summary", default=None, metavar="DIR")
    ap.add_argument("--staged-bytes", type=int, default=0, help="with --trace-summary: the GT bytes the BCF route of the profiled run staged")
    args = ap.parse_args()
    if args.trace_summary:
        return trace_summary(args.trace_summary, args.staged_bytes)

    import tempfile

    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine
    from sai_amd.utils import bcf, device_vcf

    holder = None if args.dir else tempfile.TemporaryDirectory(prefix="bcf_rate_")
    directory = Path(args.dir or holder.name)
    directory.mkdir(parents=True, exist_ok=True)
    t0 = time.perf_counter()
    vcf_path, bcf_path, names = write_inputs(directory, args.rows, args.samples, args.seed)
    print(f"inputs: {args.rows} rows x {args.samples} samples as {vcf_path} ({os.path.getsize(vcf_path)} bytes) and {bcf_path} "
          f"({os.path.getsize(bcf_path)} bytes), written or found in {time.perf_counter() - t0:.1f} s (not part of any figure)")  # fmt: skip
    eng = Engine.get(0)
    ploidies, genotypes = [2] * len(names), args.rows * args.samples

    def read_bcf(trace=None):
        os.environ["SAI_AMD_GPU_INFLATE"] = "0"
        return bcf.load_dosage_device(eng, bcf_path, "1", names, ploidies, trace=trace)

    def read_bcf_gpu_walk(trace=None):
        os.environ["SAI_AMD_GPU_INFLATE"] = "1"
        trace = {} if trace is None else trace
        got = bcf.load_dosage_device(eng, bcf_path, "1", names, ploidies, trace=trace)
        assert trace["route"] == "device", "the GPU route handed the read to the host route"
        return got

    def read_vcf(gpu_inflate):
        def read(trace=None):
            os.environ["SAI_AMD_GPU_INFLATE"] = "1" if gpu_inflate else "0"
            return device_vcf.load_dosage_device(eng, vcf_path, "1", names, ploidies)

        return read

    def timed_read(read):
        torch.cuda.synchronize()
        t = time.perf_counter()
        read()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    routes = {"bcf": read_bcf, "vcf_host_inflate": read_vcf(False), "vcf_gpu_inflate": read_vcf(True), "bcf_gpu_walk": read_bcf_gpu_walk}
    before = os.environ.get("SAI_AMD_GPU_INFLATE")
    result = {"rows": args.rows, "samples": args.samples, "routes": {}}
    reference = None
    for route in args.routes.split(","):
        read = routes[route]

        def timed(trace=None):
            torch.cuda.synchronize()
            t = time.perf_counter()
            pos, dos, _, _ = read(trace)
            torch.cuda.synchronize()
            return time.perf_counter() - t, pos, dos

        _, pos, dos = timed()  # warm-up: page-locks the staging buffers, loads the code object, fills the page cache
        assert len(pos) == args.rows and tuple(dos.shape) == (args.rows, args.samples), (route, len(pos), tuple(dos.shape))
        if reference is None:
            reference = dos
        else:
            assert torch.equal(dos, reference), f"{route}: the dosage block differs from the first route's"
        del dos
        whole = [timed()[0] for _ in range(args.repeats)]
        median, spread = sorted(whole)[len(whole) // 2], max(whole) - min(whole)
        print(f"{route}: read overlapped (as `score` reads it), ms per read: " + " ".join(f"{1e3 * t:.1f}" for t in whole))
        print(f"  median {1e3 * median:.1f} ms (spread {1e3 * spread:.1f}) = {genotypes / median / 1e9:.3f} G genotypes/s")
        result["routes"][route] = {"ms": [round(1e3 * t, 2) for t in whole], "median_ms": round(1e3 * median, 2), "spread_ms": round(1e3 * spread, 2),
                                   "genotypes_per_s": round(genotypes / median)}  # fmt: skip
    del reference
    if "bcf" in result["routes"]:
        base = result["routes"]["bcf"]["median_ms"]
        for route, got in result["routes"].items():
            if route != "bcf":
                print(f"bcf against {route}: {got['median_ms'] / base:.2f} times the genotypes per second")
        trace = {"serial": True}
        os.environ["SAI_AMD_GPU_INFLATE"] = "0"
        torch.cuda.synchronize()
        t = time.perf_counter()
        read_bcf(trace)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        staged, inflated = trace["staged_bytes"], trace["inflated_bytes"]
        print(f"bcf: every phase on its own ({1e3 * dt:.1f} ms in all; {inflated} bytes inflated, {staged} bytes of GT arrays staged), ms per phase:")
        phases = ("file_read", "inflate", "walk", "copy_to_staging", "wait_for_buffer", "h2d", "decode")
        for name in phases:
            n_bytes = inflated if name in ("inflate", "walk") else staged if name in ("copy_to_staging", "h2d", "decode") else 0
            rate = f"{n_bytes / trace[name] / 1e9:.1f} GB/s of {'inflated' if n_bytes == inflated else 'GT'} bytes" if n_bytes and trace.get(name) else ""
            print(f"  {name:16s} {1e3 * trace.get(name, 0.0):9.1f}   {rate}")
        slowest = max((p for p in phases if p != "wait_for_buffer"), key=lambda k: trace.get(k, 0.0))
        print(f"  the phase that bounds the route: {slowest}; kernel rate / H2D rate = {trace['h2d'] / trace['decode']:.2f}")
        print(f"staged: {args.repeats + 2} reads x {staged} bytes of GT arrays over PCIe on the BCF route (warm-up and the serial read included)")
        result["bcf_phases_ms"] = {k: round(1e3 * trace.get(k, 0.0), 2) for k in phases}
        result["bcf_bounded_by"] = slowest
        bcf.release_buffers(eng)
    if "bcf_gpu_walk" in result["routes"]:
        if "bcf" in result["routes"]:
            print(f"bcf_gpu_walk against bcf: {result['routes']['bcf']['median_ms'] / result['routes']['bcf_gpu_walk']['median_ms']:.2f} times the genotypes per second")
        phases = ("file_read", "header_inflate", "wait_for_buffer", "h2d", "inflate_gpu", "walk_gpu", "select", "decode")
        seg_before = os.environ.get("SAI_AMD_BCF_SEG_BYTES")
        result["bcf_gpu_walk_phases_ms"] = {}
        for seg in args.seg_bytes.split(","):
            os.environ["SAI_AMD_BCF_SEG_BYTES"] = seg
            read_bcf_gpu_walk()  # warm-up at this segment size
            trace = {"serial": True}
            torch.cuda.synchronize()
            t = time.perf_counter()
            read_bcf_gpu_walk(trace)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            whole = sorted(timed_read(read_bcf_gpu_walk) for _ in range(3))
            print(f"bcf_gpu_walk, seg_bytes {seg}: every phase on its own ({1e3 * dt:.1f} ms in all; {trace['comp_bytes']} compressed bytes over PCIe; "
                  f"walk_gpu = both kernels, the summaries and heads copied back and the stitch), overlapped median of 3: {1e3 * whole[1]:.1f} ms; ms per phase:")  # fmt: skip
            for name in phases:
                print(f"  {name:16s} {1e3 * trace.get(name, 0.0):9.1f}")
            result["bcf_gpu_walk_phases_ms"][seg] = {**{k: round(1e3 * trace.get(k, 0.0), 2) for k in phases}, "overlapped_median_ms": round(1e3 * whole[1], 2)}
        if seg_before is None:
            os.environ.pop("SAI_AMD_BCF_SEG_BYTES", None)
        else:
            os.environ["SAI_AMD_BCF_SEG_BYTES"] = seg_before
        bcf.release_buffers(eng)
    if before is None:
        os.environ.pop("SAI_AMD_GPU_INFLATE", None)
    else:
        os.environ["SAI_AMD_GPU_INFLATE"] = before
    print(json.dumps(result))
    if holder is not None:
        holder.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
