#!/usr/bin/env python3
"""Rate of `sai convert --out-pfile`, the kernels behind it and the fileset it writes, next to `--out-bfile`, in one call.

Writes, from a seed, --rows records x --samples unphased diploid calls on chromosome 1 as plain VCF text, once per width
of --samples: ``tools/pgen_rate.py``'s spectrum (alternative-allele frequencies with density 1 / x, 0.5 % missing calls;
writing is not timed).  Then, per width, with the file in the page cache, one process on one GPU:

  (1) the kernels: the plan, scan and write kernels of ``sai_pgen_encode`` over the whole block, one launch each
      (``stages``), and the D2H copy of the records plus the three tables, next to ``sai_bed_encode`` and the D2H copy
      of its rows; device events, alternating, after a warm-up round;
  (2) the bytes of the records against the bytes of the ``.bed`` rows, and on the first --check-rows rows the assertion
      that the records' total is the test writer's (``tests/pgen_builder.py``, the smallest of types 0, 1, 4, 6, 7);
  (3) ``convert --out-pfile`` against ``convert --out-bfile`` from the same file, wall time, alternating.  The condition:
      the ``.pgen`` route's median is not above the ``.bed`` route's by more than the larger of the two spreads;
  (4) ``score`` from the ``.pgen`` against ``score`` from the ``.bed`` (wall time; record only), and whether the two
      tables are the same bytes.

Every figure is a median with its spread (max - min) over --repeats.
"""

from __future__ import annotations

import argparse
import ctypes as C
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


def write_input(directory: Path, rows: int, samples: int, seed: int):
    """(path, names): the seeded calls as plain VCF text, found again when the file exists."""
    path = directory / f"pgen_export_{rows}x{samples}_{seed}.vcf"
    names = [f"s{k}" for k in range(samples)]
    if path.exists():
        return str(path), names
    rng = np.random.default_rng(seed)
    header = "##fileformat=VCFv4.2\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    text_of = np.array([b"0/0\t", b"0/1\t", b"1/1\t", b"./.\t"], dtype="S4")  # by hard-call code
    with open(path, "wb") as out:
        out.write(header.encode())
        pos = 0
        for lo in range(0, rows, CHUNK_ROWS):
            n = min(rows, lo + CHUNK_ROWS) - lo
            freq = np.exp(rng.uniform(np.log(0.5 / samples), np.log(0.5), size=n))  # density 1 / x
            codes = rng.binomial(2, freq[:, None], size=(n, samples)).astype(np.uint8)
            codes[rng.random(codes.shape) < 0.005] = 3
            steps = rng.integers(1, 200, n)
            text = []
            for k in range(n):
                pos += int(steps[k])
                text.append(f"1\t{pos}\tv{lo + k}\tA\tC\t.\tPASS\t.\tGT\t".encode() + text_of[codes[k]].tobytes()[:-1] + b"\n")
            out.write(b"".join(text))
    return str(path), names


def stats(values):
    values = sorted(values)
    return values[len(values) // 2], values[-1] - values[0]


def fmt(values, unit="ms"):
    med, spread = stats(values)
    return f"median {med:.3f} {unit} (spread {spread:.3f}; " + " ".join(f"{v:.3f}" for v in values) + ")"


def kernel_figures(eng, dos, repeats):
    """(1): {step: ms per repeat}, alternating; the records' bytes, the rows' bytes, the tables (host arrays)."""
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import bed_writer, pgen_writer as W

    bed, pgen = bed_writer.load(), W.load()
    n_rows, n_slots = dos.shape
    row_bytes = (n_slots + 3) // 4
    dense = n_rows * row_bytes
    rows_dev = torch.empty((dense,), dtype=torch.uint8, device=eng.device)
    rec_dev = torch.empty((dense,), dtype=torch.uint8, device=eng.device)
    vrtype = torch.empty((n_rows,), dtype=torch.uint8, device=eng.device)
    length, status, bed_status = (torch.empty((n_rows,), dtype=torch.int32, device=eng.device) for _ in range(3))
    offsets = torch.empty((n_rows + 1,), dtype=torch.int32, device=eng.device)
    pinned = torch.empty((dense,), dtype=torch.uint8).pin_memory()
    tables_pinned = torch.empty((9 * n_rows,), dtype=torch.uint8).pin_memory()
    stream = torch.cuda.current_stream(eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def stage(bits):
        _ffi.check(pgen.sai_pgen_encode(eng.ctx, p(dos), n_rows, n_slots, None, 2, p(rec_dev), p(vrtype), p(length), p(offsets), p(status), bits, C.c_void_p(stream.cuda_stream)))

    stage(W.ENCODE_ALL)
    torch.cuda.synchronize()
    total = int(offsets[n_rows].item()) & 0xFFFFFFFF

    def d2h_pgen():
        pinned[:total].copy_(rec_dev[:total], non_blocking=True)
        tables_pinned[:n_rows].copy_(vrtype, non_blocking=True)
        tables_pinned[n_rows : 5 * n_rows].copy_(length.view(torch.uint8), non_blocking=True)
        tables_pinned[5 * n_rows :].copy_(status.view(torch.uint8), non_blocking=True)

    steps = {
        "plan": lambda: stage(W.ENCODE_PLAN), "scan": lambda: stage(W.ENCODE_SCAN), "write": lambda: stage(W.ENCODE_WRITE), "pgen_d2h": d2h_pgen,
        "bed_encode": lambda: _ffi.check(bed.sai_bed_encode(eng.ctx, p(dos), n_rows, n_slots, None, 2, p(rows_dev), p(bed_status), C.c_void_p(stream.cuda_stream))),
        "bed_d2h": lambda: pinned.copy_(rows_dev, non_blocking=True),
    }  # fmt: skip
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
    assert not bool(status.any()) and not bool(bed_status.any()), "the seeded block holds a call that does not fit"
    return times, total, dense, vrtype.cpu().numpy(), length.cpu().numpy().view(np.uint32)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--samples", default="2000,2002", help="widths, comma-separated")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20264)
    ap.add_argument("--check-rows", type=int, default=2000, help="rows whose records are sized by the test writer as well")
    ap.add_argument("--dir", default=None, help="where the inputs and the filesets are written (kept when given; default: a temporary directory)")
    ap.add_argument("--no-score", action="store_true", help="leave (4) out")
    args = ap.parse_args()

    import tempfile

    import torch

    import __graft_entry__ as entry

    entry.build()
    import pgen_export_cases as PC
    from sai_amd.engine import Engine
    from sai_amd.sai import convert, score
    from sai_amd.utils import device_vcf

    holder = None if args.dir else tempfile.TemporaryDirectory(prefix="pgen_export_rate_")
    directory = Path(args.dir or holder.name)
    directory.mkdir(parents=True, exist_ok=True)
    eng = Engine.get(0)
    result = {"rows": args.rows, "widths": {}}
    for samples in (int(s) for s in args.samples.split(",")):
        t0 = time.perf_counter()
        vcf, names = write_input(directory, args.rows, samples, args.seed)
        print(f"== {args.rows} rows x {samples} samples: {vcf} ({os.path.getsize(vcf)} bytes), written or found in {time.perf_counter() - t0:.1f} s "
              "(not part of any figure)")  # fmt: skip
        here = result["widths"][samples] = {}
        # (1), (2)
        pos, dos, _, _ = device_vcf.load_dosage_device(eng, vcf, "1", names, [2] * samples)
        torch.cuda.synchronize()
        assert len(pos) == args.rows
        times, total, dense, vrtype, length = kernel_figures(eng, dos, args.repeats)
        print(f"(1) {args.rows * samples} bytes in; device events, alternating, ms:")
        for name in times:
            print(f"  {name:10s} {fmt(times[name])}")
        med = {name: stats(v)[0] for name, v in times.items()}
        print(f"  plan + scan + write = {med['plan'] + med['scan'] + med['write']:.3f} ms, with the D2H {med['plan'] + med['scan'] + med['write'] + med['pgen_d2h']:.3f} ms; "
              f"sai_bed_encode + its D2H = {med['bed_encode'] + med['bed_d2h']:.3f} ms")  # fmt: skip
        kinds = np.bincount(vrtype, minlength=8)
        print(f"(2) records {total} bytes, .bed rows {dense} bytes: {dense / total:.2f} times fewer; record types " +
              ", ".join(f"{k}: {int(c)}" for k, c in enumerate(kinds) if c))  # fmt: skip
        check = min(args.check_rows, args.rows)
        block = dos[:check].cpu().numpy()
        codes = np.select([block == 0, block == 1, block == 2], [0, 1, 2], 3).astype(np.uint8)
        want_types, want_records = PC.reference_of(("rate", samples), codes)
        assert vrtype[:check].tolist() == want_types and length[:check].tolist() == [len(r) for r in want_records], "the kernels and the test writer disagree"
        print(f"    the first {check} rows: types and lengths are the test writer's ({sum(len(r) for r in want_records)} bytes)")
        here["kernel_ms"] = {k: [round(v, 4) for v in vs] for k, vs in times.items()}
        here["bytes"] = {"records": total, "bed_rows": dense}
        del dos
        # (3)
        runs, phases = {"pfile": [], "bfile": []}, {"pfile": [], "bfile": []}
        prefix = {kind: str(directory / f"out_{samples}_{kind}") for kind in runs}
        for rep in range(args.repeats + 1):  # the first round is the warm-up
            for kind in ("pfile", "bfile"):
                for ext in (".bed", ".bim", ".fam", ".pgen", ".pvar", ".psam"):
                    if os.path.exists(prefix[kind] + ext):
                        os.remove(prefix[kind] + ext)
                torch.cuda.synchronize()
                t = time.perf_counter()
                summary = convert(vcf, "1", **({"out_pfile": prefix[kind]} if kind == "pfile" else {"out_prefix": prefix[kind]}))
                dt = (time.perf_counter() - t) * 1e3
                if rep:
                    runs[kind].append(dt), phases[kind].append(summary["ms"])
        for kind in runs:
            print(f"(3) convert --out-{kind}, wall ms: {fmt(runs[kind])}")
            for phase in ("read", "site_scan", "encode", "d2h", "write"):
                print(f"      {phase:10s} {fmt([s[phase] for s in phases[kind]])}")
        (p_med, p_spread), (b_med, b_spread) = stats(runs["pfile"]), stats(runs["bfile"])
        holds = p_med <= b_med + max(p_spread, b_spread)
        print(f"    condition (.pgen median not above .bed median by more than the larger spread): {'holds' if holds else 'DOES NOT HOLD'}: "
              f"{p_med:.1f} ms against {b_med:.1f} ms + {max(p_spread, b_spread):.1f} ms")  # fmt: skip
        if not holds:
            worst = max(("encode", "d2h", "write"), key=lambda ph: stats([s[ph] for s in phases["pfile"]])[0] - stats([s[ph] for s in phases["bfile"]])[0])
            print(f"    the phase that grew most against the .bed route: {worst}")
        sizes = {ext: os.path.getsize(prefix["pfile" if ext.startswith(".p") else "bfile"] + ext) for ext in (".pgen", ".pvar", ".psam", ".bed", ".bim", ".fam")}
        print(f"    files: {sizes}; .bed / .pgen = {sizes['.bed'] / sizes['.pgen']:.2f}")
        here["convert_ms"], here["phases_ms"], here["condition_holds"], here["sizes"] = runs, phases, bool(holds), sizes
        # (4)
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
            for label, source in (("pgen", prefix["pfile"] + ".pgen"), ("bed", prefix["bfile"] + ".bed")):
                took = []
                for rep in range(min(args.repeats, 3) + 1):
                    out = directory / f"score_{samples}_{label}.tsv"
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    score(vcf_file=source, chr_name="1", win_len=50000, win_step=10000, anc_allele_file=None, output_file=str(out), config=str(cfg),
                          num_workers=1, layout="int8")  # fmt: skip
                    torch.cuda.synchronize()
                    if rep:
                        took.append((time.perf_counter() - t) * 1e3)
                outputs[label] = out.read_bytes()
                print(f"(4) score from the .{label:5s} wall ms: {fmt(took)}")
                here[f"score_{label}_ms"] = took
            print(f"    the two score tables are {'byte-identical' if outputs['pgen'] == outputs['bed'] else 'DIFFERENT'}")
        if holder is not None:  # a temporary directory holds one width at a time
            for path in directory.iterdir():
                path.unlink()
    print(json.dumps(result))
    if holder is not None:
        holder.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
