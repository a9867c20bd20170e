#!/usr/bin/env python3
"""What a packed2 block of a PLINK 2 fileset costs by the two routes, in the same call, alternating:

  (a) the int8 route to a packed block: ``pgen.load_dosage_device`` (the int8 [record][slot] block) ->
      ``Engine.tile_columns`` per population -> ``Engine.pack2`` per population;
  (b) ``pgen.load_packed_device``: the records decoded straight into the layout (``sai_pgen_pack2``).

The input is the panel-like fileset of ``pgen_rate.py`` (--rows x --samples genotypes on chromosome 1 with a 1 / x
frequency spectrum and 0.5 % missing calls, the smallest encoding per record; written by pure Python, so keep --rows
modest -- writing is not timed and is skipped when the files exist, ``--write-only`` stops there and needs no GPU).
It is read as three populations: the first and the second half of the samples but two, and the last two.  Per route:
--repeats end-to-end reads after one warm-up (host clock around a device synchronise; the files are in the page cache
by then), their median and their spread (max - min), and one read with every phase synchronised on its own
(``trace["serial"]``: index, file read, H2D, decode -- the decode kernel's time and its rate over the file's bytes --
and for (a) re-tile and pack), and ``torch.cuda.max_memory_allocated`` of a read.  The blocks of the two routes are
compared once.  What is printed is also written to --out (default profiles/pgen_packed_ingest.txt).

The kernels' own rates come from a run of their own,
``rocprofv3 --kernel-trace --memory-copy-trace --stats -- python tools/pgen_packed_rate.py ...`` (no counters in it).
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for entry_dir in (ROOT, ROOT / "tools", ROOT / "tests"):
    if str(entry_dir) not in sys.path:
        sys.path.insert(0, str(entry_dir))

from pgen_rate import write_inputs  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", required=True, help="where the input is written (kept and reused)")
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--samples", type=int, default=2002)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--write-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pgen_packed_ingest.txt"))
    args = ap.parse_args()
    directory = Path(args.dir)
    directory.mkdir(parents=True, exist_ok=True)
    prefix = write_inputs(directory, args.rows, args.samples, args.seed)
    if args.write_only:
        return 0

    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine
    from sai_amd.utils import pgen

    lines = []

    def say(text: str) -> None:
        print(text, flush=True)
        lines.append(text)

    names = [f"s{i}" for i in range(args.samples)]
    file_bytes = os.path.getsize(prefix + ".pgen")
    half = (args.samples - 2) // 2
    pops = [(names[:half], 2), (names[half : args.samples - 2], 2), (names[args.samples - 2 :], 2)]
    bounds = [0, half, args.samples - 2, args.samples]
    say("command: python tools/pgen_packed_rate.py " + " ".join(a if a != args.dir else "DIR" for a in sys.argv[1:]))
    say(f"input: {os.path.basename(prefix)}.pgen, {file_bytes} bytes ({args.rows} rows x {args.samples} samples; the .bed of the same genotypes: "
        f"{args.rows * ((args.samples + 3) // 4)} bytes); populations of {', '.join(str(len(n)) for n, _ in pops)} samples")  # fmt: skip
    eng = Engine.get(0)

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    def route_a(trace=None):
        """(seconds, pos, [PackedPop]); the int8 block and the tiled copies are dropped before the function returns."""
        t = sync()
        pos, dos, _, _ = pgen.load_dosage_device(eng, prefix, "1", names, [2] * len(names), trace=trace)
        t1 = sync()
        tiled = [eng.tile_columns(dos, list(range(lo, hi))) for lo, hi in zip(bounds, bounds[1:])]
        t2 = sync()
        packed = [eng.pack2(p) for p in tiled]
        t3 = sync()
        if trace is not None:
            trace["re-tile"], trace["pack"] = t2 - t1, t3 - t2
        return t3 - t, pos, packed

    def route_b(trace=None):
        t = sync()
        pos, packed, _, _ = pgen.load_packed_device(eng, prefix, "1", pops, trace=trace)
        return sync() - t, pos, packed

    routes = {"a": route_a, "b": route_b}
    label = {"a": "(a) load_dosage_device -> tile_columns -> pack2", "b": "(b) load_packed_device"}
    result = {"rows": args.rows, "samples": args.samples, "pgen_bytes": file_bytes, "routes": {}}
    blocks = {}
    for key, read in routes.items():  # warm-up: page-locks the staging buffers, loads the code objects, fills the page cache
        _, pos, packed = read()
        assert len(pos) == args.rows
        blocks[key] = [p.data for p in packed]
    assert all(torch.equal(x, y) for x, y in zip(blocks["a"], blocks["b"])), "the two routes give different blocks"
    say("the packed blocks of the two routes are equal byte for byte")
    del blocks, packed
    times = {key: [] for key in routes}
    for _ in range(args.repeats):  # alternating: both routes see the same machine
        for key, read in routes.items():
            times[key].append(read()[0])
    for key, read in routes.items():
        whole = times[key]
        median, spread = statistics.median(whole), max(whole) - min(whole)
        say(f"{label[key]}: end to end, ms per read: " + " ".join(f"{1e3 * t:.1f}" for t in whole))
        say(f"  median {1e3 * median:.1f} ms (spread {1e3 * spread:.1f}) = {file_bytes / median / 1e9:.3f} GB/s of .pgen")
        trace = {"serial": True}
        dt = read(trace)[0]
        n_bytes = trace["pgen_bytes"]
        phases = ["index", "file_read", "h2d", "decode"] + (["re-tile", "pack"] if key == "a" else [])
        say(f"{label[key]}: every phase synchronised on its own ({1e3 * dt:.1f} ms in all), ms per phase:")
        for name in phases:
            note = f"{n_bytes / trace[name] / 1e9:.2f} GB/s of .pgen" if name in ("file_read", "h2d", "decode") else ""
            if name == "decode":
                note += " (the decode kernel, a launch and a synchronise per batch" + (" and population" if key == "b" else "") + " included)"
            say(f"  {name:9s} {1e3 * trace[name]:9.1f}   {note}")
        pgen.release_buffers(eng)
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        kept = read()
        peak = torch.cuda.max_memory_allocated() - base
        held = sum(p.data.numel() for p in kept[2])
        say(f"  max_memory_allocated over a read (staging included): {peak / 1e6:.1f} MB above the start; the packed blocks it leaves: {held / 1e6:.1f} MB")
        del kept
        result["routes"][key] = {"ms": [round(1e3 * t, 2) for t in whole], "median_ms": round(1e3 * median, 2), "spread_ms": round(1e3 * spread, 2),
                                 "phases_ms": {k: round(1e3 * trace[k], 2) for k in phases}, "peak_bytes": int(peak)}  # fmt: skip
    a, b = result["routes"]["a"], result["routes"]["b"]
    say(f"(b) - (a), medians: {b['median_ms'] - a['median_ms']:+.1f} ms, against a margin (the spread of the five reads of (a)) of {a['spread_ms']:.1f} ms; "
        f"(b) / (a): end to end {b['median_ms'] / a['median_ms']:.2f}, peak memory {b['peak_bytes'] / a['peak_bytes']:.2f}; "
        f"(b) decode {b['phases_ms']['decode']:.1f} ms against (a) decode + re-tile + pack "
        f"{a['phases_ms']['decode'] + a['phases_ms']['re-tile'] + a['phases_ms']['pack']:.1f} ms")  # fmt: skip
    say(json.dumps(result))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
