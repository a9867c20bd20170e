#!/usr/bin/env python3
"""What a packed2 block of a PLINK 1 fileset costs by the two routes, in the same call, alternating:

  (a) the int8 route to a packed block: ``plink.load_dosage_device`` (the int8 [record][slot] block) ->
      ``Engine.tile_columns`` per population -> ``Engine.pack2`` per population;
  (b) ``plink.load_packed_device``: the ``.bed`` rows decoded straight into the layout (``sai_bed_pack2``).

Writes, from a seed, ONE ``.bed`` of --rows x --samples genotypes on chromosome 1 (the file of ``plink_rate.py``:
the shape of profiles/plink_ingest.txt; writing is not timed) and reads it as three populations: the first and the
second half of the samples but two, and the last two.  Per route: --repeats end-to-end reads after one warm-up
(host clock around a device synchronise), one read with every phase synchronised on its own (``trace["serial"]``:
index, file read, H2D, decode -- the decode kernel's time and its rate over the input bytes -- and for (a) re-tile and
pack), and ``torch.cuda.max_memory_allocated`` of a read.  The blocks of the two routes are compared once.  Then one
``ResidentScorer`` step over the block in each layout.

``SAI_BED_PACK2_GROUPS`` (groups of 64 individuals a wavefront of the new kernel walks, default 8) is read once
per process: ``--routes b`` measures route (b) alone, for a sweep over it.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for entry_dir in (ROOT, ROOT / "tools"):
    if str(entry_dir) not in sys.path:
        sys.path.insert(0, str(entry_dir))

from plink_rate import PCIE_GBS, write_inputs  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--samples", type=int, default=2002)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261)
    ap.add_argument("--routes", default="ab", choices=("ab", "b"))
    ap.add_argument("--steps", type=int, default=5, help="timed ResidentScorer steps per layout")
    ap.add_argument("--dir", default=None, help="where the input is written (kept and reused when given; default: a temporary directory)")
    args = ap.parse_args()

    import tempfile

    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd import _ffi
    from sai_amd.engine import Engine
    from sai_amd.packed_scorer import packed_scorer
    from sai_amd.resident import ResidentBlock, ResidentScorer, default_windows
    from sai_amd.utils import plink

    holder = None if args.dir else tempfile.TemporaryDirectory(prefix="plink_packed_rate_")
    directory = Path(args.dir or holder.name)
    directory.mkdir(parents=True, exist_ok=True)
    t0 = time.perf_counter()
    bed, _, names = write_inputs(directory, args.rows, args.samples, 0, args.seed)
    data_bytes = args.rows * ((args.samples + 3) // 4)
    half = (args.samples - 2) // 2
    pops = [(names[:half], 2), (names[half : args.samples - 2], 2), (names[args.samples - 2 :], 2)]
    bounds = [0, half, args.samples - 2, args.samples]
    print(f"input: {bed}.bed, {os.path.getsize(bed + '.bed')} bytes ({args.rows} rows x {args.samples} samples), written or found in "
          f"{time.perf_counter() - t0:.1f} s (not part of any figure); populations of {', '.join(str(len(n)) for n, _ in pops)} samples; "
          f"SAI_BED_PACK2_GROUPS={os.environ.get('SAI_BED_PACK2_GROUPS', 'unset (8)')}")  # fmt: skip
    eng = Engine.get(0)

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    def route_a(trace=None):
        """(seconds, pos, [TiledPop], [PackedPop]); the int8 block is dropped before the function returns."""
        t = sync()
        pos, dos, _, _ = plink.load_dosage_device(eng, bed, "1", names, [2] * len(names), trace=trace)
        t1 = sync()
        tiled = [eng.tile_columns(dos, list(range(lo, hi))) for lo, hi in zip(bounds, bounds[1:])]
        t2 = sync()
        packed = [eng.pack2(p) for p in tiled]
        t3 = sync()
        if trace is not None:
            trace["re-tile"], trace["pack"] = t2 - t1, t3 - t2
        return t3 - t, pos, tiled, packed

    def route_b(trace=None):
        t = sync()
        pos, packed, _, _ = plink.load_packed_device(eng, bed, "1", pops, trace=trace)
        return sync() - t, pos, None, packed

    routes = {"a": route_a, "b": route_b} if args.routes == "ab" else {"b": route_b}
    label = {"a": "(a) load_dosage_device -> tile_columns -> pack2", "b": "(b) load_packed_device"}
    result = {"rows": args.rows, "samples": args.samples, "data_bytes": data_bytes, "routes": {}}
    blocks = {}
    for key, read in routes.items():  # warm-up: page-locks the staging buffers, loads the code objects
        _, pos, _, packed = read()
        assert len(pos) == args.rows
        blocks[key] = [p.data for p in packed]
    if len(blocks) == 2:
        assert all(torch.equal(x, y) for x, y in zip(blocks["a"], blocks["b"])), "the two routes give different blocks"
        print("the packed blocks of the two routes are equal byte for byte")
    del blocks, packed
    times = {key: [] for key in routes}
    for _ in range(args.repeats):  # alternating: both routes see the same machine
        for key, read in routes.items():
            times[key].append(read()[0])
    for key, read in routes.items():
        whole = times[key]
        median, spread = sorted(whole)[len(whole) // 2], max(whole) - min(whole)
        print(f"{label[key]}: end to end, ms per read: " + " ".join(f"{1e3 * t:.1f}" for t in whole))
        print(f"  median {1e3 * median:.1f} ms (spread {1e3 * spread:.1f}) = {data_bytes / median / 1e9:.2f} GB/s of .bed")
        trace = {"serial": True}
        dt = read(trace)[0]
        n_bytes = trace["bed_bytes"]
        phases = ["index", "file_read", "h2d", "decode"] + (["re-tile", "pack"] if key == "a" else [])
        print(f"{label[key]}: every phase synchronised on its own ({1e3 * dt:.1f} ms in all), ms per phase:")
        for name in phases:
            note = ""
            if name in ("file_read", "h2d", "decode"):
                note = f"{n_bytes / trace[name] / 1e9:.1f} GB/s of .bed"
            if name == "h2d":
                note += f"; ceiling PCIe Gen5 x16, {PCIE_GBS:.0f} GB/s by specification"
            if name == "decode":
                note += " (the decode kernel, a launch and a synchronise per batch and population included)"
            print(f"  {name:9s} {1e3 * trace[name]:9.1f}   {note}")
        print(f"  decode rate / H2D rate = {trace['h2d'] / trace['decode']:.2f} (the kernel must not be the bound: >= 1)")
        plink.release_buffers(eng)
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        kept = read()
        peak = torch.cuda.max_memory_allocated() - base
        held = sum(p.data.numel() for p in kept[3])
        print(f"  max_memory_allocated over a read (staging included): {peak / 1e6:.1f} MB above the start; the packed blocks it leaves: {held / 1e6:.1f} MB")
        del kept
        result["routes"][key] = {"ms": [round(1e3 * t, 2) for t in whole], "median_ms": round(1e3 * median, 2), "spread_ms": round(1e3 * spread, 2),
                                 "phases_ms": {k: round(1e3 * trace[k], 2) for k in phases}, "peak_bytes": int(peak)}  # fmt: skip
    if len(routes) == 2:
        a, b = result["routes"]["a"], result["routes"]["b"]
        print(f"(b) / (a): end to end {b['median_ms'] / a['median_ms']:.2f}, peak memory {b['peak_bytes'] / a['peak_bytes']:.2f}; "
              f"(b) decode {b['phases_ms']['decode']:.1f} ms against (a) decode + re-tile + pack "
              f"{a['phases_ms']['decode'] + a['phases_ms']['re-tile'] + a['phases_ms']['pack']:.1f} ms")  # fmt: skip
        # one scorer step per layout on the block
        _, pos, tiled, _ = route_a()
        _, _, _, packed = route_b()
        pos_dev = torch.from_numpy(pos).to(eng.device)
        windows = default_windows(int(pos[0]), int(pos[-1]), 50000, 10000)
        sets = [_ffi.make_params(0.01, 0.5, 0.95, [("=", 1.0)], False, n_src=1)]
        result["step_ms"] = {}
        for name, scorer in (("int8", ResidentScorer(eng, ResidentBlock(tiled, [2, 2, 2], pos_dev), windows, sets)),
                             ("packed2", packed_scorer(eng, ResidentBlock(packed, [2, 2, 2], pos_dev), windows, sets))):  # fmt: skip
            for _ in range(2):
                scorer.step()
            scorer.results(grow=True)
            wall = []
            for _ in range(args.steps):
                t = sync()
                scorer.step(time_counts=True)
                scorer.results(grow=True)
                wall.append(time.perf_counter() - t)
            site = scorer.site_pass_ms()
            print(f"ResidentScorer step, {name}: {len(windows)} windows, site pass ms: " + " ".join(f"{v:.3f}" for v in site) +
                  "; step + results, host clock, ms: " + " ".join(f"{1e3 * v:.3f}" for v in wall))  # fmt: skip
            result["step_ms"][name] = {"site_pass": [round(v, 3) for v in site], "step_and_results": [round(1e3 * v, 3) for v in wall]}
            scorer.close()
    print(json.dumps(result))
    if holder is not None:
        holder.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
