#!/usr/bin/env python3
"""Rate of the gathering re-tile (``sai_tile_rows_from_site_major``, sai_amd/csrc/join/tile_rows.hip) next to what it
replaces, on the same blocks in the same call:

  (a) ``sai_tile_from_site_major``                      -- the re-tile of the one-input read, every row;
  (b) the new kernel with ``rows = NULL``               -- the same bytes, so (b) against (a) is kernel against kernel;
  (c) the new kernel with a list of about 90 % of the rows, against
  (d) ``index_select`` of those rows + ``sai_tile_from_site_major`` of the copy -- which moves every genotype twice.

One process.  Two block shapes from a seed, random int8: --sites x 2 002 samples cut into populations of 1 000 / 1 000 / 2
columns (the shape profiles/plink_ingest.txt was taken at), and --sites x 4 samples as one population (a narrow source
block).  The outputs of (a) and (b), and of (c) and (d), are asserted equal byte for byte first.  Then, after a warm-up of
all, --repeats timed runs of each, alternating; a run is --inner back-to-back calls (one call = all populations of the
block) between two device events, reported per call.  Bytes are the algorithm's: every selected genotype read once and
written once (the padding of the last tile and the 4-byte row indices are not counted); (d) is charged the same bytes, so
its GB/s says what the caller gets, not what the memory system moves.  The gates compare medians, with the larger spread
of the two as the margin: (b) not slower than (a), (c) not slower than (d).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GATHER_CEILING_GBS = 6000.0  # gathering ~1 KB rows by index through LDS from HBM, chip-wide: the figure DESIGN_INGEST.md cites


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="calls per timed run")
    ap.add_argument("--keep", type=float, default=0.9, help="share of the rows the list of (c) and (d) keeps")
    ap.add_argument("--seed", type=int, default=20264)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")

    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine
    from sai_amd.site_join_device import RowTiler

    eng = Engine.get(0)
    gen = torch.Generator(device=eng.device).manual_seed(args.seed)
    tiler = RowTiler(eng)
    result = {"sites": args.sites, "inner": args.inner, "keep": args.keep, "shapes": []}
    all_passed = True
    for name, width, sizes in (("wide", 2002, (1000, 1000, 2)), ("narrow", 4, (4,))):
        n = args.sites
        block = torch.randint(-128, 128, (n, width), dtype=torch.int8, device=eng.device, generator=gen)
        kept = torch.nonzero(torch.rand(n, device=eng.device, generator=gen) < args.keep).reshape(-1)
        rows32, rows64 = kept.to(torch.int32), kept
        runs_of = [(sum(sizes[:k]), size) for k, size in enumerate(sizes)]  # (first column, columns) of every population

        def old_kernel():
            return [eng.tile_columns(block, list(range(c0, c0 + w))) for c0, w in runs_of]

        def new_identity():
            return [tiler.tile(block, c0, w) for c0, w in runs_of]

        def new_gather():
            return [tiler.tile(block, c0, w, rows32) for c0, w in runs_of]

        def two_steps():
            copy = block.index_select(0, rows64)
            return [eng.tile_columns(copy, list(range(c0, c0 + w))) for c0, w in runs_of]

        forms = {"a_old_kernel": old_kernel, "b_new_identity": new_identity, "c_new_gather": new_gather, "d_index_select_then_old": two_steps}
        for x, y in (("a_old_kernel", "b_new_identity"), ("c_new_gather", "d_index_select_then_old")):
            for p, q in zip(forms[x](), forms[y]()):
                assert (p.n_sites, p.n_ind) == (q.n_sites, q.n_ind) and torch.equal(p.tiles, q.tiles), f"{name}: {x} and {y} differ"
        tiler.check()
        n_kept = int(kept.numel())
        moved = {"a_old_kernel": 2 * n * sum(sizes), "b_new_identity": 2 * n * sum(sizes), "c_new_gather": 2 * n_kept * sum(sizes),
                 "d_index_select_then_old": 2 * n_kept * sum(sizes)}  # fmt: skip
        print(f"shape {name}: {n} rows x {width} samples, populations of {' / '.join(map(str, sizes))} columns; the list keeps {n_kept} rows "
              f"({n_kept / n:.3f}); outputs equal byte for byte: (a) = (b), (c) = (d)")  # fmt: skip

        def timed(fn) -> float:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(args.inner):
                fn()
            stop.record()
            torch.cuda.synchronize()
            tiler._bad.clear()  # the counts were read above; nothing of a timed run is kept
            return start.elapsed_time(stop) / args.inner  # ms per call

        for fn in forms.values():  # warm-up: code objects, the allocator's blocks
            timed(fn)
        ms = {form: [] for form in forms}
        for _ in range(args.repeats):
            for form, fn in forms.items():
                ms[form].append(timed(fn))
        shape = {"name": name, "width": width, "sizes": list(sizes), "kept_rows": n_kept, "forms": {}}
        for form, runs in ms.items():
            median, spread = sorted(runs)[len(runs) // 2], max(runs) - min(runs)
            gbs = moved[form] / (median * 1e-3) / 1e9
            print(f"  {form}: ms per call, {args.inner} calls per run: " + " ".join(f"{t:.4f}" for t in runs))
            print(f"    median {median:.4f} ms (spread {spread:.4f}) = {gbs:.0f} GB/s of read + write = {gbs / GATHER_CEILING_GBS:.3f} of "
                  f"{GATHER_CEILING_GBS / 1000:.1f} TB/s")  # fmt: skip
            shape["forms"][form] = {"ms": [round(t, 5) for t in runs], "median_ms": round(median, 5), "spread_ms": round(spread, 5),
                                    "gb_per_s": round(gbs, 1), "of_gather_ceiling": round(gbs / GATHER_CEILING_GBS, 4)}  # fmt: skip
        f = shape["forms"]
        for gate, x, y in (("b_not_slower_than_a", "b_new_identity", "a_old_kernel"), ("c_not_slower_than_d", "c_new_gather", "d_index_select_then_old")):
            margin = max(f[x]["spread_ms"], f[y]["spread_ms"])
            shape[gate] = f[x]["median_ms"] <= f[y]["median_ms"] + margin
            all_passed &= shape[gate]
            print(f"  gate {gate}: {f[x]['median_ms']:.4f} ms against {f[y]['median_ms']:.4f} ms ({f[x]['median_ms'] / f[y]['median_ms']:.3f} of the "
                  f"time; margin {margin:.4f} ms, the larger spread): {'passed' if shape[gate] else 'FAILED'}")  # fmt: skip
        result["shapes"].append(shape)
        del block, kept, rows32, rows64
        torch.cuda.empty_cache()
    result["gates_passed"] = bool(all_passed)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
