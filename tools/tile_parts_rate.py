#!/usr/bin/env python3
"""Rate of the re-tile from parts (``sai_tile_rows_from_parts``, sai_amd/csrc/join/tile_parts.hip) next to the two forms
it can be measured against, on the same blocks in the same call:

  (a) the only composition that gives the same population today: ``index_select`` of every part's rows, ``torch.cat``
      of the copies along the individuals, ``sai_tile_from_site_major`` of the result -- every genotype moved three times;
  (b) one ``sai_tile_rows_from_site_major`` launch per part into separate populations -- NOT equivalent (P populations
      instead of one): the floor for P launches that gather while they tile;
  (n) the new kernel: one launch, every part gathered by its own list.

One process.  Two shapes from a seed, random int8: "genomes" -- four parts of one individual each, one archaic genome
per file -- and "wide" -- parts of 1 000 + 2 individuals, a wide part next to a narrow one.  Every part is a block of
--sites rows of its own with an ascending list of about --keep of them; all lists are cut to the shortest.  The outputs of
(n) and (a) are asserted equal byte for byte first, and every population of (b) against ``index_select`` + the old
kernel.  Then, after a warm-up of all, --repeats timed runs of each form, alternating; a run is --inner back-to-back
calls between two device events, reported per call.  Bytes are the algorithm's: every selected genotype read once and
written once (padding and the 4-byte row indices are not counted); every form is charged the same bytes.  No ratio is
fixed in advance: the medians, their spreads and the ratios are reported.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="calls per timed run")
    ap.add_argument("--keep", type=float, default=0.9, help="share of its rows every part's list keeps")
    ap.add_argument("--seed", type=int, default=20265)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")

    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine
    from sai_amd.site_join_device import RowTiler
    from sai_amd.site_join_parts import tile_parts

    eng = Engine.get(0)
    gen = torch.Generator(device=eng.device).manual_seed(args.seed)
    tiler = RowTiler(eng)
    result = {"sites": args.sites, "inner": args.inner, "keep": args.keep, "shapes": []}
    for name, widths in (("genomes", (1, 1, 1, 1)), ("wide", (1000, 2))):
        n = args.sites
        blocks = [torch.randint(-128, 128, (n, w), dtype=torch.int8, device=eng.device, generator=gen) for w in widths]
        kept = [torch.nonzero(torch.rand(n, device=eng.device, generator=gen) < args.keep).reshape(-1) for _ in widths]
        n_rows = min(int(k.numel()) for k in kept)
        rows64 = [k[:n_rows].contiguous() for k in kept]
        rows32 = [k.to(torch.int32) for k in rows64]
        n_ind = sum(widths)

        def composed():
            stacked = torch.cat([b.index_select(0, r) for b, r in zip(blocks, rows64)], dim=1)
            return [eng.tile_columns(stacked, list(range(n_ind)))]

        def per_part():
            return [tiler.tile(b, 0, w, r) for b, w, r in zip(blocks, widths, rows32)]

        def from_parts():
            return [tile_parts(tiler, [(b, 0, w, r) for b, w, r in zip(blocks, widths, rows32)], n_rows)]

        forms = {"a_index_select_cat_old": composed, "b_one_launch_per_part": per_part, "n_from_parts": from_parts}
        (p,), (q,) = composed(), from_parts()
        assert (p.n_sites, p.n_ind) == (q.n_sites, q.n_ind) == (n_rows, n_ind) and torch.equal(p.tiles, q.tiles), f"{name}: (n) and (a) differ"
        for got, b, w, r in zip(per_part(), blocks, widths, rows64):
            want = eng.tile_columns(b.index_select(0, r), list(range(w)))
            assert torch.equal(got.tiles, want.tiles), f"{name}: a population of (b) differs"
        tiler.check()
        del p, q, got, want
        moved = 2 * n_rows * n_ind
        print(f"shape {name}: parts of {' + '.join(map(str, widths))} individuals, {n} rows a block; every list keeps {n_rows} rows "
              f"({n_rows / n:.3f}); outputs equal byte for byte: (n) = (a), every population of (b) = index_select + the old kernel")  # fmt: skip

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
        shape = {"name": name, "widths": list(widths), "kept_rows": n_rows, "forms": {}}
        for form, runs in ms.items():
            median, spread = sorted(runs)[len(runs) // 2], max(runs) - min(runs)
            gbs = moved / (median * 1e-3) / 1e9
            print(f"  {form}: ms per call, {args.inner} calls per run: " + " ".join(f"{t:.4f}" for t in runs))
            print(f"    median {median:.4f} ms (spread {spread:.4f}) = {gbs:.0f} GB/s of read + write")
            shape["forms"][form] = {"ms": [round(t, 5) for t in runs], "median_ms": round(median, 5), "spread_ms": round(spread, 5),
                                    "gb_per_s": round(gbs, 1)}  # fmt: skip
        f = shape["forms"]
        for against in ("a_index_select_cat_old", "b_one_launch_per_part"):
            ratio = f["n_from_parts"]["median_ms"] / f[against]["median_ms"]
            shape[f"n_over_{against[0]}"] = round(ratio, 4)
            print(f"  (n) against ({against[0]}): {f['n_from_parts']['median_ms']:.4f} ms against {f[against]['median_ms']:.4f} ms = {ratio:.3f} of the time")
        result["shapes"].append(shape)
        del blocks, kept, rows64, rows32
        torch.cuda.empty_cache()
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
