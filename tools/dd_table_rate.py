#!/usr/bin/env python3
"""DD of one source population by the table route (sai_amd/dd_table.py, sai_amd/csrc/dd_table/dd_table.hip) next to the
route it replaces, on the same blocks in the same call:

  (o) the old route: ``Engine.site_absdiff`` of ref and of tgt -- one stream of the population per two source
      individuals, a term tensor uint32 [n_src_ind][n_sites] each -- and ``Engine.window_dd``;
  (t) the table route: ``site_absdiff_table`` of ref and of tgt -- one stream each, 28 bytes per site written -- and
      ``window_dd_table``.

One process.  Random dosages 0 .. 2 from a seed (the window kernel's lookups are data-dependent; the streaming passes
are not), --sites sites, --ref + --tgt individuals, windows of --window sites at a step of half of that, source
populations of 5, 8, 32 and 128 individuals.  Per source count the two routes' DD are asserted equal bit for bit first.
Then, after a warm-up of both, --repeats timed runs of each, alternating; a run is --inner back-to-back calls between two
device events, reported per call.  The table passes are also timed alone and charged their own bytes: every genotype
read once plus 28 bytes per site and population written.  No ratio is fixed in advance: the medians, their spreads and
the ratios are reported, and written with everything else to --out.
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
    ap.add_argument("--sites", type=int, default=1 << 20)
    ap.add_argument("--ref", type=int, default=1000)
    ap.add_argument("--tgt", type=int, default=1000)
    ap.add_argument("--window", type=int, default=500, help="sites per window; the step is half of it")
    ap.add_argument("--sources", type=int, nargs="+", default=[5, 8, 32, 128])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2, help="calls per timed run")
    ap.add_argument("--seed", type=int, default=20266)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dd_table.txt"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")

    import torch

    import __graft_entry__ as entry

    entry.build()
    import bench
    from sai_amd import dd_table
    from sai_amd.engine import Engine

    lines = []

    def say(text: str) -> None:
        print(text, flush=True)
        lines.append(text)

    eng = Engine.get(0)
    gen = torch.Generator(device=eng.device).manual_seed(args.seed)
    n = args.sites

    def block(n_ind):
        return eng.tile(torch.randint(0, 3, (n, n_ind), dtype=torch.int8, device=eng.device, generator=gen))

    ref_t, tgt_t = block(args.ref), block(args.tgt)
    starts = torch.arange(0, max(n - args.window, 1), max(args.window // 2, 1), dtype=torch.int32, device=eng.device)
    lo, hi = starts.contiguous(), (starts + args.window).clamp(max=n).contiguous()
    say(f"dd_table_rate: {torch.cuda.get_device_name(0)}, sources {bench.source_digest()}, {n} sites, ref {args.ref} + tgt {args.tgt} individuals, "
        f"{int(lo.numel())} windows of {args.window} sites, {args.inner} calls per run, {args.repeats} runs per form")  # fmt: skip

    def timed(fn) -> float:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.inner):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.inner  # ms per call

    def summary(runs):
        return sorted(runs)[len(runs) // 2], max(runs) - min(runs)

    result = {"sites": n, "ref": args.ref, "tgt": args.tgt, "windows": int(lo.numel()), "window": args.window, "inner": args.inner,
              "source_digest": bench.source_digest(), "sources": []}  # fmt: skip

    def tables():
        return dd_table.site_absdiff_table(eng, ref_t), dd_table.site_absdiff_table(eng, tgt_t)

    for n_src in args.sources:
        src_t = block(n_src)

        def old():
            return eng.window_dd(eng.site_absdiff(ref_t, src_t), ref_t.n_ind, eng.site_absdiff(tgt_t, src_t), tgt_t.n_ind, lo, hi)

        def table():
            table_ref, table_tgt = tables()
            return dd_table.window_dd_table(eng, src_t, table_ref, ref_t.n_ind, table_tgt, tgt_t.n_ind, lo, hi)

        want = old()
        got, unlisted = table()
        assert int(unlisted.cpu()[0]) == 0 and torch.equal(got.view(torch.int64), want.view(torch.int64)), f"{n_src} source individuals: the routes differ"
        del want, got
        forms = {"o_site_absdiff_x2_window_dd": old, "t_tables_x2_window_dd_table": table, "t_tables_alone": tables}
        for fn in forms.values():  # warm-up: code objects, the allocator's blocks
            timed(fn)
        ms = {form: [] for form in forms}
        for _ in range(args.repeats):
            for form, fn in forms.items():
                ms[form].append(timed(fn))
        say(f"{n_src} source individuals: DD equal bit for bit on both routes")
        rec = {"n_src_ind": n_src, "forms": {}}
        for form, runs in ms.items():
            median, spread = summary(runs)
            say(f"  {form}: ms per call: " + " ".join(f"{t:.3f}" for t in runs))
            say(f"    median {median:.3f} ms (spread {spread:.3f})")
            rec["forms"][form] = {"ms": [round(t, 4) for t in runs], "median_ms": round(median, 4), "spread_ms": round(spread, 4)}
        f = rec["forms"]
        own_bytes = n * (args.ref + args.tgt) + 2 * 28 * n
        gbs = own_bytes / (f["t_tables_alone"]["median_ms"] * 1e-3) / 1e9
        rec["table_pass_gb_per_s"] = round(gbs, 1)
        say(f"  the two table passes alone: {own_bytes / 1e9:.3f} GB of their own (genotypes + 28 B per site and population) = {gbs:.0f} GB/s")
        ratio = f["t_tables_x2_window_dd_table"]["median_ms"] / f["o_site_absdiff_x2_window_dd"]["median_ms"]
        faster_in_every_run = all(t < o for t, o in zip(ms["t_tables_x2_window_dd_table"], ms["o_site_absdiff_x2_window_dd"]))
        rec["t_over_o"], rec["t_faster_in_every_run"] = round(ratio, 4), faster_in_every_run
        say(f"  (t) against (o): {f['t_tables_x2_window_dd_table']['median_ms']:.3f} ms against {f['o_site_absdiff_x2_window_dd']['median_ms']:.3f} ms = "
            f"{ratio:.3f} of the time; (t) faster in every run: {faster_in_every_run}")  # fmt: skip
        result["sources"].append(rec)
        del src_t
        torch.cuda.empty_cache()
    say("not measured: other shapes (site counts, population widths, window lengths), missing calls, the kernels under rocprofv3")
    say(json.dumps(result))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
