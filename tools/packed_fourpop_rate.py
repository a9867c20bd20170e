#!/usr/bin/env python3
"""Rate of the site half of fd / df / Danc / Dplus in the 2-bit layout: the frequency kernel
(``sai_packed2_site_freqs``, one launch) next to the two launches it replaces (``sai_site_pass_packed2`` with counts,
then ``sai_site_freqs``), on the same blocks in the same call.

One process.  From a seed: packed2 blocks of --sizes individuals (default: 1 000 / 1 000 / 2 / 100 -- ref, tgt, one
source, an outgroup) over --sites sites (default 2^20), any codes, the fields of padding individuals 0.  The two routes'
frequencies are asserted equal bit for bit first.  Then, after a warm-up of both, --repeats timed runs of each,
alternating; a run is --inner back-to-back calls between two device events (one call is a fraction of a millisecond),
reported per call.  Bytes per site are the algorithm's: the packed genotypes once, plus 8 B of frequency per
population for the kernel, plus 8 B of counts per population written and read back for the two launches.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def tile_words(n_ind: int) -> int:
    return (n_ind // 64) * 256 + ((n_ind % 64 + 15) // 16) * 64


def random_block(rng, n_sites: int, n_ind: int) -> np.ndarray:
    """Any words are a packed2 block as long as the fields of the padding individuals are 0."""
    n_full, rem = n_ind // 64, n_ind % 64
    w_tail = (rem + 15) // 16
    words = rng.integers(0, 1 << 32, size=(-(-n_sites // 64), tile_words(n_ind)), dtype=np.uint32)
    tail = words[:, n_full * 256 :].reshape(len(words), 64, w_tail)
    for j in range(w_tail):
        if rem - 16 * j < 16:
            tail[:, :, j] &= np.uint32((1 << (2 * (rem - 16 * j))) - 1)
    return words.reshape(-1).view(np.uint8)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sites", type=int, default=1 << 20)
    ap.add_argument("--sizes", default="1000,1000,2,100", help="individuals per population, comma-separated (at most 8)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100, help="calls per timed run")
    ap.add_argument("--seed", type=int, default=20263)
    args = ap.parse_args()

    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine, PackedPop
    from sai_amd.packed_stats import packed_site_freqs

    sizes = [int(v) for v in args.sizes.split(",")]
    if not 1 <= len(sizes) <= 8 or args.repeats < 5:
        ap.error("1..8 populations (the two launches take no more) and at least 5 repeats")
    eng = Engine.get(0)
    rng = np.random.default_rng(args.seed)
    n_sites, ploidies = args.sites, [2] * len(sizes)
    pops = [PackedPop(torch.from_numpy(random_block(rng, n_sites, n)).to(eng.device), n_sites, n) for n in sizes]
    packed_bytes = sum(tile_words(n) * 4 // 64 for n in sizes)
    bytes_per_site = {"kernel": packed_bytes + 8 * len(sizes), "two_launches": packed_bytes + 3 * 8 * len(sizes)}
    counts = torch.empty((len(sizes), n_sites, 2), dtype=torch.int32, device=eng.device)

    def kernel():
        return packed_site_freqs(eng, pops, ploidies)

    def two_launches():
        eng.site_pass_packed2(pops, ploidies, [], counts=counts)
        return eng.site_freqs(counts, ploidies)

    routes = {"kernel": kernel, "two_launches": two_launches}
    a, b = kernel(), two_launches()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "the two routes' frequencies differ"
    n_nan = int(torch.isnan(a).sum())
    del a, b
    print(f"shape: {n_sites} sites x {' / '.join(map(str, sizes))} individuals; packed genotypes {packed_bytes} B per site; "
          f"kernel {bytes_per_site['kernel']} B per site, two launches {bytes_per_site['two_launches']} B per site "
          f"(ratio {bytes_per_site['kernel'] / bytes_per_site['two_launches']:.2f}); frequencies equal bit for bit ({n_nan} NaN)")  # fmt: skip

    def timed(fn) -> float:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.inner):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.inner  # ms per call

    for fn in routes.values():  # warm-up: code objects, the allocator's blocks
        timed(fn)
    ms = {name: [] for name in routes}
    for _ in range(args.repeats):
        for name, fn in routes.items():
            ms[name].append(timed(fn))
    result = {"sites": n_sites, "sizes": sizes, "inner": args.inner, "bytes_per_site": bytes_per_site, "routes": {}}
    for name, runs in ms.items():
        median, spread = sorted(runs)[len(runs) // 2], max(runs) - min(runs)
        gbs = bytes_per_site[name] * n_sites / (median * 1e-3) / 1e9
        print(f"{name}: ms per call, {args.inner} calls per run: " + " ".join(f"{t:.4f}" for t in runs))
        print(f"  median {median:.4f} ms (spread {spread:.4f}) = {gbs:.0f} GB/s of its {bytes_per_site[name]} B per site")
        result["routes"][name] = {"ms": [round(t, 5) for t in runs], "median_ms": round(median, 5), "spread_ms": round(spread, 5), "gb_per_s": round(gbs, 1)}
    k, t = result["routes"]["kernel"], result["routes"]["two_launches"]
    margin = max(k["spread_ms"], t["spread_ms"])
    result["kernel_over_two_launches"] = round(k["median_ms"] / t["median_ms"], 4)
    result["gate_passed"] = k["median_ms"] <= t["median_ms"] + margin
    print(f"kernel / two launches: {result['kernel_over_two_launches']:.3f} of the time (expected from the bytes: "
          f"{bytes_per_site['kernel'] / bytes_per_site['two_launches']:.2f}); gate (kernel median <= two-launch median + "
          f"{margin:.4f} ms, the larger spread): {'passed' if result['gate_passed'] else 'FAILED'}")  # fmt: skip
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
