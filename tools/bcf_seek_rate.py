#!/usr/bin/env python3
"""What a `.csi` index saves a region read of a BCF file, range by range, on both routes, in one call.

On the file of ``tools/bcf_rate.py`` (--rows x --samples phased diploid calls on chromosome 1, written from a seed;
writing is not timed) and an index written beside it by the tests' writer (tests/csi_builder.py, min_shift 14, depth 5),
reads --ranges consecutive position ranges of equal record count, each with the index and without it
(``SAI_AMD_BCF_INDEX=0``: the parent commit's behaviour, the yardstick), on the GPU route and on the host route of
``bcf.load_dosage_device`` in turn -- one warm-up round, then --repeats rounds, the files in the page cache, host clock
around a device synchronise -- checks that the blocks of a range are equal whichever way it was read, and prints per
route the median per range, the bytes of the file each read took, and the sums over the ranges.  Then one read of the
last range per route and way with every phase on its own.

The inputs and the index are written by this process, which never opens the GPU; the measurement runs in a child
process under its own ``timeout`` (--limit seconds).
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for entry_dir in (ROOT, ROOT / "tests", ROOT / "tools"):
    if str(entry_dir) not in sys.path:
        sys.path.insert(0, str(entry_dir))


def prepare(directory: Path, rows: int, samples: int, seed: int, n_ranges: int) -> dict:
    import bcf_rate
    import csi_builder as X

    t0 = time.perf_counter()
    _, bcf_path, names = bcf_rate.write_inputs(directory, rows, samples, seed)
    with open(bcf_path, "rb") as f:
        records = X.records_of(f.read())
    X.write_index_bytes(bcf_path, X.index_stream(records, 14, 5))
    pos = [r["pos0"] + 1 for r in records]
    cuts = [len(pos) * k // n_ranges for k in range(n_ranges + 1)]
    ranges = [(pos[cuts[k]], pos[cuts[k + 1]] - 1 if k + 1 < n_ranges else pos[-1]) for k in range(n_ranges)]
    print(f"inputs: {rows} rows x {samples} samples as {os.path.basename(bcf_path)} ({os.path.getsize(bcf_path)} bytes) and its .csi "
          f"({os.path.getsize(bcf_path + '.csi')} bytes, min_shift 14, depth 5), written or found in {time.perf_counter() - t0:.1f} s (not part of any figure)")  # fmt: skip
    return {"bcf": bcf_path, "names": names, "ranges": ranges, "rows": [cuts[k + 1] - cuts[k] for k in range(n_ranges)]}


def measure(plan: dict, repeats: int) -> int:
    import torch

    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine
    from sai_amd.utils import bcf

    eng = Engine.get(0)
    path, names, ranges = plan["bcf"], plan["names"], [tuple(r) for r in plan["ranges"]]
    ploidies, size = [2] * len(names), os.path.getsize(path)

    def read(route, indexed, k, trace):
        os.environ["SAI_AMD_GPU_INFLATE"] = "1" if route == "gpu" else "0"
        os.environ["SAI_AMD_BCF_INDEX"] = "1" if indexed else "0"
        torch.cuda.synchronize()
        t = time.perf_counter()
        pos, dos, _, _ = bcf.load_dosage_device(eng, path, "1", names, ploidies, *ranges[k], trace=trace)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert trace["route"] == ("device" if route == "gpu" else "host"), (route, trace["route"])
        assert trace["seek"]["made"] == (indexed and k > 0), (route, indexed, k, trace["seek"])
        return dt, pos, dos

    reference = [None] * len(ranges)
    times = {(route, indexed): [[] for _ in ranges] for route in ("gpu", "host") for indexed in (True, False)}
    file_bytes = {key: [0] * len(ranges) for key in times}
    for rnd in range(repeats + 1):  # round 0 warms up: page-locks the staging, loads the code objects, fills the page cache
        for k in range(len(ranges)):
            for route in ("gpu", "host"):
                for indexed in (True, False):
                    trace = {}
                    dt, pos, dos = read(route, indexed, k, trace)
                    assert len(pos) == plan["rows"][k], (route, indexed, k, len(pos))
                    if reference[k] is None:
                        reference[k] = dos
                    else:
                        assert torch.equal(dos, reference[k]), f"range {k}, {route}, index {indexed}: the block differs"
                    del dos
                    if rnd:
                        times[route, indexed][k].append(dt)
                    file_bytes[route, indexed][k] = trace["seek"]["file_bytes"]
    result = {"ranges": ranges, "file_bytes": size, "routes": {}}
    median = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for route in ("gpu", "host"):
        print(f"{route} route, ms per range (median of {repeats}; spread) and MB of the file read, with the index | without:")
        sums = {True: 0.0, False: 0.0}
        for k in range(len(ranges)):
            cells = []
            for indexed in (True, False):
                v = times[route, indexed][k]
                sums[indexed] += median(v)
                cells.append(f"{1e3 * median(v):8.1f} ({1e3 * (max(v) - min(v)):5.1f}) {file_bytes[route, indexed][k] / 1e6:7.1f} MB")
            print(f"  range {k} {ranges[k][0]:>9}-{ranges[k][1]:<9} " + " | ".join(cells))
        inflates = {i: sum(file_bytes[route, i]) / size for i in (True, False)}
        print(f"  sum over the {len(ranges)} ranges: {1e3 * sums[True]:.1f} ms with the index, {1e3 * sums[False]:.1f} ms without = {sums[False] / sums[True]:.2f} times; "
              f"the file read {inflates[True]:.2f} times with the index, {inflates[False]:.2f} times without")  # fmt: skip
        result["routes"][route] = {"with_index_ms": [round(1e3 * median(times[route, True][k]), 2) for k in range(len(ranges))],
                                   "without_ms": [round(1e3 * median(times[route, False][k]), 2) for k in range(len(ranges))],
                                   "sum_with_index_ms": round(1e3 * sums[True], 2), "sum_without_ms": round(1e3 * sums[False], 2),
                                   "file_reads_with_index": round(inflates[True], 3), "file_reads_without": round(inflates[False], 3)}  # fmt: skip
    last = len(ranges) - 1
    phases = {"gpu": ("file_read", "header_inflate", "wait_for_buffer", "h2d", "inflate_gpu", "walk_gpu", "select", "decode"),
              "host": ("file_read", "inflate", "walk", "copy_to_staging", "wait_for_buffer", "h2d", "decode")}  # fmt: skip
    for route in ("gpu", "host"):
        print(f"{route} route, the last range with every phase on its own, ms with the index | without:")
        traces = {}
        for indexed in (True, False):
            traces[indexed] = {"serial": True}
            read(route, indexed, last, traces[indexed])
        for name in phases[route]:
            print(f"  {name:16s} {1e3 * traces[True].get(name, 0.0):9.1f} | {1e3 * traces[False].get(name, 0.0):9.1f}")
    bcf.release_buffers(eng)
    print(json.dumps(result))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=2002)
    ap.add_argument("--ranges", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20262)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring child process may take")
    ap.add_argument("--dir", default=None, help="where the inputs are written (kept and reused when given; default: a temporary directory)")
    ap.add_argument("--measure", default=None, metavar="PLAN.json", help="(the child process) measure what the plan names")
    args = ap.parse_args()
    if args.measure:
        return measure(json.loads(Path(args.measure).read_text()), args.repeats)

    import tempfile

    holder = None if args.dir else tempfile.TemporaryDirectory(prefix="bcf_seek_rate_")
    directory = Path(args.dir or holder.name)
    directory.mkdir(parents=True, exist_ok=True)
    plan = prepare(directory, args.rows, args.samples, args.seed, args.ranges)
    plan_path = directory / "seek_plan.json"
    plan_path.write_text(json.dumps(plan))
    env = {k: v for k, v in os.environ.items() if k not in ("SAI_AMD_GPU_INFLATE", "SAI_AMD_BCF_INDEX", "SAI_AMD_INGEST", "SAI_AMD_INFLATE_BATCH")}
    res = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--measure", str(plan_path), "--repeats", str(args.repeats)], env=env)
    if holder is not None:
        holder.cleanup()
    return res.returncode


if __name__ == "__main__":
    sys.exit(main())
