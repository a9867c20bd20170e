#!/usr/bin/env python3
"""Rate of the PLINK 2 fileset route, phase by phase, next to the PLINK 1 route on the same genotypes.

Writes, from a seed, --rows x --samples genotypes on chromosome 1 whose alternative-allele frequencies follow a
1 / x spectrum (most variants rare, as in a sequenced panel; 0.5 % missing calls), once as PREFIX.bed / .bim / .fam
and once as PREFIX.pgen / .pvar / .psam with the smallest encoding per record (tests/pgen_builder.py: pure Python,
so keep --rows modest; writing is not timed and is skipped when the files exist -- ``--write-only`` stops there,
which needs no GPU).  Then, for both filesets,

  * reads chromosome 1 with ``load_dosage_device`` --repeats times after one warm-up, overlapped as `score` reads
    it (host clock around a device synchronise), and checks that the two blocks are equal;
  * reads it once more with every phase synchronised on its own: index, file read, H2D, decode.

The decode kernel's own rate comes from ``rocprofv3 --kernel-trace --stats -- python tools/pgen_rate.py ...``.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for entry in (str(ROOT), str(ROOT / "tests")):
    if entry not in sys.path:
        sys.path.insert(0, entry)


def write_inputs(directory: Path, rows: int, samples: int, seed: int) -> str:
    import pgen_builder as B

    prefix = str(directory / f"rate_{rows}x{samples}_{seed}")
    if all(os.path.exists(prefix + ext) for ext in (".bed", ".bim", ".fam", ".pgen", ".pvar", ".psam")):
        return prefix
    rng = np.random.default_rng(seed)
    freq = np.exp(rng.uniform(np.log(0.5 / samples), np.log(0.5), size=rows))  # density 1 / x
    codes = rng.binomial(2, freq[:, None], size=(rows, samples)).astype(np.uint8)  # 0 hom REF, 1 het, 2 hom ALT
    codes[rng.random(codes.shape) < 0.005] = 3
    names = [f"s{i}" for i in range(samples)]
    positions = np.cumsum(rng.integers(1, 200, size=rows)).tolist()
    to_bed = np.array([3, 2, 0, 1], dtype=np.uint8)[codes]  # PLINK 1: 0 A1 A1 (ALT ALT), 1 missing, 2 het, 3 A2 A2
    padded = np.zeros((rows, -(-samples // 4) * 4), dtype=np.uint8)
    padded[:, :samples] = to_bed
    quads = padded.reshape(rows, -1, 4)
    with open(prefix + ".bed", "wb") as f:
        f.write(b"\x6c\x1b\x01" + (quads[:, :, 0] | quads[:, :, 1] << 2 | quads[:, :, 2] << 4 | quads[:, :, 3] << 6).astype(np.uint8).tobytes())
    with open(prefix + ".bim", "w") as f:
        f.writelines(f"1\tv{k}\t0\t{positions[k]}\tC\tA\n" for k in range(rows))
    with open(prefix + ".fam", "w") as f:
        f.writelines(f"f{i} {n} 0 0 0 -9\n" for i, n in enumerate(names))
    table = B.write_fileset(prefix, ["1"] * rows, positions, [f"v{k}" for k in range(rows)], ["A"] * rows, ["C"] * rows, codes, names, len_bytes=2)
    kinds = np.bincount([t[2] & 7 for t in table], minlength=8)
    print(json.dumps({"written": prefix, "record_types": {str(k): int(c) for k, c in enumerate(kinds) if c}}))
    return prefix


def measure(reader, eng, source, names, repeats: int, bytes_key: str) -> dict:
    import torch

    ploidies = [2] * len(names)
    times = []
    for k in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pos, dos, _, _ = reader.load_dosage_device(eng, source, "1", names, ploidies)
        torch.cuda.synchronize()
        if k:
            times.append(time.perf_counter() - t0)
    trace = {"serial": True}
    reader.load_dosage_device(eng, source, "1", names, ploidies, trace=trace)
    torch.cuda.synchronize()
    genotypes = dos.numel()
    out = {"ms_median": 1e3 * statistics.median(times), "ms_min": 1e3 * min(times), "ms_max": 1e3 * max(times),
           "file_bytes": int(trace[bytes_key]), "genotypes": genotypes, "G_genotypes_per_s": genotypes / statistics.median(times) / 1e9}  # fmt: skip
    out.update({f"{phase}_ms": 1e3 * trace[phase] for phase in ("index", "file_read", "h2d", "decode")})
    return out, dos


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", required=True)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--samples", type=int, default=2002)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--write-only", action="store_true")
    args = ap.parse_args()
    directory = Path(args.dir)
    directory.mkdir(parents=True, exist_ok=True)
    prefix = write_inputs(directory, args.rows, args.samples, args.seed)
    sizes = {ext: os.path.getsize(prefix + ext) for ext in (".bed", ".pgen")}
    print(json.dumps({"bed_bytes": sizes[".bed"], "pgen_bytes": sizes[".pgen"], "ratio": sizes[".bed"] / sizes[".pgen"]}))
    if args.write_only:
        return
    import __graft_entry__ as entry

    entry.build()
    from sai_amd.engine import Engine
    from sai_amd.utils import pgen, plink

    eng = Engine.get(0)
    names = [f"s{i}" for i in range(args.samples)]
    bed, bed_block = measure(plink, eng, prefix + ".bed", names, args.repeats, "bed_bytes")
    new, pgen_block = measure(pgen, eng, prefix + ".pgen", names, args.repeats, "pgen_bytes")
    assert bool((bed_block == pgen_block).all()), "the two routes disagree"
    print(json.dumps({"bed": bed}))
    print(json.dumps({"pgen": new}))
    print(json.dumps({"pgen_over_bed_genotypes_per_s": new["G_genotypes_per_s"] / bed["G_genotypes_per_s"]}))


if __name__ == "__main__":
    main()
