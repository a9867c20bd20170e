#!/usr/bin/env python3
"""Rate of `sai convert --out-pfile --ld-compress`, the kernels behind it and the fileset it writes, next to the same
conversion without the option, in one call.  Writes everything it prints to --out (profiles/pgen_ld.txt) as well.

Writes, from a seed, --rows records x --samples unphased diploid calls on chromosome 1 as plain VCF text: the LD panel of
``tests/pgen_ld_cases.py`` (blocks of near-copied rows, 10 % of the copies with 0 and 2 exchanged, 0.5 % missing calls;
synthetic, not real data; writing is not timed).  Then, with the file in the page cache, one process on one GPU:

  (1) the kernels: plan, scan and write of ``sai_pgen_encode_ld`` over the whole block, one launch each (``stages``),
      next to the three kernels of ``sai_pgen_encode``; device events, alternating, after a warm-up round;
  (2) the bytes of the records of both, the record types, and on the first --check-rows rows the assertion that the LD
      records' types and lengths are the test writer's (``tests/pgen_builder.py`` by the segment rule);
  (3) ``convert --out-pfile`` with and without ``--ld-compress`` from the same file, wall time and phases, alternating.
      The one condition: in every LD call the ``encode`` phase (all three kernels) takes no longer than the ``read``
      phase of the same call, so that the conversion stays bound by the read;
  (4) ``score`` from both filesets, warm (wall time; record only: a type 2 / 3 record expands its base first), and
      whether the two tables are the same bytes.

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
_lines = []


def say(text=""):
    print(text, flush=True)
    _lines.append(text)


def write_input(directory: Path, rows: int, samples: int, seed: int):
    """(path, names): the seeded LD panel as plain VCF text, found again when the file exists."""
    import pgen_ld_cases as LC

    path = directory / f"pgen_ld_{rows}x{samples}_{seed}.vcf"
    names = [f"s{k}" for k in range(samples)]
    if path.exists():
        return str(path), names
    rng = np.random.default_rng(seed)
    header = "##fileformat=VCFv4.2\n##contig=<ID=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    text_of = np.array([b"0/0\t", b"0/1\t", b"1/1\t", b"./.\t"], dtype="S4")  # by hard-call code
    with open(path, "wb") as out:
        out.write(header.encode())
        pos = 0
        for lo in range(0, rows, CHUNK_ROWS):  # a chunk starts a new block of the panel
            n = min(rows, lo + CHUNK_ROWS) - lo
            codes = LC.ld_panel(rng, n, samples)
            steps = rng.integers(1, 200, n)
            text = []
            for k in range(n):
                pos += int(steps[k])
                text.append(f"1\t{pos}\tv{lo + k}\tA\tC\t.\tPASS\t.\tGT\t".encode() + text_of[codes[k]].tobytes()[:-1] + b"\n")
            out.write(b"".join(text))
    return str(path), names


def kernel_figures(eng, dos, repeats):
    """(1): {step: ms per repeat}, alternating; per form the records' bytes and the tables (host arrays)."""
    import torch

    from sai_amd import _ffi
    from sai_amd.utils import pgen_writer as W

    lib = W.load_ld()
    n_rows, n_slots = dos.shape
    dense = n_rows * ((n_slots + 3) // 4)
    forms = {}
    for form, encode in (("ld", lib.sai_pgen_encode_ld), ("plain", lib.sai_pgen_encode)):
        forms[form] = dict(encode=encode, rec=torch.empty((dense,), dtype=torch.uint8, device=eng.device), vrtype=torch.empty((n_rows,), dtype=torch.uint8, device=eng.device),
                           length=torch.empty((n_rows,), dtype=torch.int32, device=eng.device), status=torch.empty((n_rows,), dtype=torch.int32, device=eng.device),
                           offsets=torch.empty((n_rows + 1,), dtype=torch.int32, device=eng.device))  # fmt: skip
    stream = torch.cuda.current_stream(eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def stage(form, bits):
        f = forms[form]
        _ffi.check(f["encode"](eng.ctx, p(dos), n_rows, n_slots, None, 2, p(f["rec"]), p(f["vrtype"]), p(f["length"]), p(f["offsets"]), p(f["status"]), bits,
                               C.c_void_p(stream.cuda_stream)))  # fmt: skip

    steps = {}
    for name, bits in (("plan", W.ENCODE_PLAN), ("scan", W.ENCODE_SCAN), ("write", W.ENCODE_WRITE)):
        for form in ("ld", "plain"):  # the forms alternate stage by stage
            steps[f"{form}_{name}"] = lambda form=form, bits=bits: stage(form, bits)
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
    out = {}
    for form, f in forms.items():
        assert not bool(f["status"].any()), "the seeded block holds a call that does not fit"
        out[form] = (int(f["offsets"][n_rows].item()) & 0xFFFFFFFF, f["vrtype"].cpu().numpy(), f["length"].cpu().numpy().view(np.uint32))
    return times, out, dense


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--samples", type=int, default=2002)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20265)
    ap.add_argument("--check-rows", type=int, default=640, help="rows whose records are sized by the test writer as well")
    ap.add_argument("--dir", default=None, help="where the input and the filesets are written (kept when given; default: a temporary directory)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pgen_ld.txt"), help="the file everything printed is written to")
    ap.add_argument("--no-score", action="store_true", help="leave (4) out")
    args = ap.parse_args()

    import tempfile

    import torch

    import __graft_entry__ as entry

    entry.build()
    import pgen_export_rate as plain_rate
    import pgen_ld_cases as LC
    from sai_amd.engine import Engine
    from sai_amd.sai import convert, score
    from sai_amd.utils import device_vcf

    stats, fmt = plain_rate.stats, plain_rate.fmt
    holder = None if args.dir else tempfile.TemporaryDirectory(prefix="pgen_ld_rate_")
    directory = Path(args.dir or holder.name)
    directory.mkdir(parents=True, exist_ok=True)
    eng = Engine.get(0)
    samples = args.samples
    result = {"rows": args.rows, "samples": samples}
    say(f"tools/pgen_ld_rate.py --rows {args.rows} --samples {samples} --repeats {args.repeats} --seed {args.seed}; {torch.cuda.get_device_name(0)}")
    t0 = time.perf_counter()
    vcf, names = write_input(directory, args.rows, samples, args.seed)
    say(f"== {args.rows} rows x {samples} samples, the synthetic LD panel: {os.path.basename(vcf)} ({os.path.getsize(vcf)} bytes), written or found in "
        f"{time.perf_counter() - t0:.1f} s (not part of any figure)")  # fmt: skip
    # (1), (2)
    pos, dos, _, _ = device_vcf.load_dosage_device(eng, vcf, "1", names, [2] * samples)
    torch.cuda.synchronize()
    assert len(pos) == args.rows
    times, forms, dense = kernel_figures(eng, dos, args.repeats)
    say(f"(1) {args.rows * samples} bytes in; device events, alternating, ms (ld: sai_pgen_encode_ld, plain: sai_pgen_encode):")
    for name in times:
        say(f"  {name:12s} {fmt(times[name])}")
    med = {name: stats(v)[0] for name, v in times.items()}
    for form in ("ld", "plain"):
        say(f"  {form}: plan + scan + write = {med[form + '_plan'] + med[form + '_scan'] + med[form + '_write']:.3f} ms")
    for form, (total, vrtype, _) in forms.items():
        kinds = np.bincount(vrtype, minlength=8)
        say(f"(2) {form:5s} records {total} bytes ({dense / total:.2f} times fewer than the dense {dense}); record types " +
            ", ".join(f"{k}: {int(c)}" for k, c in enumerate(kinds) if c))  # fmt: skip
    say(f"    plain / ld = {forms['plain'][0] / forms['ld'][0]:.3f}")
    check = min(args.check_rows, args.rows)
    block = dos[:check].cpu().numpy()
    codes = np.select([block == 0, block == 1, block == 2], [0, 1, 2], 3).astype(np.uint8)
    want_types, want_records, _ = LC.reference_of(("rate", samples), codes)
    assert forms["ld"][1][:check].tolist() == want_types and forms["ld"][2][:check].tolist() == [len(r) for r in want_records], "the kernels and the test writer disagree"
    say(f"    the first {check} rows: types and lengths are the test writer's ({sum(len(r) for r in want_records)} bytes)")
    result["kernel_ms"] = {k: [round(v, 4) for v in vs] for k, vs in times.items()}
    result["bytes"] = {form: forms[form][0] for form in forms}
    del dos
    # (3)
    runs, phases = {"ld": [], "plain": []}, {"ld": [], "plain": []}
    prefix = {kind: str(directory / f"out_{kind}") for kind in runs}
    for rep in range(args.repeats + 1):  # the first round is the warm-up
        for kind in ("ld", "plain"):
            for ext in (".pgen", ".pvar", ".psam"):
                if os.path.exists(prefix[kind] + ext):
                    os.remove(prefix[kind] + ext)
            torch.cuda.synchronize()
            t = time.perf_counter()
            summary = convert(vcf, "1", out_pfile=prefix[kind], **({"ld_compress": True} if kind == "ld" else {}))
            dt = (time.perf_counter() - t) * 1e3
            if rep:
                runs[kind].append(dt), phases[kind].append(summary["ms"])
    for kind in runs:
        say(f"(3) convert --out-pfile{' --ld-compress' if kind == 'ld' else ''}, wall ms: {fmt(runs[kind])}")
        for phase in ("read", "site_scan", "encode", "d2h", "write"):
            say(f"      {phase:10s} {fmt([s[phase] for s in phases[kind]])}")
    holds = all(s["encode"] <= s["read"] for s in phases["ld"])
    say(f"    the condition (in every LD call, encode <= read of the same call): {'holds' if holds else 'DOES NOT HOLD'}: " +
        "; ".join(f"{s['encode']:.1f} <= {s['read']:.1f}" for s in phases["ld"]))  # fmt: skip
    sizes = {kind: os.path.getsize(prefix[kind] + ".pgen") for kind in runs}
    say(f"    .pgen files: {sizes}; plain / ld = {sizes['plain'] / sizes['ld']:.3f}")
    result["convert_ms"], result["phases_ms"], result["condition_holds"], result["sizes"] = runs, phases, bool(holds), sizes
    # (4)
    if not args.no_score:
        half = (samples - 2) // 2
        groups = (("ref", "R", names[:half]), ("tgt", "T", names[half : 2 * half]), ("src", "S", names[2 * half : 2 * half + 2]))
        for group, pop, members in groups:
            (directory / f"{group}.list").write_text("".join(f"{pop}\t{s}\n" for s in members))
        uq = "    ref:\n      R: 0.3\n    tgt:\n      T: {x}\n    src:\n      S: \"=1\"\n"
        cfg = directory / "cfg.yaml"
        cfg.write_text("statistics:\n  U:\n" + uq.format(x=0.2) + "  Q:\n" + uq.format(x=0.95) + "ploidies:\n  ref:\n    R: 2\n  tgt:\n    T: 2\n  src:\n    S: 2\n"
                       "populations:\n" + "".join(f"  {g}: \"{directory}/{g}.list\"\n" for g, _, _ in groups))  # fmt: skip
        outputs, took = {}, {"ld": [], "plain": []}
        for rep in range(min(args.repeats, 5) + 1):
            for kind in ("ld", "plain"):
                out = directory / f"score_{kind}.tsv"
                torch.cuda.synchronize()
                t = time.perf_counter()
                score(vcf_file=prefix[kind] + ".pgen", chr_name="1", win_len=50000, win_step=10000, anc_allele_file=None, output_file=str(out), config=str(cfg),
                      num_workers=1, layout="int8")  # fmt: skip
                torch.cuda.synchronize()
                if rep:
                    took[kind].append((time.perf_counter() - t) * 1e3)
                outputs[kind] = out.read_bytes()
        for kind in took:
            say(f"(4) score --pfile from the {kind:5s} fileset, warm, wall ms: {fmt(took[kind])}")
            result[f"score_{kind}_ms"] = took[kind]
        say(f"    the two score tables are {'byte-identical' if outputs['ld'] == outputs['plain'] else 'DIFFERENT'}")
    say(json.dumps(result))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(_lines) + "\n")
    if holder is not None:
        holder.cleanup()
    return 0 if holds else 1


if __name__ == "__main__":
    sys.exit(main())
