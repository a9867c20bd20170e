"""The cases of several source files (DESIGN_INGEST.md, "Several source files"), shared by the CPU and the GPU tests: the
fixture tests/data/test.with.outgroup.vcf.gz with four of its samples as two source populations, cut into a panel and 2
or 3 source files in mixed formats, and the one VCF of the common sites that every result is compared with.

The fixture has one source sample, so three samples of its ``tgt`` list are taken as sources too:
    NEA = src_i1, tgt_i502, tgt_i501   -- spans the files of every cut, and not in the files' order
    DEN = tgt_i503                     -- lies in one file
    cut 2:  A = {src_i1, tgt_i502} as BCF,      B = {tgt_i501, tgt_i503} as text .geno
    cut 3:  A = {src_i1} as bgzip VCF,          B = {tgt_i501, tgt_i503} as .bed,      C = {tgt_i502} as packed .geno
Every file has sites of its own removed and sites of its own added; A has REF / ALT swapped and its calls recoded in
every fifth record; B writes homozygous-reference rows whose REF is the ancestral allele with ALT = "."."""

import numpy as np

import site_join_cases as K

NEA, DEN = ["src_i1", "tgt_i502", "tgt_i501"], ["tgt_i503"]
SOURCES = ["src_i1", "tgt_i501", "tgt_i502", "tgt_i503"]
CUTS = {
    2: [("bcf", ["src_i1", "tgt_i502"]), ("geno-text", ["tgt_i501", "tgt_i503"])],
    3: [("vcf.gz", ["src_i1"]), ("bed", ["tgt_i501", "tgt_i503"]), ("geno-packed", ["tgt_i502"])],
}
OWN_SITES = ((60, 7001, 30001, 39995), (70, 8001, 31001), (80, 9001, 32001))
REGION = dict(start=5000, end=30000)


def _absent(k, f):
    """Record k is absent from file f: another residue class for every file."""
    return k % (7 + 2 * f) == 3 + f


def write_inputs(tmp):
    """The panel, the ancestral alleles, the sample lists, the configuration, and per cut the records of every source
    file and the common VCF.  Returns {"panel", "anc", "config", "lists", "sources": {cut: [...]}, "common": {cut: path},
    "n_common": {cut: n}, "n_fixture"}."""
    meta, columns, records = K._records()
    anc_lines = open(K.ANC).read().splitlines()
    ancestral = {int(ln.split("\t")[2]): ln.split("\t")[3] for ln in anc_lines}
    taken = {int(r[1]) for r in records}
    at = {name: columns.index(name) for name in SOURCES}
    keep = [i for i in range(len(columns)) if i not in at.values()]
    extra = lambda pos, n: ["1", str(pos), ".", "A", "T", "1000", "PASS", ".", "GT", *(["1|1"] * n)]  # noqa: E731
    own_panel = [p for p in (50, 5001, 20001, 39990) if p not in taken]
    by_pos = lambda rows: sorted(rows, key=lambda r: int(r[1]))  # noqa: E731
    panel = [[r[i] for i in keep] for r in records] + [extra(p, len(keep) - 9) for p in own_panel]
    out = {"panel": str(tmp / "panel.vcf"), "anc": str(tmp / "anc.bed"), "sources": {}, "common": {}, "n_common": {}, "n_fixture": len(records)}
    open(out["panel"], "w").write(K._vcf_text(meta, [columns[i] for i in keep], by_pos(panel)))
    own = [p for f in range(3) for p in OWN_SITES[f] if p not in taken]
    assert len(own) == sum(map(len, OWN_SITES))
    anc_lines += [f"1\t{p - 1}\t{p}\tA" for p in own_panel + own]
    open(out["anc"], "w").write("\n".join(sorted(anc_lines, key=lambda ln: int(ln.split("\t")[2]))) + "\n")
    for cut, files in CUTS.items():
        specs = []
        for f, (fmt, names) in enumerate(files):
            rows, no_alt = [], 0
            for k, r in enumerate(records):
                if _absent(k, f):
                    continue
                calls = [r[at[n]] for n in names]
                row = r[:9] + calls
                if f == 0 and k % 5 == 1:
                    row[3], row[4], row[9:] = r[4], r[3], [K._swap(c) for c in calls]
                elif f == 1 and k % 4 == 0 and all(c in ("0/0", "0|0") for c in calls) and ancestral[int(r[1])] == r[3]:
                    row[4] = "."  # kept with dosage 0: the ancestral allele is its REF
                    no_alt += 1
                rows.append(row)
            rows += [extra(p, len(names)) for p in OWN_SITES[f]]
            assert f != 1 or no_alt >= 5
            specs.append({"fmt": fmt, "names": names, "meta": meta, "columns": columns[:9] + names, "records": by_pos(rows)})
        common = [r for k, r in enumerate(records) if not any(_absent(k, f) for f in range(len(files)))]
        out["sources"][cut] = specs
        out["common"][cut] = str(tmp / f"common{cut}.vcf")
        out["n_common"][cut] = len(common)
        open(out["common"][cut], "w").write(K._vcf_text(meta, columns, common))
    # the sample lists: the fixture's, with the three borrowed samples moved from tgt to src
    fixture = {g: K.DATA / f"test.with.outgroup.{g}.list" for g in ("ref", "tgt", "src", "out")}
    lists = {"ref": str(fixture["ref"]), "outgroup": str(fixture["out"]), "tgt": str(tmp / "tgt.list"), "src": str(tmp / "src.list")}
    tgt = [ln for ln in open(fixture["tgt"]).read().splitlines() if ln.split() and ln.split()[1] not in SOURCES]
    open(lists["tgt"], "w").write("\n".join(tgt) + "\n")
    open(lists["src"], "w").write("".join(f"NEA\t{n}\n" for n in NEA) + "".join(f"DEN\t{n}\n" for n in DEN))
    out["lists"] = lists
    out["config"] = str(tmp / "config.yaml")
    open(out["config"], "w").write(config_text(lists, "statistics:\n  fd: True\n  df: True\n  Danc: True\n  Dplus: True\n"))
    return out


def config_text(lists, statistics):
    return (statistics + "\nploidies:\n  ref:\n    ref: 2\n  tgt:\n    tgt: 2\n  src:\n    NEA: 2\n    DEN: 2\n  outgroup:\n    out: 2\n\n"
            "populations:\n" + "".join(f'  {g}: "{lists[g]}"\n' for g in ("ref", "tgt", "src", "outgroup")))  # fmt: skip


def write_sources(inputs, cut, tmp):
    """The source files of a cut, each in its format; returns the paths ``score`` takes, in the cut's order."""
    import bcf_builder
    from test_eigenstrat_cpu import write_eigenstrat
    from test_plink_cpu import write_fileset

    paths = []
    for f, src in enumerate(inputs["sources"][cut]):
        fmt, names, recs = src["fmt"], src["names"], src["records"]
        text = K._vcf_text(src["meta"], src["columns"], recs)
        stem = tmp / f"cut{cut}_{'ABC'[f]}"
        if fmt == "vcf.gz":
            path = str(stem) + ".vcf.gz"
            open(path, "wb").write(b"".join(bcf_builder.bgzf_members(text.encode())))
        elif fmt == "bcf":
            path = bcf_builder.write_bcf(str(stem) + ".bcf", text)
        else:
            chroms, positions, ids = [r[0] for r in recs], [int(r[1]) for r in recs], [f"v{k}" for k in range(len(recs))]
            ref, alt = [r[3] for r in recs], [r[4] for r in recs]
            n_alt = np.array([[sum(c == "1" for c in call) for call in r[9:]] for r in recs], dtype=np.uint8)  # copies of ALT: 0, 1 or 2
            if fmt == "bed":
                write_fileset(str(stem), chroms, positions, ids, alt, ref, np.array([3, 2, 0], dtype=np.uint8)[n_alt], names)
                path = str(stem) + ".bed"
            else:
                write_eigenstrat(str(stem), fmt.split("-")[1], chroms, positions, ids, ref, alt, 2 - n_alt, names)
                path = str(stem) + ".geno"
        paths.append(str(path))
    return paths


def reader_arguments(inputs):
    """(cfg, [ref, tgt, src, outgroup sample files]) of the cases' configuration."""
    from sai_amd.sai import load_config

    cfg = load_config(inputs["config"])
    return cfg, [cfg.populations.get_population(g) for g in ("ref", "tgt", "src", "outgroup")]
