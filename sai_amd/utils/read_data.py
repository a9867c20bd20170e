"""Load the ref / tgt / src populations of one chromosome region (mirror of sai/utils/utils.py:215-356
``read_data`` and :649-761 ``_load_population_data``).  ``read_data`` has the reference's signature and
defaults; the combination WindowGenerator asks for (window_generator.py:105-120: unphased, no
fixed-variant or missing-call filter) is served by the native tokenizers as int8 dosages
(``read_dosage_data`` on the host, ``read_data_device`` in HBM), every other combination by the
allele-level reader of ``geno.py`` (calls from the same native tokenizer, allele by allele)."""

from __future__ import annotations

import os
import warnings
from typing import Optional

import numpy as np

from .genomic_dataclasses import ChromosomeData
from .samples import parse_ind_file


def read_data(
    vcf_file: str,
    chr_name: str,
    ploidy_config,
    ref_ind_file: Optional[str],
    tgt_ind_file: Optional[str],
    src_ind_file: Optional[str],
    out_ind_file: Optional[str] = None,
    anc_allele_file: Optional[str] = None,
    start: int = None,
    end: int = None,
    is_phased: bool = True,
    filter_ref: bool = True,
    filter_tgt: bool = True,
    filter_src: bool = False,
    filter_out: bool = False,
    filter_missing: bool = True,
    engine: str = "native",
) -> dict[str, tuple[Optional[dict[str, ChromosomeData]], Optional[dict[str, list[str]]]]]:
    """{"ref": (data, samples), "tgt": ..., "src": ..., "outgroup": ...} with the reference's options
    (utils.py:215-356): ``is_phased`` = haplotype columns [sites][individuals * ploidy] instead of the
    dosage [sites][individuals]; ``filter_<group>`` = drop the variants fixed in a population;
    ``filter_missing`` = drop the sites where a sample of the population has a missing allele.  Blocks
    carry REF / ALT.  All options off and unphased is the ``score`` path's request: it goes to the native
    tokenizer (``read_dosage_data``: int8 dosages, REF / ALT not kept)."""
    from .filesets import name_of

    if not (is_phased or filter_ref or filter_tgt or filter_src or filter_out or filter_missing):
        return read_dosage_data(vcf_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file,
                                anc_allele_file, start, end, engine)  # fmt: skip
    kind = name_of(vcf_file)
    if kind is not None:
        # a fileset has neither phase nor REF / ALT columns to hand out: only the dosage request is served from it
        raise ValueError(f"{vcf_file}: {kind} is read as unphased dosages only "
                         "(is_phased=False and every filter_* option off); convert it to VCF for the other options")  # fmt: skip
    from .geno import load_population_data

    results = {}
    for group, ind_file, fixed in (("ref", ref_ind_file, filter_ref), ("tgt", tgt_ind_file, filter_tgt),
                                   ("src", src_ind_file, filter_src), ("outgroup", out_ind_file, filter_out)):  # fmt: skip
        if ind_file is None or (group == "outgroup" and group not in ploidy_config.root):  # utils.py:331-337
            results[group] = (None, None)
            continue
        results[group] = load_population_data(vcf_file, str(chr_name), ind_file, anc_allele_file, start, end, is_phased, fixed,
                                              filter_missing, ploidy_config, group, engine)  # fmt: skip
    return results


def read_dosage_data(
    vcf_file: str,
    chr_name: str,
    ploidy_config,
    ref_ind_file: Optional[str],
    tgt_ind_file: Optional[str],
    src_ind_file: Optional[str],
    out_ind_file: Optional[str] = None,
    anc_allele_file: Optional[str] = None,
    start: int = None,
    end: int = None,
    engine: str = "native",
    *,
    src_file: Optional[str] = None,
) -> dict[str, tuple[Optional[dict[str, ChromosomeData]], Optional[dict[str, list[str]]]]]:
    """``read_data(..., is_phased=False, filter_*=False, filter_missing=False)``:
    {"ref": (data, samples), "tgt": ..., "src": ..., "outgroup": (data, samples) or (None, None)}.

    ``data`` maps population -> ChromosomeData for the populations that have a ploidy entry
    (others are skipped with the reference's RuntimeWarning, utils.py:722-728); a population
    with a ploidy but no samples is a ValueError (:713-718); ``data`` is None when the region
    holds no record.  The VCF is parsed once per distinct ploidy for all groups (the reference
    re-reads it per population) by the native tokenizer of libsaihip (``engine="native"``) or by
    the Python statement of the same rules (``engine="python"``, used by the tests as the
    cross-check); REF/ALT are not kept (nothing reads them after polarisation).

    ``src_file``: the samples of the ``src`` group are read from that file, those of the other groups from ``vcf_file``,
    each by its own reader with the same ancestral alleles; the blocks hold the sites both readers kept
    (``sai_amd.site_join``), and the result carries ``"site_join"``, the join's summary.  A list or tuple of 2 to 16 paths:
    every sample of the ``src`` group comes from the one file that holds it, and the blocks hold the sites all readers kept
    (``sai_amd.site_join_many``); a sequence of one path is that path."""
    if src_file is not None:
        from ..site_join import join_host_results, require_second_input
        from ..site_join_many import is_many, read_host, source_files

        src_file = source_files(src_file)
        if is_many(src_file):
            return read_host(vcf_file, src_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file,
                             anc_allele_file, start, end, engine)  # fmt: skip

        require_second_input(src_file, anc_allele_file)
        panel = read_dosage_data(vcf_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, None, out_ind_file, anc_allele_file,
                                 start, end, engine)  # fmt: skip
        source = read_dosage_data(src_file, chr_name, ploidy_config, None, None, src_ind_file, None, anc_allele_file, start, end, engine)
        return join_host_results(panel, source, vcf_file, src_file)
    chr_name = str(chr_name)
    samples_by_group = _parse_groups(ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file)
    # one pass per distinct ploidy (normally one or two), each over the samples that need it
    by_ploidy: dict[int, list[str]] = {}
    seen: dict[int, set[str]] = {}
    for _, names, ploidy in _wanted(samples_by_group, ploidy_config):
        bucket, have = by_ploidy.setdefault(ploidy, []), seen.setdefault(ploidy, set())
        for n in names:  # first occurrence keeps its place (a sample may sit in several populations)
            if n not in have:
                have.add(n)
                bucket.append(n)
    if not any(by_ploidy.values()):
        return {"outgroup": (None, None), **{group: (None, samples) for group, samples in samples_by_group.items()}}

    loader = _load_python if engine == "python" else _load_native
    where = chr_name if start is None and end is None else f"{chr_name}:{start}-{end}"
    loaded = {}
    for ploidy, names in by_ploidy.items():
        try:
            pos, dos, n_matched, n_anc = loader(vcf_file, chr_name, names, ploidy, start, end, anc_allele_file)
        except FileNotFoundError:
            raise
        except Exception as e:  # utils.py:139-140
            raise ValueError(f"Failed to read VCF file {vcf_file} from {where}: {e}") from e
        _check_anc_found(anc_allele_file, n_matched, n_anc, chr_name, start, end)
        loaded[ploidy] = (pos, dos, {n: i for i, n in enumerate(names)}, n_matched)

    def block(population, names, ploidy):
        pos, dos, column, n_matched = loaded[ploidy]
        if n_matched == 0:  # no record in the region: the reference's "vcf_data is None" case
            return None
        cols = [column[n] for n in names]
        if cols and cols == list(range(cols[0], cols[0] + len(cols))):  # the usual case: one block of columns
            gt = np.ascontiguousarray(dos[:, cols[0] : cols[0] + len(cols)])
        else:
            gt = np.ascontiguousarray(dos[:, cols])
        return ChromosomeData(POS=pos.copy(), REF=None, ALT=None, GT=gt)

    return _assemble(samples_by_group, ploidy_config, block)


def _parse_groups(ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file) -> dict:
    """group -> {population: sample names} (None for a group without a sample file), in the order ref, tgt, src,
    outgroup; every population with a ploidy entry must be in its group's sample file."""
    groups = [("ref", ref_ind_file), ("tgt", tgt_ind_file), ("src", src_ind_file)]
    # utils.py:331-337: an outgroup file only counts when the ploidy section names outgroups
    if out_ind_file is not None and "outgroup" in ploidy_config.root:
        groups.append(("outgroup", out_ind_file))
    samples_by_group: dict[str, Optional[dict[str, list[str]]]] = {}
    for group, ind_file in groups:
        if ind_file is None:
            samples_by_group[group] = None
            continue
        samples = parse_ind_file(ind_file)
        if group not in ploidy_config.root:
            raise ValueError(f"Ploidy configuration missing group '{group}'.")
        for population in ploidy_config.root[group]:
            if population not in samples:
                raise ValueError(
                    f"Population '{population}' in ploidy_config[{group}] not found in sample file: {ind_file}"
                )
        samples_by_group[group] = samples
    return samples_by_group


def _wanted(samples_by_group, ploidy_config):
    """(population, sample names, ploidy) of every population that has a ploidy entry, in file order."""
    for group, samples in samples_by_group.items():
        for population, names in (samples or {}).items():
            if population in ploidy_config.root[group]:
                yield population, names, ploidy_config.root[group][population]


def _check_anc_found(anc_allele_file, n_matched, n_anc, chr_name, start, end) -> None:
    if anc_allele_file and n_matched and n_anc == 0:  # read_anc_allele, utils.py:480-487
        if start is not None or end is not None:
            raise ValueError(f"No ancestral allele is found for chromosome {chr_name} in the region {start}-{end}.")
        raise ValueError(f"No ancestral allele is found for chromosome {chr_name}.")


def _assemble(samples_by_group, ploidy_config, block) -> dict:
    """The readers' result: ``block(population, names, ploidy)`` gives the ChromosomeData of a population (None when
    the region holds no record); a population without a ploidy entry is skipped with the reference's RuntimeWarning."""
    results: dict = {"outgroup": (None, None)}
    for group, samples in samples_by_group.items():
        if samples is None:
            results[group] = (None, None)
            continue
        data: dict[str, ChromosomeData] = {}
        for population, names in samples.items():
            if population not in ploidy_config.root[group]:
                warnings.warn(
                    f"Population '{population}' found in sample file but not in ploidy_config[{group}]; skipping.",
                    RuntimeWarning,
                )
                continue
            got = block(population, names, ploidy_config.root[group][population])
            if got is not None:
                data[population] = got
        results[group] = (data if data else None, samples)
    return results


def read_data_device(eng, vcf_file: str, chr_name: str, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file,
                     out_ind_file=None, anc_allele_file=None, start: int = None, end: int = None, layout: str = "int8", *,
                     src_file: Optional[str] = None):
    """``read_data`` with the genotypes left in HBM: one streaming pass over the file (text over PCIe,
    tokenised on the GPU, ``device_vcf.load_dosage_device``) for all populations and ploidies, then one
    re-tiling launch per population straight from the shared [record][sample] block.  Returns
    ``(results, pos_dev)``: ``results`` as ``read_data`` gives it, except that every ``GT`` is a
    ``TiledPop``; ``pos_dev`` = the int32 device copy of the positions (None without data).  A PLINK 1
    fileset takes the same way with its own reader (``plink.load_dosage_device``: ``.bed`` rows over PCIe,
    decoded on the GPU), and so does an EIGENSOFT one (``eigenstrat.load_dosage_device``); there a slot is a
    (sample, ploidy) request, so one pass always serves all.

    ``layout="packed2"`` (a PLINK 1 or a PLINK 2 fileset): every ``GT`` is a ``PackedPop``, decoded from the ``.bed``
    rows or the ``.pgen`` records straight into the 2-bit layout (the reader's ``load_packed_device``); no int8 block
    is built on the way.

    ``src_file`` (int8 layout): the samples of the ``src`` group are read from that file, those of the other groups from
    ``vcf_file``, each by its own reader with the same region and ancestral alleles; the positions are joined on the host
    (``site_join.join_host``) and every population of both inputs is tiled from the rows of the common sites by one
    launch that gathers while it re-tiles (``site_join_device.RowTiler``).  All blocks share one ``POS``, the common
    positions, and the result carries ``"site_join"``, as ``read_dosage_data(..., src_file=)``'s does.  A list or tuple of 2 to
    16 paths: as there, and a population whose samples lie in more than one file is tiled from all of them by one launch
    (``site_join_parts.tile_parts``)."""
    import torch

    from .filesets import reader_for

    if src_file is not None:
        from ..site_join import require_second_input
        from ..site_join_many import as_list, is_many, read_device, source_files

        src_file = source_files(src_file)
        require_second_input(as_list(src_file)[0], anc_allele_file)
        if layout == "packed2":
            raise ValueError("a source file of its own is read in the int8 layout: `src_file` cannot be combined with layout 'packed2'.")
        if layout != "int8":
            raise ValueError("layout must be 'int8' or 'packed2'")
        if is_many(src_file):
            return read_device(eng, vcf_file, src_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file,
                               anc_allele_file, start, end)  # fmt: skip
        return _read_joined_device(eng, vcf_file, src_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file,
                                   anc_allele_file, start, end)  # fmt: skip
    reader = reader_for(vcf_file)
    if layout == "packed2":
        return _read_packed_device(eng, reader, vcf_file, str(chr_name), ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file,
                                   out_ind_file, anc_allele_file, start, end)  # fmt: skip
    if layout != "int8":
        raise ValueError("layout must be 'int8' or 'packed2'")
    samples_by_group, column, blocks, pos, n_matched = _read_blocks_device(eng, reader, vcf_file, chr_name, ploidy_config, ref_ind_file,
                                                                          tgt_ind_file, src_ind_file, out_ind_file, anc_allele_file,
                                                                          start, end)  # fmt: skip
    if column is None:
        return {"outgroup": (None, None), **{group: (None, samples) for group, samples in samples_by_group.items()}}, None

    def block(population, pop_names, ploidy):
        if n_matched == 0:
            return None
        where_cols = [column[(nme, ploidy)] for nme in pop_names]
        used = {k for k, _ in where_cols}
        if len(used) == 1:
            tiled = eng.tile_columns(blocks[used.pop()], [c for _, c in where_cols])
        else:  # the population's samples were tokenised in different passes: gather its columns first
            tiled = eng._tile_device(torch.stack([blocks[k][:, c] for k, c in where_cols], dim=1).contiguous())
        return ChromosomeData(POS=pos, REF=None, ALT=None, GT=tiled)

    pos_dev = torch.from_numpy(pos).to(eng.device) if n_matched else None
    return _assemble(samples_by_group, ploidy_config, block), pos_dev


def _read_blocks_device(eng, reader, vcf_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file,
                        anc_allele_file, start, end, samples_by_group=None):
    """What ``read_data_device`` has before it tiles: ``(samples_by_group, column, blocks, pos, n_matched)`` -- the
    samples of every group, (sample, ploidy) -> (pass, column of the pass's block), the int8 [record][sample] device
    block of every pass, the positions the reader kept and the records it met.  ``column`` is None (and nothing was
    read) when no population with a ploidy entry names a sample.  ``samples_by_group``: the samples to read, in place of the
    sample files (one source file's share of the ``src`` list)."""
    fileset = reader is not None
    if fileset:
        load_dosage_device = reader.load_dosage_device
    else:
        from .device_vcf import load_dosage_device

    chr_name = str(chr_name)
    if samples_by_group is None:
        samples_by_group = _parse_groups(ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file)
    # One streaming pass maps a VCF column to ONE output slot, so a sample that sits in populations of
    # different ploidy (the reference reads every population on its own, with its own ploidy:
    # utils.py:123-138) is tokenised in a further pass: passes[k] holds each sample at most once.
    column, passes = {}, []
    for _, pop_names, ploidy in _wanted(samples_by_group, ploidy_config):
        for nme in pop_names:  # one output column per (sample, ploidy): the first occurrence keeps its place
            if (nme, ploidy) not in column:
                k = 0 if fileset and passes else next((i for i, p in enumerate(passes) if nme not in p["seen"]), len(passes))
                if k == len(passes):
                    passes.append({"names": [], "ploidies": [], "seen": set()})
                column[(nme, ploidy)] = (k, len(passes[k]["names"]))
                passes[k]["names"].append(nme)
                passes[k]["ploidies"].append(ploidy)
                passes[k]["seen"].add(nme)
    if not passes:
        return samples_by_group, None, [], None, 0
    where = chr_name if start is None and end is None else f"{chr_name}:{start}-{end}"
    if not fileset and not os.path.exists(vcf_file):
        raise ValueError(f"Failed to read VCF file {vcf_file} from {where}: cannot open VCF {vcf_file}")
    try:
        blocks = []
        for p in passes:  # one pass unless a sample is read at two ploidies
            pos, dos, n_matched, n_anc = load_dosage_device(eng, vcf_file, chr_name, p["names"], p["ploidies"], start, end,
                                                            anc_allele_file)  # fmt: skip
            blocks.append(dos)
    except FileNotFoundError:
        raise
    except Exception as e:  # utils.py:139-140
        raise ValueError(f"Failed to read VCF file {vcf_file} from {where}: {e}") from e
    _check_anc_found(anc_allele_file, n_matched, n_anc, chr_name, start, end)
    return samples_by_group, column, blocks, pos, n_matched


def _read_joined_device(eng, vcf_file, src_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file,
                        anc_allele_file, start, end):
    """``read_data_device(..., src_file=)``: the panel's blocks and the source file's, each read as a one-input call
    reads them, then the host join of their positions and one gathering re-tile per population."""
    import torch

    from .. import site_join
    from ..site_join_device import RowTiler, upload_rows
    from .filesets import reader_for

    sides = [_read_blocks_device(eng, reader_for(f), f, chr_name, ploidy_config, *lists, anc_allele_file, start, end)
             for f, lists in ((vcf_file, (ref_ind_file, tgt_ind_file, None, out_ind_file)), (src_file, (None, None, src_ind_file, None)))]  # fmt: skip

    def merged(block_of_side):
        """ref, tgt and outgroup of the panel and src of the source file as one result (``site_join._merged``)."""
        out = {}
        for side, (samples_by_group, *_), block in zip((0, 1), sides, block_of_side):
            got = _assemble(samples_by_group, ploidy_config, block)
            for group in site_join.GROUPS:
                if (group == "src") == (side == 1):
                    out[group] = got.get(group, (None, None))
        return out

    no_data = lambda population, pop_names, ploidy: None  # noqa: E731
    if any(column is None or n_matched == 0 for _, column, _, _, n_matched in sides):  # a region without a record in one of the inputs
        return merged((no_data, no_data)), None
    pos_a, pos_b = sides[0][3], sides[1][3]
    rows_a, rows_b, info = site_join.join_host(pos_a, pos_b)
    site_join._check_info(info, pos_a, pos_b, vcf_file, src_file)
    summary = site_join._summary(info, pos_a.size, pos_b.size, vcf_file, src_file)
    if summary["n_common"] == 0:
        out = merged((no_data, no_data))
        out["site_join"] = summary
        return out, None
    pos = np.ascontiguousarray(pos_a).copy() if summary["panel_identity"] else np.ascontiguousarray(pos_a[rows_a])
    tiler = RowTiler(eng)

    def tiling(side, identity, rows):
        _, column, blocks, _, _ = sides[side]
        rows_dev = None if identity else upload_rows(eng, rows)  # one upload per input; the identity passes no list

        def block(population, pop_names, ploidy):
            where_cols = [column[(nme, ploidy)] for nme in pop_names]
            used, cols = {k for k, _ in where_cols}, [c for _, c in where_cols]
            if len(used) == 1 and cols == list(range(cols[0], cols[0] + len(cols))):  # the usual case: one run of columns
                source, col0 = blocks[used.pop()], cols[0]
            elif cols:  # gathered by columns first, as the one-input read does
                source, col0 = torch.stack([blocks[k][:, c] for k, c in where_cols], dim=1).contiguous(), 0
            else:
                source, col0 = blocks[0][:, :0], 0
            return ChromosomeData(POS=pos, REF=None, ALT=None, GT=tiler.tile(source, col0, len(cols), rows_dev))

        return block

    out = merged((tiling(0, summary["panel_identity"], rows_a), tiling(1, summary["source_identity"], rows_b)))
    tiler.check()
    out["site_join"] = summary
    return out, torch.from_numpy(pos).to(eng.device)


def _read_packed_device(eng, reader, vcf_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file,
                        anc_allele_file, start, end):
    """``read_data_device(..., layout="packed2")``: one pass over the ``.bed`` or the ``.pgen`` with the reader's
    ``load_packed_device``, one packed2 block per population."""
    import torch

    from . import pgen, plink

    if reader is not plink and reader is not pgen:
        raise ValueError(f"{vcf_file}: the packed2 layout is read from a PLINK 1 fileset (.bed + .bim + .fam) or a PLINK 2 fileset "
                         "(.pgen + .pvar + .psam) only")  # fmt: skip
    samples_by_group = _parse_groups(ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file)
    wanted = list(_wanted(samples_by_group, ploidy_config))
    if not any(names for _, names, _ in wanted):
        return {"outgroup": (None, None), **{group: (None, samples) for group, samples in samples_by_group.items()}}, None
    where = chr_name if start is None and end is None else f"{chr_name}:{start}-{end}"
    try:
        pos, packed, n_matched, n_anc = reader.load_packed_device(eng, vcf_file, chr_name, [(names, ploidy) for _, names, ploidy in wanted],
                                                                  start, end, anc_allele_file)  # fmt: skip
    except FileNotFoundError:
        raise
    except Exception as e:  # utils.py:139-140
        raise ValueError(f"Failed to read VCF file {vcf_file} from {where}: {e}") from e
    _check_anc_found(anc_allele_file, n_matched, n_anc, chr_name, start, end)
    in_order = iter(packed)  # _assemble asks for the populations in the order _wanted names them

    def block(population, pop_names, ploidy):
        pop = next(in_order)
        return ChromosomeData(POS=pos, REF=None, ALT=None, GT=pop) if n_matched else None

    pos_dev = torch.from_numpy(pos).to(eng.device) if n_matched else None
    return _assemble(samples_by_group, ploidy_config, block), pos_dev


def _load_native(vcf_file, chr_name, names, ploidy, start, end, anc_allele_file):
    """libsaihip's multithreaded tokenizer (sai_amd/csrc/vcf_ingest.cpp), or its fileset reader
    (sai_amd/csrc/plink, sai_amd/csrc/eigenstrat) when the path names a PLINK 1 or an EIGENSOFT fileset."""
    from .filesets import reader_for
    from .native_vcf import load_dosage

    reader = reader_for(vcf_file)
    if reader is not None:
        return reader.load_dosage(vcf_file, chr_name, names, [ploidy] * len(names), start, end, anc_allele_file)
    if not os.path.exists(vcf_file):
        raise ValueError(f"cannot open VCF {vcf_file}")
    return load_dosage(vcf_file, chr_name, names, [ploidy] * len(names), start, end, anc_allele_file)


def _load_python(vcf_file, chr_name, names, ploidy, start, end, anc_allele_file):
    """The readable statement of the same rules (sai_amd/utils/vcf.py); tests compare the two."""
    from .vcf import dosage_matrices, polarisation_masks, read_anc_allele, read_region

    region = read_region(vcf_file, chr_name, names, start, end)
    dos, fdos = dosage_matrices(region, list(range(len(names))), ploidy)
    pos, n_matched, n_anc = region.pos, len(region), 0
    if anc_allele_file and len(region):
        try:
            anc = read_anc_allele(anc_allele_file, chr_name, start, end)
        except ValueError:
            anc = {}
        table = anc.get(chr_name, {})
        n_anc = len(table)
        keep, flip = polarisation_masks(region, table)
        dos[flip] = fdos[flip]
        dos, pos = dos[keep], pos[keep]
    return pos, dos, n_matched, n_anc
