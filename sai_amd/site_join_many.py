"""Sources from several files of their own (DESIGN_INGEST.md, "Several source files"): one all-sites VCF per archaic
individual, or a small fileset per lab, next to the panel.  Every input is read by its own reader with the same
ancestral alleles, region and chromosome; a site is kept when the panel's reader and every source file's reader keep it
(``sai_site_join_many_host``, one k-pointer merge on the host); the individuals of a source population stand in the
order of the ``src`` sample list, whichever file holds them.  The host readers apply the rows with numpy; the resident
reader uploads each file's row list once and tiles a population that lies in one file as the one-file route does
(``RowTiler.tile``), one whose samples lie in more than one block with ``sai_tile_rows_from_parts`` -- one launch that
gathers every part by its own list (``sai_amd.site_join_parts``).

One source file -- a ``str``, or a sequence of one path -- is the route of ``sai_amd.site_join``, unchanged.
"""

from __future__ import annotations

import ctypes as C
import importlib
import logging
import os

import numpy as np

from . import _ffi, site_join
from ._binding import extension

log = logging.getLogger("sai_amd.site_join")

SAI_JOIN_MANY_ABI_VERSION = 1
MAX_SOURCE_FILES = 16

_p, _i32 = C.c_void_p, C.c_int32

# name -> (restype, argtypes): the names sai_amd/csrc/join/site_join_many_host.cpp declares
SIGNATURES = {
    "sai_join_many_abi_version": (C.c_int, []),
    "sai_site_join_many_host": (C.c_int, [_i32, _p, _p, _p, _p]),
}
HOST_SYMBOLS = tuple(SIGNATURES)  # host code only

load, load_host = extension("k-way join", "sai_amd/csrc/join/site_join_many_host.cpp", "sai_join_many_abi_version", SAI_JOIN_MANY_ABI_VERSION,
                            SIGNATURES, HOST_SYMBOLS, built_from="join/site_join_many_host.cpp")  # fmt: skip


def source_files(src_file):
    """``src_file`` as the readers take it: None, the ``str`` of one file (a sequence of one path is that path), or the
    list of 2 to 16 different paths."""
    if src_file is None or isinstance(src_file, (str, os.PathLike)):
        return None if src_file is None else str(src_file)
    files = [str(f) for f in src_file]
    if not files:
        raise ValueError("`src_file` is an empty sequence: name the source files, or pass None to read the sources from the main input.")
    if len(files) == 1:
        return files[0]
    if len(files) > MAX_SOURCE_FILES:
        raise ValueError(f"`src_file` names {len(files)} source files; at most {MAX_SOURCE_FILES} are joined in one run.")
    for k, f in enumerate(files):
        if f in files[:k]:
            raise ValueError(f"`src_file` names {f} twice: every source file is read and joined once.")
    return files


def is_many(src_file) -> bool:
    return isinstance(src_file, (list, tuple))


def as_list(src_file) -> list:
    return [] if src_file is None else list(src_file) if is_many(src_file) else [src_file]


def owners(files, names) -> dict:
    """sample -> the number of the file that holds it, for the samples of the ``src`` list; every sample is held by
    exactly one of the files, and every file holds one."""
    from .utils.filesets import input_samples

    held = [set(input_samples(f)) for f in files]
    owner = {}
    for name in names:
        holders = [k for k, samples in enumerate(held) if name in samples]
        if not holders:
            raise ValueError(f"source sample {name} is held by none of the source files: {', '.join(files)}")
        if len(holders) > 1:
            raise ValueError(f"source sample {name} is held by two source files, {files[holders[0]]} and {files[holders[1]]}: "
                             "it must come from exactly one.")  # fmt: skip
        owner[name] = holders[0]
    for k, f in enumerate(files):
        if k not in owner.values():
            raise ValueError(f"source file {f} holds no sample of the src list: it would only remove sites. Leave it out.")
    return owner


def src_samples(ploidy_config, src_ind_file):
    """(population -> names of the ``src`` sample file, the names of the populations with a ploidy entry in first-seen order)."""
    from .utils.read_data import _parse_groups, _wanted

    groups = _parse_groups(ploidy_config, None, None, src_ind_file, None)
    names = []
    for _, pop_names, _ in _wanted(groups, ploidy_config):
        names += [n for n in pop_names if n not in names]
    return groups, names


def require_sources(files, ploidy_config, src_ind_file) -> dict:
    """The sample rule, checked before anything is read: ``owners`` of the configuration's ``src`` samples."""
    _, names = src_samples(ploidy_config, src_ind_file)
    return owners(files, names)


def join_many_host(lists):
    """``(rows, info)`` of 2 to 17 int32 position lists with ``sai_site_join_many_host``: per list the rows of the
    common positions (int32 arrays of n_common entries), and the ``2 + 2 k`` words of the entry point."""
    lib = load_host()
    lists = [np.ascontiguousarray(pos, dtype=np.int32) for pos in lists]
    k = len(lists)
    room = min(pos.size for pos in lists) if lists else 0
    rows = [np.empty(room, dtype=np.int32) for _ in lists]
    info = np.zeros(2 + 2 * k, dtype=np.int64)
    pos_ptrs = (C.c_void_p * max(k, 1))(*[pos.ctypes.data for pos in lists])
    row_ptrs = (C.c_void_p * max(k, 1))(*[r.ctypes.data for r in rows])
    sizes = np.array([pos.size for pos in lists], dtype=np.int64)
    _ffi.check(lib.sai_site_join_many_host(k, pos_ptrs, sizes.ctypes.data_as(C.c_void_p), row_ptrs, info.ctypes.data_as(C.c_void_p)), lib)
    n = int(info[0])
    return [r[:n] for r in rows], info


def _check_info(info, lists, files) -> None:
    if info[1] != -1:
        j = int(info[1])
        i = int(info[2 + j])
        raise ValueError(f"{files[j]}: position {int(lists[j][i])} repeats or does not ascend (after {int(lists[j][i - 1])}); two inputs are "
                         "joined on strictly ascending positions.")  # fmt: skip


def _summary(info, lists, files) -> dict:
    k = len(lists)
    identities = [bool(info[2 + k + j]) for j in range(k)]
    out = {"n_common": int(info[0]), "n_panel": int(lists[0].size), "n_sources": [int(pos.size) for pos in lists[1:]],
           "panel_identity": identities[0], "source_identities": identities[1:]}  # fmt: skip
    log.info("site join of %s and %s: %d common sites of %d and %s; panel rows: %s", files[0], ", ".join(files[1:]), out["n_common"],
             out["n_panel"], ", ".join(map(str, out["n_sources"])), "identity" if out["panel_identity"] else "selected")  # fmt: skip
    return out


def _no_data(panel, src_groups) -> dict:
    out = {group: (None, (panel.get(group) or (None, None))[1]) for group in ("ref", "tgt", "outgroup")}
    out["src"] = (None, src_groups["src"])
    return out


def read_host(vcf_file, files, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file, anc_allele_file, start, end,
              engine) -> dict:  # fmt: skip
    """``read_dosage_data(..., src_file=[...])``: the panel as a one-input read gives it, every source file's share of the
    ``src`` samples from its own reader, the k-way join, and the rows applied with numpy."""
    from .utils.genomic_dataclasses import ChromosomeData

    R = importlib.import_module(__package__ + ".utils.read_data")  # ``utils.read_data`` itself is the function of that name
    site_join.require_second_input(files[0], anc_allele_file)
    chr_name = str(chr_name)
    src_groups, names = src_samples(ploidy_config, src_ind_file)
    owner = owners(files, names)
    panel = R.read_dosage_data(vcf_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, None, out_ind_file, anc_allele_file, start, end,
                               engine)  # fmt: skip
    loader = R._load_python if engine == "python" else R._load_native
    where = chr_name if start is None and end is None else f"{chr_name}:{start}-{end}"
    loaded, positions, matched = {}, [], []  # (file, ploidy) -> (matrix, sample -> column)
    for j, f in enumerate(files):
        by_ploidy: dict = {}
        for _, pop_names, ploidy in R._wanted(src_groups, ploidy_config):
            bucket = by_ploidy.setdefault(ploidy, [])
            bucket += [n for n in pop_names if owner[n] == j and n not in bucket]
        pos_j, n_matched = None, 0
        for ploidy, wanted in by_ploidy.items():
            if not wanted:
                continue
            try:
                pos, dos, n_matched, n_anc = loader(f, chr_name, wanted, ploidy, start, end, anc_allele_file)
            except FileNotFoundError:
                raise
            except Exception as e:  # utils.py:139-140
                raise ValueError(f"Failed to read VCF file {f} from {where}: {e}") from e
            R._check_anc_found(anc_allele_file, n_matched, n_anc, chr_name, start, end)
            if pos_j is not None and not np.array_equal(pos_j, pos):
                raise RuntimeError(f"{f}: the passes over the file kept different records")
            pos_j = pos
            loaded[(j, ploidy)] = (dos, {n: i for i, n in enumerate(wanted)})
        positions.append(pos_j)
        matched.append(n_matched)
    panel_blocks = site_join._blocks_of(panel, ("ref", "tgt", "outgroup"))
    if not panel_blocks or any(m == 0 for m in matched):  # a region without a record in one of the inputs
        return _no_data(panel, src_groups)
    lists = [site_join._as_pos(site_join._one_position_list(panel_blocks, vcf_file)), *map(site_join._as_pos, positions)]
    names_of_files = [vcf_file, *files]
    rows, info = join_many_host(lists)
    _check_info(info, lists, names_of_files)
    summary = _summary(info, lists, names_of_files)
    if summary["n_common"] == 0:
        out = _no_data(panel, src_groups)
        out["site_join"] = summary
        return out
    pos = lists[0].copy() if summary["panel_identity"] else lists[0][rows[0]]
    identity = [summary["panel_identity"], *summary["source_identities"]]

    def of_panel(cd):
        return ChromosomeData(POS=pos, REF=None, ALT=None, GT=cd.GT if identity[0] else np.ascontiguousarray(cd.GT[rows[0]]))

    def of_sources(population, pop_names, ploidy):
        columns = []
        for n in pop_names:
            dos, column = loaded[(owner[n], ploidy)]
            col = dos[:, column[n]]
            columns.append(col if identity[1 + owner[n]] else col[rows[1 + owner[n]]])
        gt = np.ascontiguousarray(np.stack(columns, axis=1)) if columns else np.zeros((pos.size, 0), dtype=np.int8)
        return ChromosomeData(POS=pos, REF=None, ALT=None, GT=gt)

    out = {}
    for group in ("ref", "tgt", "outgroup"):
        data, samples = panel.get(group, (None, None))
        out[group] = ({p: of_panel(cd) for p, cd in data.items()} if data is not None else None, samples)
    out["src"] = R._assemble(src_groups, ploidy_config, of_sources)["src"]
    out["site_join"] = summary
    return out


def read_device(eng, vcf_file, files, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, src_ind_file, out_ind_file, anc_allele_file,
                start, end):  # fmt: skip
    """``read_data_device(..., src_file=[...])``: the panel's blocks and every source file's, each read as a one-input call
    reads them, the k-way join on the host, one upload of each input's row list, and per population one launch."""
    import torch

    from .site_join_device import RowTiler, upload_rows
    from .site_join_parts import SAI_TILE_MAX_PARTS, tile_parts
    from .utils.filesets import reader_for
    from .utils.genomic_dataclasses import ChromosomeData

    R = importlib.import_module(__package__ + ".utils.read_data")
    src_groups, names = src_samples(ploidy_config, src_ind_file)
    owner = owners(files, names)
    panel = R._read_blocks_device(eng, reader_for(vcf_file), vcf_file, chr_name, ploidy_config, ref_ind_file, tgt_ind_file, None, out_ind_file,
                                  anc_allele_file, start, end)  # fmt: skip
    sources = []
    for j, f in enumerate(files):
        share = {"src": {population: [n for n in pop_names if owner.get(n) == j] for population, pop_names in src_groups["src"].items()
                         if population in ploidy_config.root["src"]}}  # fmt: skip
        sources.append(R._read_blocks_device(eng, reader_for(f), f, chr_name, ploidy_config, None, None, None, None, anc_allele_file, start, end,
                                             samples_by_group=share))  # fmt: skip
    no_data = lambda population, pop_names, ploidy: None  # noqa: E731

    def merged(panel_block, src_block):
        got = R._assemble(panel[0], ploidy_config, panel_block)
        out = {group: got.get(group, (None, None)) for group in ("ref", "tgt", "outgroup")}
        out["src"] = R._assemble(src_groups, ploidy_config, src_block)["src"]
        return out

    sides = [panel, *sources]
    if any(column is None or n_matched == 0 for _, column, _, _, n_matched in sides):  # a region without a record in one of the inputs
        return merged(no_data, no_data), None
    lists = [site_join._as_pos(side[3]) for side in sides]
    names_of_files = [vcf_file, *files]
    rows, info = join_many_host(lists)
    _check_info(info, lists, names_of_files)
    summary = _summary(info, lists, names_of_files)
    if summary["n_common"] == 0:
        out = merged(no_data, no_data)
        out["site_join"] = summary
        return out, None
    pos = lists[0].copy() if summary["panel_identity"] else np.ascontiguousarray(lists[0][rows[0]])
    identity = [summary["panel_identity"], *summary["source_identities"]]
    rows_dev = [None if same else upload_rows(eng, r) for same, r in zip(identity, rows)]  # one upload per input; the identity passes no list
    tiler = RowTiler(eng)
    n_common = summary["n_common"]

    def of_panel(population, pop_names, ploidy):
        _, column, blocks, _, _ = panel
        where_cols = [column[(nme, ploidy)] for nme in pop_names]
        used, cols = {k for k, _ in where_cols}, [c for _, c in where_cols]
        if len(used) == 1 and cols == list(range(cols[0], cols[0] + len(cols))):  # the usual case: one run of columns
            source, col0 = blocks[used.pop()], cols[0]
        elif cols:  # gathered by columns first, as the one-input read does
            source, col0 = torch.stack([blocks[k][:, c] for k, c in where_cols], dim=1).contiguous(), 0
        else:
            source, col0 = blocks[0][:, :0], 0
        return ChromosomeData(POS=pos, REF=None, ALT=None, GT=tiler.tile(source, col0, len(cols), rows_dev[0]))

    def of_sources(population, pop_names, ploidy):
        # runs of neighbouring columns of one block, in the order of the sample list: (file, pass, first column, columns)
        runs = []
        for nme in pop_names:
            j = owner[nme]
            k, c = sources[j][1][(nme, ploidy)]
            if runs and runs[-1][:2] == (j, k) and runs[-1][2] + runs[-1][3] == c:
                runs[-1] = (j, k, runs[-1][2], runs[-1][3] + 1)
            else:
                runs.append((j, k, c, 1))
        if not runs:
            tiled = tiler.tile(sources[0][2][0][:, :0], 0, 0, rows_dev[1])
        elif len(runs) == 1:  # a population inside one file: the one-file route's launch
            j, k, c, n = runs[0]
            tiled = tiler.tile(sources[j][2][k], c, n, rows_dev[1 + j])
        elif len(runs) <= SAI_TILE_MAX_PARTS:
            tiled = tile_parts(tiler, [(sources[j][2][k], c, n, rows_dev[1 + j]) for j, k, c, n in runs], n_common)
        else:
            raise ValueError(f"source population {population} lies in {len(runs)} runs of neighbouring columns of its source files along the src "
                             f"list; at most {SAI_TILE_MAX_PARTS} are tiled in one launch: list the samples of one file together.")  # fmt: skip
        return ChromosomeData(POS=pos, REF=None, ALT=None, GT=tiled)

    out = merged(of_panel, of_sources)
    tiler.check()
    out["site_join"] = summary
    return out, torch.from_numpy(pos).to(eng.device)
