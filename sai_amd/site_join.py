"""Sources from a file of their own: what lies between reading two inputs and scoring them (DESIGN_INGEST.md, "Sources
from a file of their own").  The panel (ref, tgt, outgroup) and the source file are each read by their own reader, both
polarised by the same ancestral alleles; here their position lists are brought to the common rows
(``sai_site_join_host``) and every population keeps the rows of the common sites only, so that everything downstream sees
one position list.  The join itself is a host call for every route: the readers hand their positions back as host
arrays and the window grid needs the common positions there.  What differs is how the rows are applied: the host
readers (``read_dosage_data(..., src_file=)``, the ``WindowGenerator`` over host matrices) select them with numpy here;
the resident reader (``read_data_device(..., src_file=)``, which ``score(..., src_file=)`` and ``sai score --src-input``
run on) uploads each input's row list once and re-tiles every population from those rows of its device block in one
launch (``sai_amd.site_join_device``).  Several source files -- a list in place of the one path -- are
``sai_amd.site_join_many``, which builds on this module.
"""

from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from . import _ffi, _ffi_join

log = logging.getLogger(__name__)

GROUPS = ("ref", "tgt", "src", "outgroup")


def require_second_input(src_file, anc_allele_file) -> None:
    """What a read with ``src_file`` cannot serve, refused before anything is read."""
    if src_file is not None and anc_allele_file is None:
        raise ValueError("A source file of its own (`src_file`) requires `anc_allele_file`: the two inputs are reconciled through the "
                         "ancestral allele, which decides in each of them which allele is counted. Joining two inputs by the panel's "
                         "REF allele instead is the follow-up.")  # fmt: skip


def _check_info(info, pos_a, pos_b, file_a, file_b) -> None:
    for word, pos, name in ((1, pos_a, file_a), (2, pos_b, file_b)):
        if info[word] != -1:
            i = int(info[word])
            raise ValueError(f"{name}: position {int(pos[i])} repeats or does not ascend (after {int(pos[i - 1])}); two inputs are joined "
                             "on strictly ascending positions.")  # fmt: skip


def _as_pos(pos) -> np.ndarray:
    return np.ascontiguousarray(pos, dtype=np.int32)


def join_host(pos_a, pos_b):
    """``(rows_a, rows_b, info)`` of two int32 position lists with ``sai_site_join_host``: the rows of the common
    positions (int32 arrays of n_common entries) and the four words of include/saihip_join.h."""
    lib = _ffi_join.load_host()
    pos_a, pos_b = _as_pos(pos_a), _as_pos(pos_b)
    room = min(pos_a.size, pos_b.size)
    rows_a, rows_b = np.empty(room, dtype=np.int32), np.empty(room, dtype=np.int32)
    info = np.zeros(_ffi_join.SAI_JOIN_INFO_WORDS, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _ffi.check(lib.sai_site_join_host(ptr(pos_a), pos_a.size, ptr(pos_b), pos_b.size, ptr(rows_a), ptr(rows_b), ptr(info)), lib)
    n = int(info[0])
    return rows_a[:n], rows_b[:n], info


def _summary(info, n_a, n_b, file_a, file_b) -> dict:
    out = {"n_common": int(info[0]), "n_panel": int(n_a), "n_source": int(n_b), "panel_identity": bool(info[3]),
           "source_identity": int(info[0]) == int(n_b)}  # fmt: skip
    log.info("site join of %s and %s: %d common sites of %d and %d; panel rows: %s", file_a, file_b, out["n_common"], n_a, n_b,
             "identity" if out["panel_identity"] else "selected")  # fmt: skip
    return out


def _blocks_of(results, groups):
    return [cd for g in groups for cd in ((results.get(g) or (None, None))[0] or {}).values()]


def _one_position_list(blocks, name):
    pos = blocks[0].POS
    for b in blocks[1:]:
        if b.POS is not pos and not np.array_equal(b.POS, pos):
            raise RuntimeError(f"{name}: the passes over the file kept different records")
    return pos


def _merged(panel, source, replace) -> dict:
    """The result of a one-input read put together from the two: ref, tgt and outgroup of the panel, src of the source
    file; ``replace(block)`` gives the joined block, or the populations are without data when it is None."""
    out = {}
    for group in GROUPS:
        data, samples = (source if group == "src" else panel).get(group, (None, None))
        if data is not None:
            data = {population: replace(cd) for population, cd in data.items()} if replace is not None else None
        out[group] = (data, samples)
    return out


def join_host_results(panel: dict, source: dict, panel_file, src_file) -> dict:
    """Two results of ``read_dosage_data`` (host matrices) as one over their common sites."""
    from .utils.genomic_dataclasses import ChromosomeData

    a, b = _blocks_of(panel, ("ref", "tgt", "outgroup")), _blocks_of(source, ("src",))
    if not a or not b:  # a region without a record in one of the inputs
        return _merged(panel, source, None)
    pos_a, pos_b = _one_position_list(a, panel_file), _one_position_list(b, src_file)
    rows_a, rows_b, info = join_host(pos_a, pos_b)
    _check_info(info, pos_a, pos_b, panel_file, src_file)
    summary = _summary(info, pos_a.size, pos_b.size, panel_file, src_file)
    if summary["n_common"] == 0:
        out = _merged(panel, source, None)
        out["site_join"] = summary
        return out
    pos = pos_a.copy() if summary["panel_identity"] else pos_a[rows_a]
    in_panel = {id(cd) for cd in a}

    def replace(cd):
        identity, rows = (summary["panel_identity"], rows_a) if id(cd) in in_panel else (summary["source_identity"], rows_b)
        return ChromosomeData(POS=pos, REF=None, ALT=None, GT=cd.GT if identity else np.ascontiguousarray(cd.GT[rows]))

    out = _merged(panel, source, replace)
    out["site_join"] = summary
    return out
