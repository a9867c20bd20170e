"""Sources from several files of their own on the GPU: ``sai_tile_rows_from_parts`` (sai_amd/csrc/join/tile_parts.hip)
against the layout formula of saihip.h computed with numpy -- every part with its own block, row count, odd stride, odd
column offset and row list --, its guard against row indices outside a part's block, its argument errors,
``read_data_device(..., src_file=[...])`` against ``Engine.tile_many`` of the host route's matrices, and ``score(...,
src_file=[...])`` against ``score`` on the one VCF of the common sites -- TSV, .U.log and .Q.log byte for byte: the
device route, the host route, several chunks, the command line and two workers."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import site_join_many_cases as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

TILE = 64
N_ROWS = (0, 1, 63, 64, 65, 129)
# [16, 1]: 17 individuals, the next workgroup width; [255, 2]: a part that straddles the 256-column block boundary
WIDTHS = ([1], [1, 1], [1, 2, 1], [3, 1], [4, 1], [16, 1], [255, 2], [150, 150], [1] * 16)
SENTINEL = 85


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


@pytest.fixture(autouse=True)
def at_the_root(monkeypatch):
    monkeypatch.chdir(ROOT)


def expected_tiles(parts, n_rows):
    """byte(t, ind0_p + i, s) = block_p[rows_p[t * 64 + s]][col0_p + i] over ``parts`` = (block, col0, n_ind, rows or
    None) in the order of their individuals; zero in the padding sites and where a row index lies outside its block."""
    n_ind = sum(n for _, _, n, _ in parts)
    n_tiles = -(-n_rows // TILE)
    padded = np.zeros((n_tiles * TILE, n_ind), dtype=np.int8)
    ind0 = 0
    for block, col0, n, rows in parts:
        rows = np.arange(n_rows, dtype=np.int64) if rows is None else np.asarray(rows[:n_rows], dtype=np.int64)
        inside = (rows >= 0) & (rows < block.shape[0])
        padded[np.flatnonzero(inside), ind0 : ind0 + n] = block[rows[inside], col0 : col0 + n]
        ind0 += n
    return np.ascontiguousarray(padded.reshape(n_tiles, TILE, n_ind).transpose(0, 2, 1)).reshape(-1)


def device_block(eng, host, margin=0, fill=0):
    """``host`` as an interior view of a device tensor with ``margin`` rows of ``fill`` before and behind it."""
    import torch

    whole = torch.full((host.shape[0] + 2 * margin, host.shape[1]), fill, dtype=torch.int8, device=eng.device)
    view = whole[margin : margin + host.shape[0]]
    view.copy_(torch.from_numpy(host))
    return view


def make_parts(rng, widths, n_rows, kind):
    """Host parts (block, col0, n_ind, rows) for ``widths``: every block has its own row count, an odd stride and an odd
    column offset.  ``kind`` names the row lists: "subsets" (ascending subsets; the first part is the identity, the NULL
    list, beside them), "reversed", "repeated", or "unsorted"."""
    parts = []
    for k, w in enumerate(widths):
        identity = kind == "subsets" and k == 0
        n_src = n_rows if identity else n_rows + 3 + 2 * k
        width = w + 3 + (w % 2)  # odd, and wider than the part
        assert width % 2 == 1
        block = rng.integers(-128, 128, size=(n_src, width), dtype=np.int8)
        if identity:
            rows = None
        elif kind == "subsets":
            rows = np.sort(rng.choice(n_src, size=n_rows, replace=False)).astype(np.int32)
        elif kind == "reversed":
            rows = np.arange(n_src, dtype=np.int32)[::-1][:n_rows].copy()
        elif kind == "repeated":
            rows = np.full(n_rows, n_src // 2, dtype=np.int32)
        else:
            rows = rng.integers(0, n_src, size=n_rows).astype(np.int32)
        parts.append((block, 1 + 2 * (k % 2), w, rows))
    return parts


def tile_on_device(eng, tiler, parts, n_rows, order=None):
    """``tile_parts`` of host parts; ``order``: the places of the parts in the call (their ``ind0`` stays)."""
    import torch

    from sai_amd import site_join_parts as P

    dev = [(device_block(eng, block), col0, n, None if rows is None else torch.from_numpy(rows).to(eng.device)) for block, col0, n, rows in parts]
    if order is None:
        return P.tile_parts(tiler, dev, n_rows)
    return raw_call(eng, tiler, dev, n_rows, order)


def raw_call(eng, tiler, dev, n_rows, order):
    """The entry point itself, the parts handed over in ``order``."""
    import torch

    from sai_amd import _ffi
    from sai_amd import site_join_parts as P
    from sai_amd.engine import TiledPop

    lib = P.load()
    ind0 = np.concatenate([[0], np.cumsum([n for _, _, n, _ in dev])])
    table = (P.TilePart * len(dev))()
    for place, k in enumerate(order):
        block, col0, n, rows = dev[k]
        table[place] = P.TilePart(block.data_ptr() + col0 if block.numel() else None, block.shape[0], block.stride(0) if block.shape[0] > 1 else block.shape[1],
                                  rows.data_ptr() if rows is not None and rows.numel() else None, int(ind0[k]), n)  # fmt: skip
    n_ind = int(ind0[-1])
    dst = torch.empty(max(int(eng.lib.sai_tiled_bytes(n_rows, n_ind)), 0), dtype=torch.int8, device=eng.device)
    n_bad = torch.empty(1, dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_tile_rows_from_parts(eng.ctx, len(dev), table, n_rows, n_ind, C.c_void_p(dst.data_ptr()), C.c_void_p(n_bad.data_ptr()),
                                            eng._stream()), lib)  # fmt: skip
    tiler._bad.append(n_bad)
    return TiledPop(dst, n_rows, n_ind)


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "-".join(map(str, w)) if len(w) < 16 else "16x1")
def test_kernel_equals_the_layout_formula(eng, widths):
    from sai_amd.site_join_device import RowTiler

    rng = np.random.default_rng(2000 + 31 * len(widths) + sum(widths))
    tiler = RowTiler(eng)
    for n in N_ROWS:
        for kind in ("subsets", "reversed", "repeated"):
            if n == 0 and kind != "subsets":
                continue
            parts = make_parts(rng, widths, n, kind)
            got = tile_on_device(eng, tiler, parts, n)
            want = expected_tiles(parts, n)
            assert (got.n_sites, got.n_ind) == (n, sum(widths))
            assert got.tiles.numel() == want.size and np.array_equal(got.tiles.cpu().numpy(), want), (widths, n, kind)
    tiler.check()


@pytest.mark.parametrize("widths", ([1, 1, 1, 1], [1, 2, 1], [16, 1], [100, 3, 40], [255, 2], [150, 150], [300, 1, 2], [1] * 16),
                         ids=lambda w: "-".join(map(str, w)) if len(w) < 16 else "16x1")  # fmt: skip
def test_kernel_over_several_workgroups_with_the_parts_in_any_order(eng, widths):
    """2 053 unsorted rows with repeats are more than two workgroups of sites at every width a workgroup takes; the parts
    are handed over last first and rotated, their individuals staying where they are."""
    from sai_amd.site_join_device import RowTiler

    rng = np.random.default_rng(sum(widths) + len(widths))
    n_rows = 2 * 16 * TILE + 5
    parts = make_parts(rng, widths, n_rows, "unsorted")
    want = expected_tiles(parts, n_rows)
    tiler = RowTiler(eng)
    got = tile_on_device(eng, tiler, parts, n_rows)
    assert np.array_equal(got.tiles.cpu().numpy(), want)
    k = len(widths)
    for order in (list(range(k))[::-1], [(i + k // 2) % k for i in range(k)]):
        again = tile_on_device(eng, tiler, parts, n_rows, order)
        assert np.array_equal(again.tiles.cpu().numpy(), want), order
    tiler.check()


@pytest.mark.parametrize("n_ind", (1, 3, 4, 17, 130, 300))
def test_one_part_equals_the_one_block_kernel(eng, n_ind):
    import torch

    from sai_amd import site_join_parts as P
    from sai_amd.site_join_device import RowTiler

    rng = np.random.default_rng(n_ind)
    tiler = RowTiler(eng)
    for n_src, n_rows in ((129, 129), (700, 333)):
        block = device_block(eng, rng.integers(-128, 128, size=(n_src, n_ind + 5), dtype=np.int8))
        rows = None if n_rows == n_src else torch.from_numpy(rng.integers(0, n_src, size=n_rows).astype(np.int32)).to(eng.device)
        one = tiler.tile(block, 3, n_ind, rows)
        got = P.tile_parts(tiler, [(block, 3, n_ind, rows)])
        assert (got.n_sites, got.n_ind) == (one.n_sites, one.n_ind) and torch.equal(got.tiles, one.tiles)
    tiler.check()


@pytest.mark.parametrize("widths,bad_part", (([2, 1, 3], 1), ([1, 7, 2], 1), ([64, 2, 40], 0), ([255, 2, 1], 1)))
def test_rows_out_of_range_in_one_part_are_counted_and_not_read(eng, widths, bad_part):
    """The bad part's block is an interior view of a tensor filled with a sentinel, one row of margin on each side: a
    kernel without the guard would read the margin (never memory outside the tensor) and show sentinel bytes."""
    import torch

    from sai_amd import site_join_parts as P
    from sai_amd.site_join_device import RowTiler

    rng = np.random.default_rng(500 + sum(widths))
    n_rows = 150
    values = np.array([v for v in range(-128, 128) if v not in (0, SENTINEL)], dtype=np.int8)
    host, dev = [], []
    bad_at = np.array([0, 5, 63, 64, 65, 127, 128, 149])
    for k, w in enumerate(widths):
        n_src = 97 + k
        block = values[rng.integers(0, values.size, size=(n_src, w + 4))]
        rows = rng.integers(0, n_src, size=n_rows).astype(np.int32)
        if k == bad_part:
            rows[bad_at] = np.where(np.arange(bad_at.size) % 2 == 0, -1, n_src)
        host.append((block, 3, w, rows))
        dev.append((device_block(eng, block, margin=1, fill=SENTINEL), 3, w, torch.from_numpy(rows).to(eng.device)))
    tiler = RowTiler(eng)
    got = P.tile_parts(tiler, dev, n_rows)
    assert int(tiler._bad[0].cpu()) == bad_at.size  # once per (site, part), however many column blocks the part lies in
    tiles = got.tiles.cpu().numpy()
    assert SENTINEL not in tiles and np.array_equal(tiles, expected_tiles(host, n_rows))
    n_ind = sum(widths)
    per_site = tiles.reshape(-1, n_ind, TILE).transpose(0, 2, 1).reshape(-1, n_ind)[:n_rows]
    lo = sum(widths[:bad_part])
    mine = per_site[:, lo : lo + widths[bad_part]]
    assert not mine[bad_at].any() and mine[np.setdiff1d(np.arange(n_rows), bad_at)].all()
    assert np.delete(per_site, np.s_[lo : lo + widths[bad_part]], axis=1).all()  # the other parts' bytes, at the bad sites too
    with pytest.raises(RuntimeError, match=rf"met {bad_at.size} row indices outside their block"):
        tiler.check()
    P.tile_parts(tiler, [(b, c, w, r[1:5].contiguous()) for b, c, w, r in dev[:1]], 4)  # a call after it starts from zero again
    tiler.check()


def test_argument_errors(eng):
    import torch

    from sai_amd import _ffi
    from sai_amd import site_join_parts as P
    from sai_amd.site_join_device import RowTiler

    lib = P.load()
    src = torch.zeros((4, 8), dtype=torch.int8, device=eng.device)
    rows = torch.zeros(4, dtype=torch.int32, device=eng.device)
    dst = torch.full((64 * 8 + 16,), 9, dtype=torch.int8, device=eng.device)
    n_bad = torch.full((1,), 7, dtype=torch.int32, device=eng.device)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def table(*parts):
        out = (P.TilePart * max(len(parts), 1))()
        for k, fields in enumerate(parts):
            out[k] = P.TilePart(*fields)
        return out

    part = lambda ind0, n, **kw: (kw.get("src", src.data_ptr()), kw.get("n_src", 4), kw.get("stride", 8), kw.get("rows", rows.data_ptr()), ind0, n)  # noqa: E731
    call = lambda ctx, n_parts, parts, n_rows, n_ind, d=p(dst), b=p(n_bad): lib.sai_tile_rows_from_parts(ctx, n_parts, parts, n_rows, n_ind, d, b, eng._stream())  # noqa: E731
    two = table(part(0, 5), part(5, 3))
    assert call(None, 2, two, 4, 8) == _ffi.SAI_ERR_ARG and lib.sai_last_error() == b"ctx is NULL"
    for args, code, words in (
        ((0, two, 4, 8), _ffi.SAI_ERR_ARG, b"n_parts 0 is outside 1..16"),
        ((17, (P.TilePart * 17)(), 4, 8), _ffi.SAI_ERR_ARG, b"n_parts 17 is outside 1..16"),
        ((2, two, -4, 8), _ffi.SAI_ERR_ARG, b"negative size"),
        ((2, two, 4, -8), _ffi.SAI_ERR_ARG, b"negative size"),
        ((2, table(part(0, 5, n_src=-1), part(5, 3)), 4, 8), _ffi.SAI_ERR_ARG, b"negative size"),
        ((2, table(part(0, -5), part(5, 3)), 4, 8), _ffi.SAI_ERR_ARG, b"negative size"),
        ((2, None, 4, 8), _ffi.SAI_ERR_ARG, b"NULL buffer"),
        ((2, two, 4, 8, p(dst), None), _ffi.SAI_ERR_ARG, b"NULL buffer"),
        ((2, two, 4, 8, None), _ffi.SAI_ERR_ARG, b"NULL buffer"),
        ((2, table(part(0, 5, src=None), part(5, 3)), 4, 8), _ffi.SAI_ERR_ARG, b"NULL buffer"),
        ((2, two, 4, 8, p(dst, 8)), _ffi.SAI_ERR_ARG, b"dst is not 16-byte aligned"),
        ((2, table(part(0, 5, stride=4), part(5, 3)), 4, 8), _ffi.SAI_ERR_ARG, b"row_stride 4 < n_ind 5"),
        ((2, table(part(0, 5), part(5, 3, rows=None)), 3, 8), _ffi.SAI_ERR_ARG, b"rows is NULL (the identity) but n_rows 3 != n_src_rows 4"),
        ((2, table(part(0, 5), part(4, 3)), 4, 8), _ffi.SAI_ERR_ARG, b"the parts overlap or leave a gap: they hold 8 individuals and cover 0 .. 5 of 8"),
        ((2, table(part(0, 5), part(6, 2)), 4, 8), _ffi.SAI_ERR_ARG, b"the parts overlap or leave a gap: they hold 7 individuals and cover 0 .. 5 of 8"),
        ((2, table(part(0, 4), part(0, 4)), 4, 8), _ffi.SAI_ERR_ARG, b"the parts overlap or leave a gap: they hold 8 individuals and cover 0 .. 4 of 8"),
        ((2, table(part(1, 4), part(5, 3)), 4, 8), _ffi.SAI_ERR_ARG, b"the parts overlap or leave a gap: they hold 7 individuals and cover 0 .. 0 of 8"),
        ((2, two, 4, 9), _ffi.SAI_ERR_ARG, b"the parts overlap or leave a gap: they hold 8 individuals and cover 0 .. 8 of 9"),
        ((1, table(part(0, 65536 * 256 + 1, stride=65536 * 256 + 1)), 4, 65536 * 256 + 1), _ffi.SAI_ERR_UNSUPPORTED, b"block too large for one launch"),
    ):  # fmt: skip
        assert call(eng.ctx, *args) == code and lib.sai_last_error() == words, words
    torch.cuda.synchronize()
    assert (dst == 9).all()  # a refused call writes nothing
    for n_ind, n_rows, parts in ((0, 4, table(part(0, 0))), (8, 0, two)):  # nothing to tile: SAI_OK, and nothing but the count is touched
        n_bad.fill_(7)
        assert call(eng.ctx, len(parts), parts, n_rows, n_ind, None) == 0
        torch.cuda.synchronize()
        assert int(n_bad.cpu()) == 0 and (dst == 9).all()
    with pytest.raises(ValueError, match="1 to 16 parts, not 17"):
        P.tile_parts(RowTiler(eng), [(src, 0, 0, None)] * 17)
    with pytest.raises(ValueError, match="different numbers of sites"):
        P.tile_parts(RowTiler(eng), [(src, 0, 4, None), (src, 4, 4, rows[:3])])


# -- the resident reader ---------------------------------------------------------------------------------------------------

GROUPS = ("ref", "tgt", "src", "outgroup")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("many_inputs")
    out = M.write_inputs(tmp)
    out["paths"] = {cut: M.write_sources(out, cut, tmp) for cut in M.CUTS}
    out["tmp"] = tmp
    return out


@pytest.fixture(scope="module")
def readers(eng, inputs):
    from sai_amd.utils.read_data import read_data_device, read_dosage_data

    os.chdir(ROOT)
    cfg, files = M.reader_arguments(inputs)
    host = lambda vcf, **kw: read_dosage_data(vcf, "1", cfg.ploidies, *files, inputs["anc"], **kw)  # noqa: E731
    device = lambda vcf, **kw: read_data_device(eng, vcf, "1", cfg.ploidies, *files, inputs["anc"], **kw)  # noqa: E731
    return host, device


def assert_device_equals_host(eng, got, pos_dev, want):
    """Every population's tiles are ``Engine.tile_many`` of the host route's matrix; ONE position array for all."""
    import torch

    keys = [(g, p) for g in GROUPS for p in (want[g][0] or {})]
    assert keys == [(g, p) for g in GROUPS for p in (got[g][0] or {})] and len(keys) == 5
    assert all(got[g][1] == want[g][1] for g in GROUPS)
    tiled = eng.tile_many([want[g][0][p].GT for g, p in keys])
    pos = got["ref"][0]["ref"].POS
    for (g, p), t in zip(keys, tiled):
        block = got[g][0][p]
        assert block.POS is pos, (g, p)
        assert (block.GT.n_sites, block.GT.n_ind) == (t.n_sites, t.n_ind) and torch.equal(block.GT.tiles, t.tiles), (g, p)
    assert pos.dtype == np.int32 and np.array_equal(pos, want["ref"][0]["ref"].POS)
    assert pos_dev.dtype == torch.int32 and np.array_equal(pos_dev.cpu().numpy(), pos)
    assert got["site_join"] == want["site_join"]


@pytest.mark.parametrize("cut", sorted(M.CUTS))
def test_reader_equals_the_host_route(eng, inputs, readers, cut):
    host, device = readers
    paths = inputs["paths"][cut]
    for kw in ({}, M.REGION):
        want = host(inputs["panel"], src_file=paths, **kw)
        got, pos_dev = device(inputs["panel"], src_file=paths, **kw)
        assert_device_equals_host(eng, got, pos_dev, want)
        join = got["site_join"]
        assert 0 < join["n_common"] < min(join["n_sources"]) and not join["panel_identity"] and len(join["n_sources"]) == cut
        assert (got["src"][0]["NEA"].GT.n_ind, got["src"][0]["DEN"].GT.n_ind) == (3, 1)
    assert want["src"][0]["NEA"].POS.size < inputs["n_common"][cut]  # the region holds a part of the common sites


def test_reader_identity_no_common_site_and_no_record(eng, inputs, readers):
    host, device = readers
    tmp = inputs["tmp"]
    # the identity on every side: the common VCF as the panel and, cut by samples, as both source files
    lines = open(inputs["common"][2]).read().splitlines()
    head = next(i for i, ln in enumerate(lines) if ln.startswith("#CHROM"))
    columns = lines[head].split("\t")
    paths = []
    for k, names in enumerate((["src_i1", "tgt_i502"], ["tgt_i501", "tgt_i503"])):
        keep = list(range(9)) + [columns.index(n) for n in names]
        text = "\n".join(lines[:head] + ["\t".join(ln.split("\t")[i] for i in keep) for ln in lines[head:]]) + "\n"
        paths.append(str(tmp / f"same_{k}.vcf"))
        open(paths[-1], "w").write(text)
    want = host(inputs["common"][2], src_file=paths)
    got, pos_dev = device(inputs["common"][2], src_file=paths)
    assert_device_equals_host(eng, got, pos_dev, want)
    assert got["site_join"]["panel_identity"] and got["site_join"]["source_identities"] == [True, True]
    one = host(inputs["common"][2])
    for g in GROUPS:
        for p, block in one[g][0].items():
            assert np.array_equal(block.GT, want[g][0][p].GT) and np.array_equal(block.POS, want[g][0][p].POS)
    # no common site: one file holds its own sites only
    a, b = inputs["paths"][3][0], inputs["paths"][3][1:]
    import gzip

    own = [ln for ln in gzip.open(a, "rt").read().splitlines() if ln.startswith("#") or int(ln.split("\t")[1]) in M.OWN_SITES[0]]
    (tmp / "apart.vcf").write_text("\n".join(own) + "\n")
    apart = [str(tmp / "apart.vcf"), *b]
    want = host(inputs["panel"], src_file=apart)
    got, pos_dev = device(inputs["panel"], src_file=apart)
    assert pos_dev is None and got["site_join"] == want["site_join"] and got["site_join"]["n_common"] == 0
    assert {g: got[g] for g in GROUPS} == {g: want[g] for g in GROUPS} and all(got[g][0] is None and got[g][1] for g in GROUPS)
    # a region without a record in one of the inputs: as the host route, without a summary
    want = host(inputs["panel"], src_file=inputs["paths"][3], start=39900, end=39910)
    got, pos_dev = device(inputs["panel"], src_file=inputs["paths"][3], start=39900, end=39910)
    assert pos_dev is None and {g: got[g] for g in GROUPS} == {g: want[g] for g in GROUPS} and "site_join" not in got and "site_join" not in want


# -- score -------------------------------------------------------------------------------------------------------------------

WIN = (8000, 4000)


def files_of(out):
    return {p.name[len(out.stem) :]: p.read_bytes() for p in out.parent.glob(out.stem + "*")}


def score_files(run, vcf, src_file, out):
    from sai_amd.sai import score

    second = {} if src_file is None else {"src_file": src_file}
    score(vcf_file=vcf, chr_name="1", win_len=WIN[0], win_step=WIN[1], anc_allele_file=run["anc"], output_file=str(out), config=run["config"],
          num_workers=1, **second)  # fmt: skip
    return files_of(out)


@pytest.fixture(scope="module")
def run(inputs, tmp_path_factory):
    """Per cut: the panel clipped to the span of the common sites (so that its window grid is the common VCF's), a
    configuration with U, Q and DD besides fd, df, Danc and Dplus, and the files ``score`` writes for the common VCF."""
    tmp = tmp_path_factory.mktemp("score_many_inputs")
    uq = "    ref:\n      ref: 0.3\n    tgt:\n      tgt: {x}\n    src:\n      NEA: \"=1\"\n      DEN: \"=1\"\n"
    statistics = "statistics:\n  U:\n" + uq.format(x=0.2) + "  Q:\n" + uq.format(x=0.9) + "  DD: true\n  fd: True\n  df: True\n  Danc: True\n  Dplus: True\n"
    (tmp / "config.yaml").write_text(M.config_text(inputs["lists"], statistics))
    out = dict(tmp=tmp, config=str(tmp / "config.yaml"), anc=inputs["anc"], panel={}, want={})
    os.chdir(ROOT)
    lines = open(inputs["panel"]).read().splitlines()
    for cut in M.CUTS:
        common = [int(ln.split("\t")[1]) for ln in open(inputs["common"][cut]) if not ln.startswith("#")]
        kept = [ln for ln in lines if ln.startswith("#") or common[0] <= int(ln.split("\t")[1]) <= common[-1]]
        panel_pos = [int(ln.split("\t")[1]) for ln in kept if not ln.startswith("#")]
        assert (panel_pos[0], panel_pos[-1]) == (common[0], common[-1]) and len(set(panel_pos) - set(common)) > 10
        out["panel"][cut] = str(tmp / f"panel{cut}.vcf")
        open(out["panel"][cut], "w").write("\n".join(kept) + "\n")
        out["want"][cut] = score_files(out, inputs["common"][cut], None, tmp / f"common{cut}" / "s.tsv")
        assert set(out["want"][cut]) == {".tsv", ".U.log", ".Q.log"} and len(out["want"][cut][".tsv"].splitlines()) > 5
    header = out["want"][2][".tsv"].splitlines()[0].split(b"\t")
    assert header[-12:] == [b"U", b"Q", *(f"{s}.{p}".encode() for s in ("DD", "fd", "df", "Danc", "Dplus") for p in ("NEA", "DEN"))]
    return out


def child_environment(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                            "SAI_AMD_INGEST", "SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT")}  # fmt: skip
    env.update(extra)
    return env


def sai_score(run, panel, sources, out, workers, **env):
    argv = [sys.executable, "-m", "sai_amd", "score", "--vcf", panel, *(a for s in sources for a in ("--src-input", s)), "--chr-name", "1",
            "--win-len", str(WIN[0]), "--win-step", str(WIN[1]), "--anc-alleles", run["anc"], "--config", run["config"], "--output", str(out),
            "--num-workers", str(workers)]  # fmt: skip
    res = subprocess.run(argv, cwd=str(ROOT), env=child_environment(**env), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    return files_of(out)


@pytest.mark.parametrize("cut", sorted(M.CUTS))
def test_score_writes_the_files_of_the_common_vcf(eng, inputs, run, tmp_path, monkeypatch, cut):
    from sai_amd import sai as sai_mod

    monkeypatch.chdir(ROOT)
    for name in ("SAI_AMD_INGEST", "SAI_AMD_HBM_BUDGET_BYTES", "SAI_AMD_LAYOUT", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    panel, sources, want = run["panel"][cut], inputs["paths"][cut], run["want"][cut]
    assert score_files(run, panel, sources, tmp_path / "device" / "s.tsv") == want
    assert score_files(run, panel, tuple(sources[::-1]), tmp_path / "reversed" / "s.tsv") == want  # the order of the files is not the order of the individuals
    monkeypatch.setenv("SAI_AMD_INGEST", "host")
    assert score_files(run, panel, sources, tmp_path / "host" / "s.tsv") == want
    monkeypatch.delenv("SAI_AMD_INGEST")
    # several chunks through the one GPU: every chunk reads and joins its own region of all files
    one_chunk = sai_mod.chunks_for_memory(panel, src_file=sources)
    monkeypatch.setenv("SAI_AMD_HBM_BUDGET_BYTES", str(os.path.getsize(panel) // 4 // 3))
    assert one_chunk == 1 and sai_mod.chunks_for_memory(panel, src_file=sources) >= 3
    assert score_files(run, panel, sources, tmp_path / "chunks" / "s.tsv") == want
    monkeypatch.delenv("SAI_AMD_HBM_BUDGET_BYTES")
    if cut == 2:  # the command, as a child process
        assert sai_score(run, panel, sources, tmp_path / "cli" / "s.tsv", 1) == want


def test_sai_score_with_two_workers_and_three_source_files(inputs, run, tmp_path):
    """`sai score --num-workers 2 --src-input A --src-input B --src-input C`: the process starts its two ranks as a child job,
    both on this box's one GPU with gloo for the gather; each rank reads and joins its own regions of all files."""
    assert sai_score(run, run["panel"][3], inputs["paths"][3], tmp_path / "two" / "s.tsv", 2, SAI_AMD_DIST_BACKEND="gloo") == run["want"][3]
