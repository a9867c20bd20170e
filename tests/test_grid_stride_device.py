"""Every kernel whose grid is capped at a multiple of the CU count, past its first grid-stride iteration.

The five fileset decoders launch at most ``16 * n_cu`` blocks and the site family at most ``16 * n_cu`` one-wave
blocks (12 or 8 per CU where the launcher says so); everything beyond is taken in a grid-stride loop.  Each test here
runs one of them at the smallest work count at which every block makes at least two passes of that loop and some make
three -- ``2 * cap + a small odd remainder`` -- and asserts that from the caps restated below, so a shape that falls
back into one iteration fails instead of passing.  What one iteration leaves for the next is what is under test: the
LDS codes of the row before, the exits after a damaged record, per-row locals, the statuses of rows a wave has left.

The cases come from tests/test_grid_stride_cpu.py, which proves them on the host: narrow rows, few distinct inputs
referenced by all rows, and the expectation a numpy statement applied to the distinct inputs and gathered.  Every
comparison is exact and covers the whole output, every status and ``unfit``, and the rows around the call.  The
64-bit-division form of ``bed_decode`` / ``geno_decode`` needs more than 4 GiB of output in one call and stays out."""

import ctypes as C

import numpy as np
import pytest

import test_grid_stride_cpu as G
from test_bed_pack2_device import DeviceCall as BedPackCall
from test_hip_kernels import oracle_decisions
from test_pgen_pack2_device import DeviceCall as PgenPackCall

pytestmark = pytest.mark.gpu

# `const int64_t cap = static_cast<int64_t>(ctx->n_cu) * 16;` -- the blocks of sai_pgen_decode (pgen/pgen_decode.hip),
# sai_pgen_pack2 (pgen/pgen_pack2.hip), sai_plink_decode (plink/bed_decode.hip), sai_eigenstrat_decode
# (eigenstrat/geno_decode.hip) and sai_bed_pack2 (plink/bed_pack2.hip)
DECODER_BLOCKS_PER_CU = 16
# `constexpr int kStreamWavesPerCu = 16;` (common.hpp) -- the most one-wave blocks per CU `stream_grid` launches, and the
# largest value `site_pass_waves_per_cu` / `dd_pass_waves_per_cu` return (they also return 12 and 8)
SITE_TILES_PER_CU = 16
BED_PACK2_WAVES_PER_BLOCK = 4  # `constexpr int kPackBlock = 256;` (plink/bed_pack2.hip): a unit per wave


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


@pytest.fixture(scope="module")
def n_cu(eng):
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def cap(n_cu):
    return DECODER_BLOCKS_PER_CU * n_cu


_records = {}


def records_of(n):
    if n not in _records:
        _records[n] = G.wide_pgen_records(n) if n > 16384 else G.pgen_records(n)
    return _records[n]


def dev(eng, a, dtype=None):
    import torch

    return torch.from_numpy(np.array(a, dtype=dtype)).to(eng.device)  # a writable copy


def stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- sai_pgen_decode ----


def run_pgen_decode(eng, case, out_row0, tail_rows=2):
    """One ``sai_pgen_decode`` call; -> (the whole block with the rows around the call, status)."""
    import torch

    from sai_amd import _ffi, _ffi_pgen

    lib = _ffi_pgen.load()
    data = dev(eng, np.frombuffer(bytes(case["data"]), dtype=np.uint8))
    rec, base, flip = dev(eng, case["rec"], np.int64), dev(eng, case["base"], np.int64), dev(eng, case["flip"])
    cols, ploidies = dev(eng, case["cols"]), dev(eng, case["ploidies"])
    n_out, n_slots, first_col, uniform = len(case["rec"]), len(case["cols"]), case["first_col"], case["uniform"]
    out = torch.full((out_row0 + n_out + tail_rows, n_slots), 77, dtype=torch.int8, device=eng.device)
    status = torch.full((n_out,), -5, dtype=torch.int32, device=eng.device)
    _ffi.check(lib.sai_pgen_decode(eng.ctx, eng._ptr(data), len(case["data"]), n_out, eng._ptr(rec), eng._ptr(base), eng._ptr(flip), case["n"], n_slots,
                                   None if first_col >= 0 else eng._ptr(cols), first_col, None if uniform else eng._ptr(ploidies), uniform,
                                   C.c_void_p(out.data_ptr()), out_row0, eng._ptr(status), stream()))  # fmt: skip
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def check_int8_block(got, status, case, out_row0, where):
    n_out = len(case["want"])
    assert np.array_equal(status, case["want_status"]), where
    assert np.array_equal(got[out_row0 : out_row0 + n_out], case["want"]), where
    assert (got[:out_row0] == 77).all() and (got[out_row0 + n_out :] == 77).all(), where  # the rows before out_row0 and behind the call


@pytest.mark.parametrize("form", ["run 1", "run 2", "list"])
@pytest.mark.parametrize("n", [70, 300])
def test_pgen_decode(eng, n_cu, cap, n, form):
    """2 * cap + 37 rows of every kind of record, every ordered pair of kinds one grid stride apart (damaged -> sound and
    sound -> damaged among them); the promised form at either ploidy with out_row0 no multiple of 16, and a column list
    with mixed ploidies; flips mixed."""
    rows = 2 * cap + G.PGEN_EXTRA_ROWS
    assert rows > 2 * DECODER_BLOCKS_PER_CU * n_cu
    case = G.pgen_decode_case(records_of(n), rows, cap, n - 9, form, seed=n)
    G.check_pgen_order(case["kinds"], case["order"], cap, case["level"])
    assert case["level"] == "fine" or cap < 16 * 16
    out_row0 = 5 if form != "list" else 0
    got, status = run_pgen_decode(eng, case, out_row0)
    check_int8_block(got, status, case, out_row0, (n, form))
    assert (status == G.BAD_RECORD).any() and (form != "run 1" or ((status > 0) & (status < G.BAD_RECORD)).any())


def test_pgen_decode_rows_wider_than_one_lds_window(eng, n_cu, cap):
    """16 384 + 600 samples, cap + 41 rows of a dozen distinct records (the first 41 blocks take a second row), a column
    list that spans both windows.  The one case that is not past 2 * cap: a row of two windows runs the tile loop twice
    per row, and what a row leaves for the next is already there when a block takes its second."""
    records = records_of(16384 + 600)
    rows = cap + 41
    assert rows > DECODER_BLOCKS_PER_CU * n_cu
    case = G.pgen_decode_case(records, rows, cap, 300, "list", seed=5)
    assert (case["cols"] < 16384).any() and (case["cols"] >= 16384).any()
    G.check_pgen_order(case["kinds"], case["order"], cap, case["level"])
    got, status = run_pgen_decode(eng, case, 3)
    check_int8_block(got, status, case, 3, "wide")
    assert (status == G.BAD_RECORD).any()


# ---- sai_pgen_pack2 ----


def run_pack_calls(call, case, cuts):
    """The calls [cuts[k], cuts[k + 1]) of the case's rows, each from its own out_row0; -> (block, status, unfit) with the
    entries of the sites before the first call in front."""
    row0 = case["out_row0"]
    for lo, hi in zip(cuts, cuts[1:]):
        got = call.run(row0 + lo, row0 + hi)
    return got, call.status.cpu().numpy(), call.unfit.cpu().numpy()


def check_packed(got, status, unfit, case, where):
    row0 = case["out_row0"]
    assert np.array_equal(status[row0:], case["want_status"]) and np.array_equal(unfit[row0:], case["want_unfit"]), where
    assert (status[:row0] == -5).all() and (unfit[:row0] == -5).all(), where  # the sites before out_row0 are nobody's
    assert np.array_equal(got, G.packed_block(case)), where


@pytest.mark.parametrize("ploidy", [1, 2])
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "general"])
@pytest.mark.parametrize("n_ind", [3, 70, 300])
def test_pgen_pack2(eng, n_cu, cap, n_ind, fast, ploidy):
    """The records and orders of ``test_pgen_decode`` from out_row0 = 64 k + 23 to the last site of a block whose site
    count is no multiple of 64 (the padding sites lie in the strided range); then a block of twice the rows written as
    two calls cut inside a tile, each call past 2 * cap."""
    import torch

    n = 300
    rows, row0 = 2 * cap + G.PGEN_EXTRA_ROWS, 2 * 64 + 23
    assert rows > 2 * DECODER_BLOCKS_PER_CU * n_cu
    for n_calls in (1, 2):
        case = G.pgen_pack2_case(records_of(n), n_calls * rows, cap, n_ind, fast, ploidy, seed=n_ind + n_calls, out_row0=row0)
        assert case["n_sites"] % 64 and (row0 + rows) % 64
        if n_calls == 1:
            G.check_pgen_order(case["kinds"], case["order"], cap, case["level"])
        lead = np.zeros((row0, 3), dtype=np.int64)  # the sites before out_row0: their table entries are never read
        call = PgenPackCall(eng, case["data"], np.vstack([lead, case["rec"]]), np.vstack([lead, case["base"]]),
                            np.concatenate([np.zeros(row0, np.uint8), case["flip"]]), n, case["cols"], case["first_col"], ploidy)  # fmt: skip
        got, status, unfit = run_pack_calls(call, case, [0, rows, 2 * rows][: n_calls + 1])
        check_packed(got, status, unfit, case, (n_ind, fast, ploidy, n_calls))
        assert (case["want_status"] == G.BAD_RECORD).any() and (case["want_unfit"].any() == (ploidy == 2))
        del call
    torch.cuda.synchronize()


# ---- sai_plink_decode, sai_eigenstrat_decode ----


def run_decode(eng, case, tail_rows=2):
    import torch

    from sai_amd import _ffi, _ffi_eigenstrat, _ffi_plink

    records, rib, flip, cols, ploidies = (dev(eng, case[k]) for k in ("records", "rib", "flip", "cols", "ploidies"))
    n_out, n_slots, first_col, uniform, out_row0 = len(case["rib"]), case["n_slots"], case["first_col"], case["uniform"], case["out_row0"]
    out = torch.full((out_row0 + n_out + tail_rows, n_slots), 77, dtype=torch.int8, device=eng.device)
    status = torch.full((n_out,), -5, dtype=torch.int32, device=eng.device)
    tail = (n_out, eng._ptr(rib), eng._ptr(flip), case["n_cols"], n_slots, None if first_col >= 0 else eng._ptr(cols), first_col,
            None if uniform else eng._ptr(ploidies), uniform, C.c_void_p(out.data_ptr()), out_row0, eng._ptr(status), stream())  # fmt: skip
    if case["kind"] == "bed":
        _ffi.check(_ffi_plink.load().sai_plink_decode(eng.ctx, eng._ptr(records), case["n_batch"], case["record_bytes"], *tail))
    else:
        _ffi.check(_ffi_eigenstrat.load().sai_eigenstrat_decode(eng.ctx, case["encoding"], eng._ptr(records), case["n_batch"], case["record_bytes"], *tail))
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("form", ["run 1", "run 2", "list"])
@pytest.mark.parametrize("n_slots", [2002, 17])
@pytest.mark.parametrize("kind", ["bed", "packed", "text"])
def test_int8_decoders(eng, n_cu, cap, kind, n_slots, form):
    """``sai_plink_decode`` and ``sai_eigenstrat_decode`` (packed and text): 2 * cap * 256 + 5 chunks of 16 output bytes
    from 173 distinct batch rows.  2 002 slots: rows straddle chunks; 17 slots: many rows per chunk and some two million
    per call.  The promised fast form at either ploidy, and a scattered column list with mixed ploidies; out_row0 such
    that the first chunk is shared; the heterozygous ploidy-1 status of every row."""
    case = G.decode_case(kind, n_slots, cap, form, seed=n_slots)
    assert case["n_chunks"] > 2 * DECODER_BLOCKS_PER_CU * n_cu * G.BLOCK_THREADS
    assert (case["out_row0"] * n_slots) % 16 and (len(case["rib"]) * n_slots) < 1 << 32
    got, status = run_decode(eng, case)
    check_int8_block(got, status, case, case["out_row0"], (kind, n_slots, form))
    assert status.any() == (form != "run 2")


# ---- sai_bed_pack2 ----


@pytest.mark.parametrize("ploidy", [1, 2])
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "general"])
@pytest.mark.parametrize("n_ind", [3, 513])
def test_bed_pack2(eng, n_cu, cap, n_ind, fast, ploidy):
    """3 individuals, one run of groups per tile: 2 * 4 * cap + 3 tiles, two to three units per wave.  513 individuals,
    nine groups = a run of 8 and a run of 1 with w_tail = 1: 4 * cap + 64 units, as wide a block as the test can afford
    (70 MB), so every wave takes one unit and the first 64 a second one -- past the cap, not past twice the cap.  Three
    ``row_in_batch`` entries outside the batch, the last tile partial."""
    n_tiles = G.bed_pack2_tiles(n_ind, cap)
    units = n_tiles * (1 if n_ind == 3 else 2)
    waves = BED_PACK2_WAVES_PER_BLOCK * DECODER_BLOCKS_PER_CU * n_cu
    assert units > (2 if n_ind == 3 else 1) * waves
    case = G.bed_pack2_case(n_ind, n_tiles, fast, ploidy, seed=n_ind)
    call = BedPackCall(eng, case["rows"], case["row_bytes"], case["rib"], case["flip"], case["n_cols"], case["cols"], case["first_col"], ploidy,
                       case["n_sites"])  # fmt: skip
    got = call.run(0, case["n_sites"])
    check_packed(got, call.status.cpu().numpy(), call.unfit.cpu().numpy(), case, (n_ind, fast, ploidy))
    assert (case["want_status"] == G.BAD_INDEX).sum() == 3 and case["n_sites"] % 64


# ---- the site family ----


@pytest.fixture(scope="module")
def n_sites(n_cu):
    n = G.site_count(SITE_TILES_PER_CU * n_cu)
    assert -(-n // 64) > 2 * SITE_TILES_PER_CU * n_cu  # tiles: past twice the largest grid of the family
    return n


_site_data = {}


def site_data(n_sites, sizes, raw):
    """(matrices, counts, DD terms [which of ref / tgt][source individual][site]) -- computed once, never changed."""
    key = (n_sites, sizes, raw)
    if key not in _site_data:
        mats = G.site_mats(n_sites, sizes, raw, seed=len(sizes) + 10 * raw)
        sources = np.concatenate(mats[2:], axis=1)
        dd = np.stack([G.absdiff_numpy(mats[which], sources) for which in (0, 1)])
        _site_data[key] = (mats, G.counts_numpy(mats), dd)
    return _site_data[key]


def check_planes_and_freq(eng, out, n_sites, mats, ploidy, specs, candidates, where, decides=True):
    """The planes word for word, and the stored target frequency bit for bit: count / (ploidy * called) in float64, at
    every site of a dense pass and at the candidates of a pass that stores those only (NaN elsewhere)."""
    decisions = oracle_decisions(mats[: 2 + len(specs[0][2])], ploidy, specs)
    want = G.planes_numpy(n_sites, specs, decisions, candidates)
    assert np.array_equal(out[1].cpu().numpy().view(np.uint64), want), where
    freq = G.freq_numpy(G.counts_numpy(mats[1:2])[0], ploidy[1])
    if candidates:
        stored = np.any([d[0] for d in decisions], axis=0)
        assert not stored.all()
        assert G.same_f64_all(eng.site_tgt_freq(out[1], out[0], n_sites).cpu().numpy(), np.where(stored, freq, np.nan)), where
    else:
        assert G.same_f64_all(out[0].cpu().numpy(), freq), where
    assert not decides or all(int(d[0].sum()) > 0 for d in decisions)  # raw values are frequencies outside [0, 1]: no candidate


def test_site_absdiff(eng, n_sites):
    """A source of 3 individuals is one launch of two rows and one of one; against the reference (5) and the target (23)."""
    mats, _, _ = site_data(n_sites, (5, 23, 3), True)
    src = eng.tile(mats[2])
    for which in (0, 1):
        got = eng.site_absdiff(eng.tile(mats[which]), src).cpu().numpy()
        assert np.array_equal(got, G.absdiff_numpy(mats[which], mats[2])), which


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "dosages"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("sizes", [(5, 23, 2), (5, 23, 1, 2)], ids=["2 source individuals", "3 source individuals"])
def test_site_pass_dd(eng, n_sites, sizes, fused, raw):
    """12 waves per CU with two source individuals, 8 with three: DD's rows, the counts, and from the fused form the
    planes and the candidates' frequencies, every site."""
    import torch

    from sai_amd import _ffi

    mats, want_counts, want_dd = site_data(n_sites, sizes, raw)
    pops = eng.tile_many(mats)
    n_src = len(sizes) - 2
    ploidy = [2] * len(sizes)
    specs = G.site_specs(n_src, 2) if fused else []
    sets = [_ffi.make_params(w, x, 0.9, y, anc) for w, x, y, anc in specs]
    counts = torch.zeros((len(pops), n_sites, 2), dtype=torch.int32, device=eng.device)
    out, ad = eng.site_pass_dd(pops, ploidy, sets, 2, n_src, counts=counts, freq_mode="candidates")
    assert np.array_equal(ad.cpu().numpy(), want_dd)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    if fused:
        check_planes_and_freq(eng, out, n_sites, mats, ploidy, specs, True, (sizes, raw), decides=not raw)


def test_site_counts(eng, n_sites):
    mats, want_counts, _ = site_data(n_sites, (5, 23, 1, 2), False)
    assert np.array_equal(eng.site_counts(eng.tile_many(mats)).cpu().numpy(), want_counts)
    mats, want_counts, _ = site_data(n_sites, (5, 23, 1, 2), True)
    assert np.array_equal(eng.site_counts(eng.tile_many(mats)).cpu().numpy(), want_counts)


@pytest.mark.parametrize("n_sets", [1, 5])
def test_site_pass(eng, n_sites, n_sets):
    """16 waves per CU with one parameter set, 12 with five."""
    import torch

    from sai_amd import _ffi

    mats, want_counts, _ = site_data(n_sites, (5, 23, 1, 2), False)
    pops, ploidy, specs = eng.tile_many(mats), [2] * 4, G.site_specs(2, n_sets)
    sets = [_ffi.make_params(w, x, 0.9, y, anc) for w, x, y, anc in specs]
    counts = torch.zeros((4, n_sites, 2), dtype=torch.int32, device=eng.device)
    out = eng.site_pass(pops, ploidy, sets, counts=counts)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    check_planes_and_freq(eng, out, n_sites, mats, ploidy, specs, False, n_sets)
    out = eng.site_pass(pops, ploidy, sets, freq_mode="candidates")
    check_planes_and_freq(eng, out, n_sites, mats, ploidy, specs, True, n_sets)


def test_site_pass_packed2(eng, n_sites):
    import torch

    from sai_amd import _ffi

    mats, want_counts, _ = site_data(n_sites, (5, 23, 1, 2), False)
    packed, ploidy, specs = [eng.pack2(p) for p in eng.tile_many(mats)], [2] * 4, G.site_specs(2, 2)
    sets = [_ffi.make_params(w, x, 0.9, y, anc) for w, x, y, anc in specs]
    counts = torch.zeros((4, n_sites, 2), dtype=torch.int32, device=eng.device)
    out = eng.site_pass_packed2(packed, ploidy, sets, counts=counts)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    check_planes_and_freq(eng, out, n_sites, mats, ploidy, specs, False, "packed2")


def test_site_family_on_moderately_wide_populations(eng, n_sites):
    """(270, 33, 2) individuals at the same site count, raw int8 values generated on the device; the reference is a
    torch integer reduction in int64: DD's terms from ``sai_site_absdiff`` and from the unfused ``sai_site_pass_dd``, and
    the counts from that pass and from ``sai_site_counts``."""
    import torch

    gen = torch.Generator(device=eng.device).manual_seed(270)
    mats = [torch.randint(-128, 128, (n_sites, n), generator=gen, device=eng.device, dtype=torch.int8) for n in (270, 33, 2)]
    pops = eng.tile_many(mats)
    want_counts = torch.stack([torch.stack([torch.where(m >= 0, m, torch.zeros_like(m)).sum(dim=1, dtype=torch.int64),
                                            (m >= 0).sum(dim=1, dtype=torch.int64)], dim=1) for m in mats])  # fmt: skip
    want_dd = torch.stack([torch.stack([(m.to(torch.int64) - mats[2][:, j : j + 1].to(torch.int64)).abs().sum(dim=1) for j in range(2)])
                           for m in mats[:2]])  # fmt: skip
    for which in (0, 1):
        assert torch.equal(eng.site_absdiff(pops[which], pops[2]).to(torch.int64), want_dd[which])
    counts = torch.zeros((3, n_sites, 2), dtype=torch.int32, device=eng.device)
    _, ad = eng.site_pass_dd(pops, [2, 2, 2], [], 2, 1, counts=counts)
    assert torch.equal(ad.to(torch.int64), want_dd) and torch.equal(counts.to(torch.int64), want_counts)
    assert torch.equal(eng.site_counts(pops).to(torch.int64), want_counts)
