"""np.sum's addition order on the GPU, both implementations, called through the C ABI on the inputs of
tests/sum_order_cases.py (test_sum_order_cases_cpu.py shows that these inputs tell numpy's order from a left-to-right
sum, from a tree that stops six levels down, from one without 8192-element pieces and from one with 136-element leaves).

sai_window_dd (numpy_sum / PairwiseNode, serial): every source-population size at which numpy's tree changes shape, 49
windows each, the per-individual differences AND their mean; window counts around the four windows of a workgroup; terms
and totals beyond int32 and uint32.  sai_window_fourpop (wave_numpy_sum, one wavefront per item): arbitrary doubles, all
seven sums and all four ratios of every (window, source) item, window lengths at the same sizes at three alignments,
workgroup counts below, at and above the eight of xcd_contiguous, zero denominators, NaN sites.  sai_site_freqs with
denominators beyond 2^31.  Every output buffer is prefilled with a NaN no kernel produces and none may be left: with as
many workgroups as groups of items, every item written means every item written once.  Every comparison is exact."""

import ctypes as C

import numpy as np
import pytest

import sum_order_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF8DEAD0000BEEF  # a NaN, but not the one the kernels or numpy write


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_doubles(got, want, where):
    """Bit for bit; NaN positions compared separately (any NaN is a NaN), and no sentinel left."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, where
    assert not (bits(got) == np.uint64(SENTINEL)).any(), (where, "unwritten", np.argwhere(bits(got).reshape(got.shape) == np.uint64(SENTINEL))[:5].tolist())
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (where, "NaN positions", np.argwhere(np.isnan(got) != nan)[:5].tolist())
    bad = np.argwhere((bits(got).reshape(got.shape) != bits(want).reshape(want.shape)) & ~nan)
    assert bad.size == 0, (where, len(bad), [(tuple(i), float(got[tuple(i)]).hex(), float(want[tuple(i)]).hex()) for i in bad[:5].tolist()])


def prefilled(eng, shape):
    import torch

    return torch.full(shape, SENTINEL, dtype=torch.int64, device=eng.device).view(torch.float64)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def bounds(eng, windows):
    import torch

    w = np.asarray(windows, dtype=np.int32).reshape(-1, 2)
    return torch.from_numpy(w[:, 0].copy()).to(eng.device), torch.from_numpy(w[:, 1].copy()).to(eng.device)


def run_dd(eng, ad_ref, ad_tgt, n_ref, n_tgt, windows):
    """sai_window_dd on uint32 terms handed over as the int32 tensors the engine uses: (scratch [W][n], dd [W])."""
    import torch

    from sai_amd import _ffi

    n, n_sites = ad_ref.shape
    d_ref = torch.from_numpy(np.ascontiguousarray(ad_ref).view(np.int32)).to(eng.device)
    d_tgt = torch.from_numpy(np.ascontiguousarray(ad_tgt).view(np.int32)).to(eng.device)
    lo, hi = bounds(eng, windows)
    scratch, dd = prefilled(eng, (len(windows), n)), prefilled(eng, (len(windows),))
    _ffi.check(eng.lib.sai_window_dd(eng.ctx, n_sites, n, ptr(d_ref), n_ref, ptr(d_tgt), n_tgt, len(windows), ptr(lo), ptr(hi),
                                     ptr(scratch), ptr(dd), eng._stream()))  # fmt: skip
    torch.cuda.synchronize()
    return scratch.cpu().numpy(), dd.cpu().numpy()


@pytest.mark.parametrize("n", sc.SIZES)
def test_window_dd_is_np_mean_at_every_tree_size(eng, n):
    ad_ref, ad_tgt = sc.dd_inputs(n)
    d, dd = sc.dd_expected(ad_ref, ad_tgt, sc.WINDOWS)
    scratch, got = run_dd(eng, ad_ref, ad_tgt, sc.N_REF, sc.N_TGT, sc.WINDOWS)
    assert_same_doubles(scratch, d, ("scratch", n))
    assert_same_doubles(got, dd, ("dd", n))
    empty = [i for i, (lo, hi) in enumerate(sc.WINDOWS) if hi <= lo]
    assert empty and not bits(got[empty]).any() and not bits(scratch[empty]).any()  # +0.0


@pytest.mark.parametrize("n_windows", [1, 3, 4, 5, 1001])
def test_window_dd_window_counts_around_a_workgroup(eng, n_windows):
    """Four windows per workgroup: a lone partial one, a full one, full ones and a partial last."""
    windows = sc.windows_of_count(n_windows)
    assert len(windows) == n_windows
    ad_ref, ad_tgt = sc.dd_inputs(9)
    d, dd = sc.dd_expected(ad_ref, ad_tgt, windows)
    scratch, got = run_dd(eng, ad_ref, ad_tgt, sc.N_REF, sc.N_TGT, windows)
    assert_same_doubles(scratch, d, ("scratch", n_windows))
    assert_same_doubles(got, dd, ("dd", n_windows))


def test_window_dd_reads_its_terms_unsigned(eng):
    """Terms at and around 255 * 2^24, 2^31 and 2^32 - 1 (bit patterns in an int32 tensor), 2^24 reference individuals,
    window totals up to 255 * 2^32; the expectation comes from Python integers."""
    ad_ref, ad_tgt, n_ref, n_tgt = sc.unsigned_inputs()
    d, dd, _ = sc.unsigned_expected(ad_ref, ad_tgt, n_ref, n_tgt, sc.WINDOWS)
    scratch, got = run_dd(eng, ad_ref, ad_tgt, n_ref, n_tgt, sc.WINDOWS)
    assert_same_doubles(scratch, d, "scratch")
    assert_same_doubles(got, dd, "dd")
    assert (d[0] > 0).all()  # a signed read of the terms would have made these negative


# ---- four populations ------------------------------------------------------------------------------------


def run_fourpop(eng, freqs, n_src, has_out, windows):
    """sai_window_fourpop: (sums [W][n_src][7], stats [W][n_src][4]) -- the sums are what Engine.window_fourpop drops."""
    import torch

    from sai_amd import _ffi

    d_freqs = torch.from_numpy(np.ascontiguousarray(freqs)).to(eng.device)
    lo, hi = bounds(eng, windows)
    sums, stats = prefilled(eng, (len(windows), n_src, 7)), prefilled(eng, (len(windows), n_src, 4))
    _ffi.check(eng.lib.sai_window_fourpop(eng.ctx, freqs.shape[1], n_src, 1 if has_out else 0, ptr(d_freqs), len(windows), ptr(lo),
                                          ptr(hi), ptr(sums), ptr(stats), eng._stream()))  # fmt: skip
    torch.cuda.synchronize()
    return sums.cpu().numpy(), stats.cpu().numpy()


def check_fourpop(eng, freqs, n_src, has_out, windows, where):
    want_sums, want_stats = sc.fourpop_expected(freqs, n_src, has_out, windows)
    sums, stats = run_fourpop(eng, freqs, n_src, has_out, windows)
    assert_same_doubles(sums, want_sums, (where, "sums"))
    assert_same_doubles(stats, want_stats, (where, "stats"))
    return sums, stats, want_sums, want_stats


def _n_src_values():
    from sai_amd import _ffi

    return [1, 3, _ffi.SAI_FUSED_SRC]


@pytest.mark.parametrize("has_out", [False, True], ids=["no_outgroup", "outgroup"])
@pytest.mark.parametrize("n_src", _n_src_values())
def test_window_fourpop_sums_and_ratios_at_every_tree_size(eng, n_src, has_out):
    """Window lengths at SIZES, each at lo % 8 = 0, 1 and 7, over 30 011 sites of arbitrary doubles: seven sums and
    four ratios per (window, source); the empty and the reversed window; windows over a NaN site."""
    freqs = sc.fourpop_freqs(n_src, has_out)
    windows = sc.fourpop_windows()
    sums, stats, want_sums, _ = check_fourpop(eng, freqs, n_src, has_out, windows, (n_src, has_out))
    for w in ((5, 5), (100, 37)):
        i = windows.index(w)
        assert not bits(sums[i]).any() and np.isnan(stats[i]).all()  # +0.0 sums, 0 / 0 ratios
    # the NaN windows: numpy's NaN slots and no others (assert_same_doubles), and they are the ones the case planted
    free = sc.FP_SITES - sc.FP_NAN_REGION
    one_source = np.isnan(sums[windows.index((free - 30, free + 20))]).all(axis=1).tolist()
    assert one_source == ([False, True] + [False] * (n_src - 2) if n_src > 1 else [True])
    assert not np.isnan(sums[windows.index((free + 10, free + 40))]).any()
    assert np.isnan(sums[windows.index((free + 30, free + 60))]).all()
    assert np.isnan(want_sums).any(axis=(1, 2)).sum() == 4


@pytest.mark.parametrize("wg,n_windows,n_src", sc.launch_shapes(), ids=[f"{s[0]}_workgroups" for s in sc.launch_shapes()])
def test_window_fourpop_every_item_once_at_every_launch_shape(eng, wg, n_windows, n_src):
    """1, 7, 8, 9, 17 and 43 workgroups of four items: every window has different content, so an item computed from
    another one's window, or never written, shows."""
    freqs = sc.fourpop_freqs(n_src, True, n_sites=sc.SHAPE_SITES, nan_region=0)
    windows = sc.shape_windows(n_windows)
    assert -(-n_windows * n_src // sc.constants()["kSumWaves"]) == wg
    _, _, want_sums, _ = check_fourpop(eng, freqs, n_src, True, windows, ("workgroups", wg))
    flat = want_sums.reshape(-1, 7)
    assert len({row.tobytes() for row in flat}) == len(flat)  # no two items expect the same sums


def test_window_fourpop_zero_denominators_are_nan(eng):
    f, n_src, has_out, windows = sc.zero_denominator_case()
    _, stats, _, want = check_fourpop(eng, f, n_src, has_out, windows, "zero denominators")
    assert not np.isinf(stats).any() and np.isnan(want).sum() == n_src * (2 * 3 + 3 * 2 + 1)


# ---- site frequencies --------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_sites", [1, 255, 256, 257])
@pytest.mark.parametrize("n_pops", [1, 9])
def test_site_freqs_is_a_float64_division(eng, n_pops, n_sites):
    """count / (called * ploidy) in f64 for one population and for the most the entry point admits, denominators up to
    255 * 2^24, NaN where nobody is called."""
    import torch

    from sai_amd import _ffi

    assert n_pops in (1, 2 + _ffi.SAI_FUSED_SRC + 1)
    counts, ploidy = sc.freq_counts(n_pops, n_sites)
    d_counts = torch.from_numpy(counts.view(np.int32)).to(eng.device)
    freqs = prefilled(eng, (n_pops, n_sites))
    pl = (C.c_int32 * n_pops)(*ploidy)
    _ffi.check(eng.lib.sai_site_freqs(eng.ctx, n_sites, n_pops, pl, ptr(d_counts), ptr(freqs), eng._stream()))
    torch.cuda.synchronize()
    assert_same_doubles(freqs.cpu().numpy(), sc.freq_expected(counts, ploidy), (n_pops, n_sites))
