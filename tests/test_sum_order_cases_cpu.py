"""tests/sum_order_cases.py checked without a GPU.

Three things are shown here.  (1) The SCHEME of wave_numpy_sum -- list the leaves of numpy's halving tree with an explicit
stack, sum each leaf as numpy sums at most 128 elements, rebuild the tree from the leaves' depths -- gives np.sum of
every piece size 1..8192 bit for bit, within the capacities fourpop.hip reserves (kMaxLeaves, kMaxDepth, 16-bit
lengths).  That is a statement about the scheme and the capacities, restated in Python from the source: it does not run
the HIP code, test_sum_order_device.py does.  (2) The expectations the device tests use are numpy's own and agree with
the oracle's operation-by-operation restatement.  (3) The inputs have teeth: at every size where a wrong addition order
can differ from numpy's, it does differ on at least two windows -- asserted, not measured."""

import numpy as np
import pytest

import sum_order_cases as sc
from conftest import same_f64
from oracle import sai_oracle as O

C = sc.constants()
MIN_DIFFERING = 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_constants_and_sizes_are_the_ones_the_cases_were_written_for():
    assert (C["leaf"], C["piece"], C["node_depth"]) == (128, 8192, 7)
    assert C["kMaxLeaves"] == 72 and C["kMaxDepth"] == 8 and C["kSumWaves"] == 4 and C["kPatternSlots"] == len(sc.SLOTS) == 7
    assert sc.SIZES == (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 255, 256, 257, 263, 1000, 2001, 4097, 7688, 7689,
                        7693, 8191, 8192, 8193, 8200, 16384 + 7700)  # fmt: skip
    assert (sc.SEVEN_LEVEL.start, sc.SEVEN_LEVEL.stop) == (7689, 8192)
    assert sc.WINDOWS[:9] == ((0, 256), (0, 63), (0, 64), (0, 65), (63, 129), (5, 5), (100, 37), (-9, 70), (150, 400))
    assert len(sc.WINDOWS) == 49 and all(0 <= lo <= 200 and 1 <= hi - lo <= 56 for lo, hi in sc.WINDOWS[9:])
    assert [s[0] for s in sc.launch_shapes()] == [1, 7, 8, 9, 17, 43]
    lo, hi = sc.clamp(sc.FIXED_WINDOWS, sc.DD_SITES)
    assert list(zip(lo.tolist(), hi.tolist())) == [(0, 256), (0, 63), (0, 64), (0, 65), (63, 129), (5, 5), (100, 100), (0, 70), (150, 256)]


def test_leaf_scheme_is_np_sum_for_every_piece_size_within_the_capacities():
    """The scheme and the capacities, not the HIP code (see the module docstring)."""
    a = np.random.default_rng(1).random(C["piece"]) ** 3
    most_leaves = deepest = highest = 0
    first_at_most = None
    for m in range(1, C["piece"] + 1):
        leaves, top = sc.list_leaves(0, m)
        assert [lf[0] for lf in leaves] == list(np.cumsum([0] + [lf[1] for lf in leaves[:-1]])) and sum(lf[1] for lf in leaves) == m
        assert all(0 < ln <= C["leaf"] for _, ln, _ in leaves)
        if m > C["leaf"]:
            assert min(ln for _, ln, _ in leaves) >= C["leaf"] // 2
        if len(leaves) > most_leaves:
            most_leaves, first_at_most = len(leaves), m
        deepest = max(deepest, max(d for _, _, d in leaves))
        highest = max(highest, top)
        # what the structure stores as short: lengths on the stack (up to the piece) and depths
        assert m <= np.iinfo(np.int16).max and all(off + ln <= m for off, ln, _ in leaves)
        got = sc.replay([np.sum(a[off : off + ln]) for off, ln, _ in leaves], [d for _, _, d in leaves], C["kMaxDepth"])
        assert same_f64(got, np.sum(a[:m])), m
    assert most_leaves <= C["kMaxLeaves"] and deepest <= C["kMaxDepth"] - 1 and highest <= C["kMaxDepth"]
    assert (most_leaves, first_at_most, deepest, highest) == (65, 7689, 7, 6)  # what the comments of fourpop.hip say
    assert deepest == C["node_depth"]  # numpy_sum.hpp unrolls its recursion exactly this far


def test_plain_python_tree_is_np_sum():
    """tree_sum (what the wrong orders are variations of) is numpy's order at every size of SIZES."""
    a = np.random.default_rng(2).random(max(sc.SIZES)) ** 3
    for n in sc.SIZES:
        assert same_f64(sc.tree_sum(a[:n]), np.sum(a[:n])), n
        assert same_f64(O.numpy_sum(a[:n]), np.sum(a[:n])), n


@pytest.fixture(scope="module")
def dd_cases():
    out = {}
    for n in sc.SIZES:
        ad_ref, ad_tgt = sc.dd_inputs(n)
        out[n] = sc.dd_expected(ad_ref, ad_tgt, sc.WINDOWS)
    return out


def test_dd_expectation_is_the_oracles_sum(dd_cases):
    lo, hi = sc.clamp(sc.WINDOWS, sc.DD_SITES)
    for n, (d, dd) in dd_cases.items():
        assert d.shape == (len(sc.WINDOWS), n) and d.flags.c_contiguous
        assert not d[hi == lo].any() and not dd[hi == lo].any() and not np.signbit(dd[hi == lo]).any()
        rows = range(len(sc.WINDOWS)) if n <= 2 * C["leaf"] + 7 or n in (7693, 8193) else (0, 9, 20)
        for w in rows:
            assert same_f64(O.numpy_sum(d[w]) / n, dd[w]), (n, w)
    ad_ref, ad_tgt = sc.dd_inputs(9)
    d = dd_cases[9][0]
    for w, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):  # the totals, the slow way
        tr, tt = ad_ref[:, a:b].astype(object).sum(axis=1), ad_tgt[:, a:b].astype(object).sum(axis=1)
        want = [float(int(x)) / sc.N_REF - float(int(y)) / sc.N_TGT for x, y in zip(np.atleast_1d(tr), np.atleast_1d(tt))] if b > a else [0.0] * 9
        assert bits(d[w]).tolist() == bits(want).tolist(), w


def test_dd_inputs_tell_every_wrong_order_from_numpys(dd_cases):
    """For every size at which a wrong order applies (left to right from 128 elements, six levels at 7689..8191, no
    pieces above 8192, 136-element leaves at 129..136), its mean differs from np.mean on at least two windows."""
    seen = set()
    for n in sc.SIZES:
        d, dd = dd_cases[n]
        for name, fn in sc.wrong_orders_for(n):
            differing = sum(not same_f64(fn(row) / n, want) for row, want in zip(d, dd))
            print(f"DD n={n} {name}: {differing} of {len(dd)} windows differ")
            assert differing >= MIN_DIFFERING, (n, name, differing)
            seen.add(name)
        if n > 2 * C["leaf"] + 7 and sc.wrong_orders_for(n):  # the machinery the wrong orders vary is right
            assert all(same_f64(sc.tree_sum(d[w]) / n, dd[w]) for w in (0, 9, 20)), n
    assert seen == {"left_to_right", "six_levels", "no_pieces", "wide_leaf"}


def test_golden_dd_cases_tell_the_wrong_orders_from_the_references_value():
    """The reference's DD of the large source populations (dd_cases.json) is none of the wrong orders' means: 129 and
    263 individuals against left to right and 136-element leaves, 7693 against left to right, six levels and
    4096-element pieces, 8193 against left to right and no pieces.  (4096-element pieces cannot show at 8192, 8193 or
    8200 elements: numpy's own first split of an 8192-element piece is at 4096.)"""
    from conftest import load_golden, unhex
    from test_oracle_golden import dd_case_inputs

    cases = {c["name"]: c for c in load_golden("dd_cases.json")}
    half_pieces = lambda a: sc.tree_sum(a, piece=C["piece"] // 2)  # noqa: E731
    wanted = {"dd_src_129_263": [(sc.left_to_right, sc.wide_leaf), (sc.left_to_right, sc.wide_leaf)],
              "dd_src_7693": [(sc.left_to_right, sc.six_levels, half_pieces)], "dd_src_8193": [(sc.left_to_right, sc.no_pieces)]}  # fmt: skip
    for name, per_source in wanted.items():
        ref, tgt, srcs = dd_case_inputs(cases[name])
        assert [s.shape[1] for s in srcs] == cases[name]["seeded"][4]
        for s, out, orders in zip(srcs, cases[name]["out"], per_source):
            s = s.astype(np.float64)
            d_ref = np.abs(s.T[:, None, :] - ref.T[None, :, :].astype(np.float64)).sum(axis=2)
            d_tgt = np.abs(s.T[:, None, :] - tgt.T[None, :, :].astype(np.float64)).sum(axis=2)
            d = np.mean(d_ref, axis=1) - np.mean(d_tgt, axis=1)
            assert same_f64(sc.tree_sum(d) / len(d), unhex(out)), name
            for fn in orders:
                assert not same_f64(fn(d) / len(d), unhex(out)), (name, len(d), fn)
    a = np.random.default_rng(12).random(8200) ** 3
    assert all(same_f64(half_pieces(a[:n]), np.sum(a[:n])) for n in (8192, 8193, 8200))


def test_unsigned_terms_are_above_every_signed_limit():
    ad_ref, ad_tgt, n_ref, n_tgt = sc.unsigned_inputs()
    assert n_ref == 1 << 24 and int(ad_ref.min()) >= (1 << 31) - 1 and (ad_ref == 255 << 24).sum() > sc.DD_SITES
    assert {(1 << 31) - 1, 1 << 31, (1 << 32) - 1} <= set(ad_ref[1].tolist())
    d, dd, totals = sc.unsigned_expected(ad_ref, ad_tgt, n_ref, n_tgt, sc.WINDOWS)
    # 256 terms of 32 bits stay below 2^40; the whole-block totals are 255 * 2^32 and thereabouts, far above 2^32
    assert all(t > 1 << 39 for t in totals[0]) and totals[0][0] == 256 * (255 << 24) == 255 << 32
    assert sum(min(t) > 1 << 32 for t in totals) > 30
    d2, dd2 = sc.dd_expected(ad_ref, ad_tgt, sc.WINDOWS, n_ref, n_tgt)  # the array route agrees with Python integers
    assert d.tobytes() == d2.tobytes() and dd.tobytes() == dd2.tobytes()
    signed = ad_ref.view(np.int32).astype(np.int64)[:, :256].sum(axis=1)
    assert (signed < 0).all()  # a kernel that read the terms as int32 would see these totals


@pytest.fixture(scope="module")
def fp_case():
    freqs = sc.fourpop_freqs(3, True)
    return freqs, sc.fourpop_windows(), sc.fourpop_expected(freqs, 3, True, sc.fourpop_windows())


def test_fourpop_inputs_are_what_they_say(fp_case):
    freqs, windows, (sums, stats) = fp_case
    assert freqs.shape == (6, sc.FP_SITES) and np.isnan(freqs).sum() == 4
    assert not np.isnan(freqs[:, : sc.FP_SITES - sc.FP_NAN_REGION]).any()
    ok = ~np.isnan(freqs)
    assert (freqs[ok] >= 0).all() and (freqs[ok] <= 1).all()
    for p in range(6):
        assert (freqs[p] == 0.0).sum() > 100 and (freqs[p] == 1.0).sum() > 100
    assert all((freqs[2 + k] == freqs[1]).sum() > 100 for k in range(3))
    mant = bits(freqs[0][(freqs[0] > 0) & (freqs[0] < 1)]) & np.uint64(0xFF)
    assert np.unique(mant).size == 256  # the low mantissa bits are in use
    lens = {(hi - lo, lo % 8) for lo, hi in windows if hi > lo >= 0 and hi <= sc.FP_SITES - sc.FP_NAN_REGION}
    assert all((n, r) in lens for n in sc.SIZES for r in sc.FP_OFFSETS)
    # NaN exactly where a NaN site lies in the window, in that source's items only
    free = sc.FP_SITES - sc.FP_NAN_REGION
    by_window = {w: np.isnan(sums[i]).all(axis=1).tolist() for i, w in enumerate(windows)}
    assert np.array_equal(np.isnan(sums).any(axis=2), np.isnan(sums).all(axis=2))
    assert by_window[(free - 30, free + 20)] == [False, True, False]
    assert by_window[(free + 10, free + 40)] == [False, False, False]
    assert by_window[(free + 30, free + 60)] == by_window[(free + 70, free + 100)] == by_window[(free + 110, sc.FP_SITES + 50)] == [True] * 3
    assert sum(any(v) for v in by_window.values()) == 4
    for w in ((5, 5), (100, 37)):
        i = windows.index(w)
        assert not sums[i].any() and not np.signbit(sums[i]).any() and np.isnan(stats[i]).all()


def test_fourpop_expectation_is_the_oracles(fp_case):
    freqs, windows, (sums, stats) = fp_case
    for i in (0, 40, len(windows) - 8):
        lo, hi = windows[i]
        for k in range(3):
            r, t, s, o = freqs[0, lo:hi], freqs[1, lo:hi], freqs[2 + k, lo:hi], freqs[5, lo:hi]
            d = np.maximum(t, s)
            want = [O.pattern_sum(r, t, s, o, p) for p in sc.SLOTS[:5]] + [O.pattern_sum(r, d, d, o, "abba"), O.pattern_sum(r, d, d, o, "baba")]
            assert bits(sums[i, k]).tolist() == bits(want).tolist()


def test_fourpop_inputs_tell_every_wrong_order_from_numpys(fp_case):
    """Per window length at 129..136, 7689..8191 and above 8192: the (window, source) items on which a wrong order's
    seven sums are not all numpy's are at least two."""
    freqs, windows, (sums, _) = fp_case
    seen = set()
    for n in sc.SIZES:
        orders = [(name, fn) for name, fn in sc.wrong_orders_for(n) if name != "left_to_right" or n <= C["leaf"] + 8]
        if n <= C["leaf"]:
            continue
        for name, fn in orders:
            differing = total = 0
            for i, (lo, hi) in enumerate(windows):
                if hi - lo != n or lo < 0:
                    continue
                for k in range(3):
                    prods = sc.window_products(freqs, 3, True, k, lo, hi)
                    differing += any(not same_f64(fn(row), want) for row, want in zip(prods, sums[i, k]))
                    total += 1
            print(f"fourpop n={n} {name}: {differing} of {total} items differ")
            assert differing >= MIN_DIFFERING, (n, name, differing, total)
            seen.add(name)
    assert seen == {"left_to_right", "six_levels", "no_pieces", "wide_leaf"}


def test_zero_denominator_case_has_zero_denominators():
    f, n_src, has_out, windows = sc.zero_denominator_case()
    sums, stats = sc.fourpop_expected(f, n_src, has_out, windows)
    nan = np.isnan(stats)
    assert not np.isinf(stats).any() and not np.isnan(sums).any()
    for w in (0, 1, 2):  # tgt = src = 0: only baaa is left
        assert nan[w].tolist() == [[True, True, False, False]] * n_src and (stats[w, :, 2:] == 1.0).all()
        assert (sums[w][:, [0, 1, 2, 4, 5, 6]] == 0).all() and (sums[w][:, 3] > 0).all()
    for w in (3, 4):  # ref = tgt = 1: only bbaa is left
        assert nan[w].tolist() == [[True, False, True, True]] * n_src and (stats[w, :, 1] == 0.0).all()
    for w in (5, 6):
        assert not nan[w].any()
    assert nan[7].tolist() == [[True, False, False, False]] * n_src  # half of each kind: only fd's donor sums stay zero


def test_frequency_counts_reach_past_int32():
    for n_pops in (1, 9):
        for n_sites in (1, 255, 256, 257):
            counts, ploidy = sc.freq_counts(n_pops, n_sites)
            want = sc.freq_expected(counts, ploidy)
            called = counts[:, :, 1].astype(np.int64)
            assert counts[0, 0].tolist() == [255 << 24, 1 << 24] and want[0, 0] == 1.0 and ploidy[0] == 255
            assert np.array_equal(np.isnan(want), called == 0)
            ok = called > 0
            assert (want[ok] >= 0).all() and (want[ok] <= 1).all()
            if n_sites >= 255:
                assert (called == 0).any() and ((called[0] * 255) > 1 << 31).any()
                assert (counts[0, :, 0].astype(np.int64) > 1 << 31).any()  # numerators too
