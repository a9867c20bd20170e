"""The inputs of tests/capacity_cases.py sit where they say: every quantity a window case claims (tiles spanned,
row words, stored frequencies over the spanned tiles, condition sites per set, the rank the quantile wants and
the members of the first-digit bin that holds it) is recomputed here from the matrices with the numpy oracle, and
the stream cases are shown to be the worst case of the packed accumulators by plain int64 arithmetic.  No GPU."""

import numpy as np
import pytest

import capacity_cases as cc
from oracle import sai_oracle as O

CASES = cc.window_cases()


def test_constants_are_read_from_the_sources():
    c = cc.constants()
    assert set(c) == {"kWaveCap", "kFreqCap", "kLdsTiles", "kRowWords", "kListCap", "kWinWaves", "kChunkIters", "kUnroll", "kTableFromSets"}
    assert all(isinstance(v, int) and v > 0 for v in c.values())
    # the parser: plain values, expressions of earlier names, and nothing that is not an integer expression
    got = cc.parse_constants("constexpr int kA = 256;\n  constexpr int kB = kA / 64;  // waves\nconstexpr int kC = (1 << 8) + 1;\n"
                             "constexpr int kD = SAI_TILE_SITES;\nconstexpr double kE = 1.5;\n")  # fmt: skip
    assert got == {"kA": 256, "kB": 4, "kC": 257}
    # what the builders assume about how the capacities relate (windows.hip: a list entry per stored frequency)
    assert c["kListCap"] >= c["kFreqCap"] and c["kFreqCap"] % cc.TILE == 0 and c["kWaveCap"] < c["kFreqCap"] // 2


def recompute(case):
    """Per window the claimed quantities, from the matrices: the oracle's condition and effective target frequency
    per site and set, the union per tile, lo / hi from the positions, the rank from (n - 1) * q."""
    ref, tgt, *srcs = [m.astype(np.int64) for m in case.mats]
    n_sites = ref.shape[0]
    conds, effs = [], []
    for s in case.specs:
        _, tf, cond = O.matching_loci(ref, tgt, srcs, s["w"], s["y_list"], case.ploidy, s["anc"])
        conds.append(cond)
        effs.append(tf)
    union = np.any(conds, axis=0)
    n_tiles = (n_sites + 63) // 64
    per_tile = np.zeros(n_tiles * 64, dtype=np.int64)
    per_tile[:n_sites] = union
    per_tile = per_tile.reshape(n_tiles, 64).sum(axis=1)
    used = 1 + len(case.specs) * (2 if any(not s["anc"] for s in case.specs) else 1)
    out = []
    for (ws, we), (lo_c, hi_c) in zip(case.windows, case.ranges):
        lo, hi = int(np.searchsorted(case.pos, ws, side="left")), int(np.searchsorted(case.pos, we, side="right"))
        assert (lo, hi) == (lo_c, hi_c)
        t0, t1 = lo // 64, -(-hi // 64)
        rec = dict(nt=t1 - t0, row_words=(t1 - t0) * used, stored=int(per_tile[t0:t1].sum()), n_cond=[], k0=[], members=[], gap=[])
        for s, cond, eff in zip(case.specs, conds, effs):
            v = np.sort(eff[lo:hi][cond[lo:hi]])
            rec["n_cond"].append(int(v.size))
            if v.size == 0:
                for key in ("k0", "members", "gap"):
                    rec[key].append(None)
                continue
            virt = np.float64(v.size - 1) * np.float64(s["quantile"])
            take_max = bool(virt >= v.size - 1)
            k0 = v.size - 1 if take_max else int(np.floor(virt))
            digit = np.where(v == 1.0, 256, np.floor(v * 256.0)).astype(np.int64)
            rec["k0"].append(k0)
            rec["members"].append(int(np.count_nonzero(digit == digit[k0])))
            rec["gap"].append(None if take_max or k0 + 1 >= v.size else int(digit[k0 + 1] - digit[k0]))
            # ... and the oracle's quantile is the interpolation between exactly these two order statistics
            want = v[k0] if take_max else O.linear_quantile(v, s["quantile"])
            assert np.float64(want).tobytes() == np.float64(np.nanquantile(v, s["quantile"])).tobytes()
        out.append(rec)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_window_case_sits_where_it_claims(case):
    got = recompute(case)
    assert len(got) == len(case.claims) == len(case.windows) > 0
    for w, (g, claim) in enumerate(zip(got, case.claims)):
        assert g == claim, (case.name, w)
    assert case.pins, "a case is about some limit"
    for key, w, s, value in case.pins:
        have = got[w][key] if s is None else got[w][key][s]
        assert have == value, (case.name, key, w, s, have, value)
    assert case.used == got[0]["row_words"] // got[0]["nt"]
    assert all(m.dtype == np.int8 for m in case.mats) and len(case.pos) == case.mats[0].shape[0] <= 20_000
    assert max(hi - lo for lo, hi in case.ranges) <= 8_400


def _pinned(key):
    """{value: set of lo % 64} over all cases' pins of one quantity."""
    seen = {}
    for case in CASES:
        for k, w, _, value in case.pins:
            if k == key:
                seen.setdefault(value, set()).add(case.ranges[w][0] % 64)
    return seen


def test_every_capacity_is_met_and_passed_aligned_and_mid_tile():
    c = cc.constants()
    offs = {0, 1, 63}
    n_cond = _pinned("n_cond")
    for v in (c["kWaveCap"] - 1, c["kWaveCap"], c["kWaveCap"] + 1, 1, 2):
        assert n_cond.get(v, set()) >= offs, v
    stored = _pinned("stored")
    assert stored[c["kFreqCap"]] >= offs and stored[c["kFreqCap"] + 1] >= offs
    members = _pinned("members")
    assert members[c["kWaveCap"]] >= offs and members[c["kWaveCap"] + 1] >= offs
    nt, words = _pinned("nt"), _pinned("row_words")
    assert nt[c["kLdsTiles"]] >= offs and nt[c["kLdsTiles"] + 1] >= offs
    for n_sets, anc in ((7, True), (4, False), (20, False), (20, True)):
        used = 1 + n_sets * (1 if anc else 2)
        at = c["kRowWords"] // used * used
        assert at <= c["kRowWords"] < at + used and words[at] >= offs and words[at + used] >= offs, used
    assert _pinned("gap").keys() >= {0, 2} and _pinned("gap")[2] >= offs and _pinned("gap")[0] >= offs
    # the shared form needs kWinWaves sets, and a wave that answers a second set from the same slice one more
    assert all(len(case.specs) >= c["kWinWaves"] for case in CASES)
    assert any(len(case.specs) > c["kWinWaves"] for case in CASES if case.name.startswith("ncond"))
    # the list of LDS slots is full exactly at the limit: the heavy set of the aligned window holds kListCap sites
    heavy = {case.name: case for case in CASES}[f"freqcap_heavy_{c['kFreqCap']}"]
    assert heavy.claims[0]["n_cond"][0] == c["kListCap"] == heavy.claims[0]["stored"]
    union = {case.name: case for case in CASES}[f"freqcap_union_{c['kFreqCap']}"]
    assert all(max(cl["n_cond"]) <= 600 for cl in union.claims)
    inverted = {case.name: case for case in CASES}[f"freqcap_inverted_{c['kFreqCap']}"]
    assert not any(s["anc"] for s in inverted.specs) and int((inverted.mats[0] == 2).all(axis=1).sum()) > 400
    # the partial last tile of a block
    assert {case.mats[0].shape[0] % 64 for case in CASES if case.name.startswith("block_edge")} == {1, 63}
    assert all(hi == case.mats[0].shape[0] for case in CASES if case.name.startswith("block_edge") for _, hi in case.ranges)


def test_stream_sizes_surround_the_multi_switch():
    c = cc.constants()
    m = 16 * c["kChunkIters"]
    sizes = cc.stream_sizes()
    assert len(sizes) == 10 and {m - 1, m, m + 1, 2 * m, 2 * m + 1} <= set(sizes) and sizes == sorted(sizes)
    # what the comments of the kernels state about the packed fields, from the parsed values
    assert c["kChunkIters"] % c["kUnroll"] == 0 and c["kChunkIters"] + c["kUnroll"] <= 255
    assert 255 * (c["kChunkIters"] + c["kUnroll"]) < 2**16


@pytest.mark.parametrize("n_ind", cc.stream_sizes())
def test_stream_rows_are_the_worst_case(n_ind):
    g = cc.stream_rows(n_ind)
    assert g.shape == (cc.STREAM_SITES, n_ind) and g.dtype == np.int8 and cc.STREAM_SITES % 64 == 2
    total, called = cc.counts_reference(g)
    assert total.dtype == np.int64 and called.dtype == np.int64
    src = cc.stream_sources(3)
    ad = cc.absdiff_reference(g, src)
    assert ad.dtype == np.int64 and ad.shape == (3, cc.STREAM_SITES)
    seen = set()
    for site in range(cc.STREAM_SITES):
        p = cc.stream_pattern_of_site(site)
        seen.add(p)
        name = cc.STREAM_PATTERNS[p]
        if name == "all 127":
            assert (total[site], called[site]) == (127 * n_ind, n_ind)
            assert ad[1, site] == 255 * n_ind  # against the constant -128 source: every |a - b| is 255
            assert ad[2, site] in (255 * n_ind, 0)
        elif name in ("all -128", "all -1"):
            assert (total[site], called[site]) == (0, 0)
            if name == "all -128":
                assert ad[0, site] == 255 * n_ind and ad[2, site] in (255 * n_ind, 0)
        elif name == "all 63":
            assert (total[site], called[site]) == (63 * n_ind, n_ind)
        elif "/" in name:
            n127 = (n_ind + 1) // 2 if name.startswith("127") else n_ind // 2
            assert (total[site], called[site]) == (127 * n127, n127)
            assert ad[0, site] == 255 * (n_ind - n127) and ad[1, site] == 255 * n127
        else:
            assert (total[site], called[site]) == (127 * (n_ind - 1), n_ind - 1)
    assert seen == set(range(len(cc.STREAM_PATTERNS)))
    assert (ad[2] == 255 * n_ind).sum() >= 4  # the alternating source meets rows of its opposite as well
    # a whole tile below 64 (the bytewise group sums), and missing calls at the individuals the issue names
    assert (g[64:128] == 63).all()
    for p, ind in zip(range(6, 10), (0, 15, 16, n_ind - 1)):
        rows = [s for s in range(64) if cc.stream_pattern_of_site(s) == p]
        assert rows and all(g[s, ind] == -1 and (g[s] == -1).sum() == 1 for s in rows)
    pk = cc.packed_rows(n_ind)
    assert pk.max() == 2 and pk.min() == -1 and (pk == 2).all(axis=1).any() and (pk == -1).all(axis=1).any()
    alt = [(pk[s, 0], pk[s, 1]) for s in range(cc.STREAM_SITES) if len(set(pk[s].tolist())) == 2]
    assert {(2, -1), (-1, 2)} <= set(alt)
