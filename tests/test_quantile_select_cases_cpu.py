"""Proof, without a GPU, that the inputs of tests/quantile_select_cases.py are what they say: every case is on the
route, at the depth and on the value source its name claims (restated with exact digits from fractions.Fraction),
all depths, rank positions and interpolation arms occur, the hand-placed doubles are the neighbours and the
digit-sharing pairs they are meant to be, the arrays follow the storage layout of saihip.h -- and a select that is
wrong in one of four ways would change the expected Q or n_cdd_q of these very inputs."""

from fractions import Fraction

import numpy as np
import pytest

import quantile_select_cases as qc
from capacity_cases import parse_constants

C = qc.constants()
SCENARIOS = qc.scenarios()
NAMES = [s.name for s in SCENARIOS]


def test_constants_are_read_from_the_source():
    text = (qc.CSRC / "windows.hip").read_text()
    found = parse_constants(text)
    for name in ("kWaveCap", "kDigitBits", "kMaxLevels", "kListCap", "kFreqCap", "kRowWords", "kLdsTiles", "kWinWaves"):
        assert C[name] == found[name] > 0
    assert qc.base() ** C["kMaxLevels"] >= 2**112  # 14 levels hold every bit of a double >= 2^-55, the 15th is spare
    assert C["kListCap"] >= C["kFreqCap"]  # a set of the list way never exceeds its list: n_c <= stored <= kFreqCap


def test_digits_are_an_exact_monotone_code():
    """digit_on_path's claim, checked on the hand-placed values: the digits spell the value (lossless), and their
    order is the order of the values (monotone)."""
    values = sorted({g.eff for s in SCENARIOS for g in s.groups})
    assert len(values) > 300
    codes = [qc.digits(v) for v in values]
    for v, code in zip(values, codes):
        assert sum(Fraction(d, qc.base() ** (i + 1)) for i, d in enumerate(code)) == Fraction(v), v
        assert all(0 <= d < qc.base() for d in code[1:]) and 0 <= code[0] <= qc.base()
    assert codes == sorted(codes) and len(set(codes)) == len(codes)


@pytest.mark.parametrize("kind", ["plain", "rich"])
@pytest.mark.parametrize("L", qc.DEPTHS)
def test_pairs_share_exactly_L_digits(kind, L):
    a, b = qc.pair_values(kind, L)
    if kind == "plain":  # the issue's own pairs
        assert a == (0.5 if L <= 6 else 2.0**-55)
        assert b == a + 2.0 ** -min(8 * (L + 1), 53 if L <= 6 else 107) and b > a
    assert qc.shared_digits(a, b) == L
    assert qc.digits(a)[L] < qc.digits(b)[L]
    for weight in ("heavy", "light"):
        sc = qc.scenario(f"{kind}{L}_{weight}")
        assert sc.pairs == [(a, b, L)]
        count = {g.role: g.count for g in sc.groups}
        if weight == "heavy":
            assert min(count["a"], count["b"]) > C["kWaveCap"]
        else:
            assert max(count["a"], count["b"]) <= C["kWaveCap"] < count["a"] + count["b"]
        # decoys: the level in the role's name is the level at which the value leaves the pair's path
        for g in sc.groups:
            if g.role.startswith(("below", "above")):
                level = int(g.role[5:])
                assert level < L and qc.shared_digits(g.eff, a) == level
                assert (g.eff < a) == g.role.startswith("below")


def test_decoys_leave_the_path_below_and_above_at_every_level():
    below, above = set(), set()
    for sc in SCENARIOS:
        for g in sc.groups:
            if g.role.startswith("below"):
                below.add(int(g.role[5:]))
            if g.role.startswith("above"):
                above.add(int(g.role[5:]))
    assert below == set(range(13)) and above == set(range(13))


def test_one_ulp_pairs_are_neighbours():
    seen = []
    for sc in SCENARIOS:
        for a, b in sc.ulp_pairs:
            assert np.nextafter(np.float64(a), np.float64(2.0)) == np.float64(b), (sc.name, a, b)
            seen.append(sc.name)
    for name in ("plain6_heavy", "plain13_light", "rich6_light", "rich13_heavy", "inverted_third_heavy", "direct_256"):
        assert name in seen
    assert np.float64(1.0) - np.float64(1.0 / 3.0) == np.nextafter(np.float64(2.0 / 3.0), np.float64(1.0))
    assert qc.shared_digits(2.0 / 3.0, float(np.float64(1.0) - np.float64(1.0 / 3.0))) == 6


def test_every_value_is_an_admissible_frequency():
    for sc in SCENARIOS:
        for g in sc.groups:
            for v in (g.v, g.eff):
                assert 0.0 <= v <= 1.0 and (v == 0.0 or v >= 2.0**-55), (sc.name, g)
        eff = [g.eff for g in sc.groups]
        assert eff == sorted(eff), sc.name
        twice = [(a, b) for a, b in zip(sc.groups, sc.groups[1:]) if a.eff == b.eff]  # only 1 - 0.0 next to 1.0
        assert all(a.inverted != b.inverted for a, b in twice) and len(twice) == (sc.name == "inverted_zero")


def _position(r) -> set:
    """What the wanted rank is in the bin that is gathered (in a bin of one it is the first and the last member)."""
    out = ({"first"} if r.rank_in_bin == 0 else set()) | ({"last"} if r.rank_in_bin == r.members - 1 else set())
    return out or {"interior"}


def _arm(r):
    if r.take_max:
        return "max"
    if r.k0 == 0 and r.g == 0:
        return "min"
    return "exact" if r.g == 0 else "below_half" if r.g < Fraction(1, 2) else "half" if r.g == Fraction(1, 2) else "above_half"


@pytest.mark.parametrize("name", NAMES)
def test_every_case_is_where_its_name_says(name):
    """Route, depth, value source, rank position and arm of every (set, window) of the scenario in all four ways; the
    x of a query is one of the two order statistics around the wanted rank."""
    sc = qc.scenario(name)
    for way in qc.WAYS:
        case = qc.case(name, way)
        asked = []
        for call in case.calls:
            assert 1 <= call.n_sets <= qc.MAX_SETS and 2 <= call.lo.size <= 6
            assert (call.n_sets < C["kWinWaves"]) == (way == "wave")
            assert call.planes.shape == (call.n_sites // qc.TILE, qc.PLANES_PER_SET * call.n_sets)
            for s, what in enumerate(call.query):
                for w in range(call.lo.size):
                    assert 600 <= int(call.hi[w] - call.lo[w]) <= 2500
                    values = call.values(s, w)
                    route, depth, source = qc.route_of(call, s, w)
                    assert source == way, (name, way, s, w, source)
                    if isinstance(what, str):
                        assert route == 1 and values.size == {"light": 5, "empty": 0, "flipped": 6}[what]
                        continue
                    q = sc.queries[what]
                    assert np.array_equal(np.sort(values), sc.sorted_eff()), (name, way, s, w)
                    assert (route, depth) == (q.route, q.depth), (name, way, s, w, route, depth)
                    r = qc.route_of_values(values, q.quantile)
                    assert q.position in _position(r), (name, s, w, q.position, r)
                    assert _arm(r) == q.arm or (_arm(r), q.arm) == ("min", "exact"), (name, s, w, q.arm, r)  # rank 0 with g = 0 is both
                    srt = np.sort(values)
                    assert q.x in srt, (name, s, w)  # U's "> x" and ">= x" differ on these values
                    if q.arm not in ("min", "max"):
                        assert q.x in (srt[r.k0], srt[r.k0 + 1]), (name, s, w)
                    assert call.sets[s]["x"] == q.x and call.sets[s]["quantile"] == q.quantile
                asked += [what for what in call.query[s : s + 1] if not isinstance(what, str)]
        assert sorted(asked) == list(range(len(sc.queries))), (name, way)  # every query runs, in every way


def test_all_depths_positions_arms_and_sources_occur():
    last = qc.last_level()
    seen = set()
    for sc in SCENARIOS:
        for q in sc.queries:
            seen.add((q.route, q.depth, q.position, q.arm))
    depths = {(route, depth) for route, depth, _, _ in seen}
    assert {(2, 0)} | {(3, d) for d in range(1, 14)} | {(3, last), (1, None)} == depths
    assert last == 14
    for depth in [(2, 0)] + [(3, d) for d in range(1, 14)] + [(3, last)]:
        here = {(p, a) for r, d, p, a in seen if (r, d) == depth}
        assert {p for p, _ in here} >= {"first", "last"}, depth
        assert {a for _, a in here} >= {"exact", "half"}, depth
    for route in (2, 3):
        here = {(p, a) for r, _, p, a in seen if r == route}
        assert {p for p, _ in here} == {"first", "last", "interior"}
        assert {a for _, a in here} == {"min", "max", "exact", "below_half", "half", "above_half"}, route
    # every deep level with both arms of the lerp at the last member of its bin
    for d in list(range(1, 14)) + [last]:
        assert {a for r, dd, p, a in seen if (r, dd, p) == (3, d, "last")} >= {"half", "above_half"}, d
    assert len(qc.case_ids()) == len(SCENARIOS) * len(qc.WAYS)


def test_route_two_inputs():
    cap = C["kWaveCap"]

    def first_bins(sc):
        d = np.array([qc.digits(float(v))[0] for v in sc.sorted_eff()])
        return {int(k): int(c) for k, c in zip(*np.unique(d, return_counts=True))}

    assert first_bins(qc.scenario(f"bin_{cap}"))[100] == cap and first_bins(qc.scenario(f"bin_{cap + 1}"))[100] == cap + 1
    assert {q.route for q in qc.scenario(f"bin_{cap}").queries} == {2}
    assert (3, 1) in {(q.route, q.depth) for q in qc.scenario(f"bin_{cap + 1}").queries}
    for name, nxt in (("gap_to_107", 107), (f"gap_to_{qc.base()}", qc.base())):
        bins = first_bins(qc.scenario(name))
        assert 100 in bins and min(k for k in bins if k > 100) == nxt
        if nxt == qc.base():
            assert qc.scenario(name).sorted_eff().max() == 1.0
    for name, want in (("own_3", {3, 4, 5, 6}), ("own_253", {253, 254, 255, 256})):
        sc = qc.scenario(name)
        assert set(first_bins(sc)) == want
        hit = set()
        for q in sc.queries:
            r = qc.route_of_values(sc.sorted_eff(), q.quantile)
            hit.add((qc.digits(float(sc.sorted_eff()[r.k0]))[0], "last" if r.rank_in_bin == r.members - 1 else "other"))
        assert {d for d, _ in hit} == want
        assert {d for d, p in hit if p == "last"} >= want - {max(want)}  # x1 is read from the bin of the next lane
    assert {4 // 5, 5 // 5} == {0, 1} and {254 // 5, 255 // 5, 256 // 5} == {50, 51}  # owners in bin_of_rank


def test_inverted_cases_hand_over_plain_v():
    third = qc.scenario("inverted_third_heavy")
    flipped = [g for g in third.groups if g.inverted]
    assert any(g.v == 1.0 / 3.0 and g.count > C["kWaveCap"] for g in flipped)
    assert any(g.v == 2.0 / 3.0 and not g.inverted and g.count > C["kWaveCap"] for g in third.groups)
    zero = qc.scenario("inverted_zero")
    assert any(g.v == 0.0 and g.inverted and g.eff == 1.0 for g in zero.groups) and any(g.v == 1.0 and not g.inverted for g in zero.groups)
    assert qc.digits(1.0)[0] == qc.base()
    for name in ("inverted_third_heavy", "inverted_third_light", "inverted_zero"):
        for way in qc.WAYS:
            for call in qc.case(name, way).calls:
                main = [s for s, what in enumerate(call.query) if not isinstance(what, str)]
                assert call.with_inv and all(not call.sets[s]["anc"] for s in main)
                n = call.n_sets
                for s in main:
                    assert call.inv[s].any() and (call.planes[:, 1 + n + s] != 0).any()
                    lo, hi = int(call.lo[0]), int(call.hi[0])
                    m = call.cond[s, lo:hi] & call.inv[s, lo:hi]
                    assert set(call.v_site[lo:hi][m]) <= {g.v for g in qc.scenario(name).groups if g.inverted}


@pytest.mark.parametrize("way", qc.WAYS)
def test_storage_layout(way):
    """saihip.h: bit b of a row's word = site 64 t + b; a tile's stored frequencies packed in its first popcount(any)
    slots.  Here "any" is a strict superset of the conditions and NaN fills whatever no set selects."""
    windows_inside_a_tile = 0
    for name in ("plain6_heavy", "rich13_light", "bin_256", "direct_40", "inverted_third_light", "last_one"):
        for call in qc.case(name, way).calls:
            n, n_tiles = call.n_sets, call.n_sites // qc.TILE
            words = call.planes.view(np.uint64)
            bit = lambda col: ((words[:, col, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)  # noqa: E731
            any_bits = bit(0)
            assert np.array_equal(any_bits, call.any)
            union = np.zeros(call.n_sites, bool)
            for s in range(n):
                assert np.array_equal(bit(1 + s), call.cond[s])
                if call.with_inv:
                    assert np.array_equal(bit(1 + n + s), call.inv[s]) and not (call.inv[s] & ~call.cond[s]).any()
                union |= call.cond[s]
            assert not words[:, call.used :].any()
            assert not (union & ~any_bits).any() and (any_bits & ~union).any()
            for w in range(call.lo.size):
                lo, hi = int(call.lo[w]), int(call.hi[w])
                t0, t1 = lo // qc.TILE, (hi + qc.TILE - 1) // qc.TILE
                assert (any_bits[t0 * qc.TILE : t1 * qc.TILE] & ~union[t0 * qc.TILE : t1 * qc.TILE]).any(), "strict superset in the window"
                windows_inside_a_tile += lo % qc.TILE != 0 and hi % qc.TILE != 0
                # condition sites right outside the window, in its edge tiles or next to them
                assert all(call.cond[s, hi] for s, what in enumerate(call.query) if not isinstance(what, str))
            tgt = call.tgt_freq.reshape(n_tiles, qc.TILE)
            for t in range(n_tiles):
                stored = np.flatnonzero(any_bits[t * qc.TILE : (t + 1) * qc.TILE]) + t * qc.TILE
                assert np.isnan(tgt[t, stored.size :]).all()
                got, sel = tgt[t, : stored.size], union[stored]
                assert np.isnan(got[~sel]).all() and np.array_equal(got[sel], call.v_site[stored][sel])
                assert not np.isnan(got[sel]).any()
    assert windows_inside_a_tile > 0


def test_the_exact_select_agrees_with_numpy_on_every_scenario():
    """model_quantile puts Q together the way wave_set does, with exact digits: on these inputs that IS numpy."""
    for sc in SCENARIOS:
        call = qc.case(sc.name, "list").calls[0]
        want = qc.statement(call)
        for s, what in enumerate(call.query):
            for w in (0, 1):
                values = call.values(s, w)
                if values.size:
                    got = qc.model_quantile(values, call.sets[s]["quantile"])
                    assert got[0] == want.q[s, w] and got[1] == want.n_cdd_q[s, w], (sc.name, s, w, got)
                    assert want.u_count[s, w] == (values > call.sets[s]["x"]).sum()


WRONG = {
    "digits_cut_after_level_2": ("plain3_light", "plain6_heavy", "plain13_heavy", "rich9_light", "inverted_third_heavy", "last_tiny"),
    "prefix_never_rejects": ("plain1_light", "rich4_heavy", "rich12_light", "plain13_heavy", "bin_257", "inverted_third_light"),
    "next_always_m_gt": ("plain6_heavy", "rich13_light", "last_half", "last_one", "bin_256", "gap_to_107", "inverted_zero"),
    "lerp_first_arm": ("arms", "gap_to_256"),
}


@pytest.mark.parametrize("variant", qc.VARIANTS)
def test_a_wrong_select_would_be_seen(variant):
    """Each of these scenarios has a record whose expected Q or n_cdd_q the broken variant does not reproduce."""
    for name in WRONG[variant]:
        call = qc.case(name, "list").calls[0]
        want = qc.statement(call)
        seen = 0
        for s, what in enumerate(call.query):
            if isinstance(what, str):
                continue
            got = qc.model_quantile(call.values(s, 0), call.sets[s]["quantile"], variant)
            seen += not (got[0] == want.q[s, 0] and got[1] == want.n_cdd_q[s, 0])
        assert seen > 0, (variant, name)


def test_one_ulp_answers_are_one_of_the_two_neighbours():
    for name in ("plain6_heavy", "plain13_light", "rich6_heavy", "rich13_light", "inverted_third_heavy"):
        sc = qc.scenario(name)
        (a, b), values = sc.ulp_pairs[0], sc.sorted_eff()
        got = {}
        for q in sc.queries:
            r = qc.route_of_values(values, q.quantile)
            if not r.take_max and (values[r.k0], values[r.k0 + 1]) == (a, b):
                got[q.arm] = float(np.quantile(values, q.quantile))
        assert {"below_half", "half", "above_half"} <= set(got) and set(got.values()) <= {a, b}
        assert got["below_half"] == a and got["above_half"] == b
        even = a if int(np.float64(a).view(np.uint64)) % 2 == 0 else b  # a + ulp / 2 is a tie: to the even mantissa
        assert got["half"] == even, name
