"""Hand-placed doubles for the Q quantile of the windows stage (wave_set, bin_of_rank, wave_select_kth and
digit_on_path in sai_amd/csrc/windows.hip).  Plain numpy; sai_window_stats takes the target frequencies and the flag
planes as arrays, so no genotypes are involved: a case IS its tgt_freq array, its plane rows, its parameter sets and
its lo / hi ranges.  test_quantile_select_cases_cpu.py proves what every case claims, test_quantile_select_device.py
runs the kernels on them.

A set's Q goes one of three ROUTES: (1) direct ranking of at most kWaveCap values; (2) the first-digit bin that holds
the wanted rank has at most kWaveCap members and is gathered; (3) the level-by-level select on base-256 digits of the
value itself.  The DEPTH of an answer is the level at which the bin that holds the wanted rank has at most kWaveCap
members (0 on route 2, 1 .. kMaxLevels - 2 on route 3), or the last level kMaxLevels - 1, which only more than
kWaveCap copies of ONE number reach.  The values are read in one of four WAYS (value sources):
  ``wave``         fewer than kWinWaves sets: one wave per window, planes and frequencies from global memory;
  ``list``         workgroup form, rows and stored frequencies in LDS, the wave's slot list (inverted: bit 15);
  ``freq_global``  workgroup form, rows in LDS, more than kFreqCap stored frequencies: those from global memory;
  ``rows_global``  workgroup form, the window's rows exceed kRowWords: everything from global memory.

A SCENARIO is a multiset of effective values (groups of equal doubles, some stored as v with the inverted bit up so
that the kernel forms 1.0 - v) and a list of queries (quantile, x) with the rank position and the interpolation arm
each is meant to hit.  Every scenario is laid out in each of the four ways; the windows of a layout hold the same
multiset in different site orders and at different offsets inside their edge tiles.

Which level a value can reach: a double >= 2^-55 has its last mantissa bit at 2^-107 or above, and bit 107 lies in
digit 13, so levels 0 .. 13 (112 fractional bits) already tell any two distinct admissible values apart -- 2^-55 and its
upper neighbour part at level 13.  Level 14, the last of kMaxLevels = 15, is spare: only more than kWaveCap copies of
one number get there (every digit of theirs is 0 by then).  The comment on kMaxLevels in windows.hip ("120 fractional
bits tell any two distinct doubles apart") is true but one level generous.

The statement of what the kernels must return is numpy (``statement``): np.quantile with its default method on the
float64 effective values, and plain comparisons for the counts and lists.  ``route_of`` restates the route decision
with digits taken from fractions.Fraction, no floating point; ``model_quantile`` is the select in exact arithmetic,
with the deliberately broken variants that the CPU test uses to show that these inputs would expose them.
"""

from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from fractions import Fraction
from functools import lru_cache
from pathlib import Path

import numpy as np

from capacity_cases import parse_constants

CSRC = Path(__file__).resolve().parent.parent / "sai_amd" / "csrc"
TILE = 64
PLANES_PER_SET = 3  # SAI_PLANES_PER_SET: words of a tile row reserved per set
WAYS = ("wave", "list", "freq_global", "rows_global")
_NAMES = ("kWaveCap", "kDigitBits", "kMaxLevels", "kListCap", "kFreqCap", "kRowWords", "kLdsTiles", "kWinWaves")
MIN_FREQ = 2.0**-55  # the smallest nonzero frequency the kernel's comment on kMaxLevels admits


@lru_cache(maxsize=None)
def constants() -> dict:
    found = parse_constants((CSRC / "windows.hip").read_text())
    missing = [n for n in _NAMES if n not in found]
    if missing:
        raise KeyError(f"windows.hip no longer defines constexpr int {missing}")
    return {n: found[n] for n in _NAMES}


def base() -> int:
    return 1 << constants()["kDigitBits"]


def last_level() -> int:
    return constants()["kMaxLevels"] - 1


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- exact digits -------------------------------------------------------------------------------------


@lru_cache(maxsize=None)
def digits(v: float, cut: int = -1) -> tuple:
    """The kMaxLevels base-256 digits of a double in [0, 1], exactly: digit l = floor(v 256^(l+1)) - 256 floor(v 256^l);
    1.0 has first digit 256 and zeros behind.  ``cut`` >= 0: the code is cut off after level ``cut`` (zeros behind),
    the first of the broken variants."""
    f, b = Fraction(float(v)), base()
    assert 0 <= f <= 1, v
    out, prefix = [], 0
    for level in range(constants()["kMaxLevels"]):
        p = (f * b ** (level + 1)).__floor__()
        out.append(p - prefix * b if cut < 0 or level <= cut else 0)
        prefix = p
    return tuple(out)


def shared_digits(a: float, b: float) -> int:
    """Leading digits that two doubles have in common (kMaxLevels when all are equal)."""
    da, db = digits(a), digits(b)
    n = 0
    while n < len(da) and da[n] == db[n]:
        n += 1
    return n


def exact_float(f: Fraction) -> float:
    v = float(f)
    if Fraction(v) != f:
        raise ValueError(f"{f} is not a double")
    return v


def from_digits(ds) -> float:
    """The double that the digits spell (a ValueError when it is none)."""
    b = base()
    return exact_float(sum(Fraction(d, b ** (i + 1)) for i, d in enumerate(ds)))


# ---- scenarios ------------------------------------------------------------------------------------------


@dataclass
class Group:
    v: float  # as stored
    inverted: bool  # the kernel forms 1.0 - v
    count: int
    role: str = ""  # "a", "b", "below<j>", "above<j>", ...

    @property
    def eff(self) -> float:
        return float(np.float64(1.0) - np.float64(self.v)) if self.inverted else self.v


@dataclass
class Query:
    quantile: float
    x: float
    position: str  # where in the gathered bin the wanted rank lies: "first", "last" (a bin of one: either), "interior"
    arm: str  # "min" (quantile 0.0), "max" (take_max), "exact" (g = 0), "below_half", "half", "above_half"
    route: int  # claimed: 1, 2, 3
    depth: int | None  # claimed: None on route 1


@dataclass
class Scenario:
    name: str
    groups: list
    queries: list
    pairs: list = field(default_factory=list)  # (a, b, L): effective doubles meant to share exactly L leading digits
    ulp_pairs: list = field(default_factory=list)  # (a, b): meant to be neighbouring doubles

    @property
    def inverted(self) -> bool:
        return any(g.inverted for g in self.groups)

    @property
    def n(self) -> int:
        return sum(g.count for g in self.groups)

    def sorted_eff(self) -> np.ndarray:
        return np.sort(np.concatenate([np.full(g.count, g.eff) for g in self.groups]))


class NoSuchQuantile(ValueError):
    pass


def quantile_for(n: int, k0: int, g: Fraction, exact: bool) -> float:
    """A double q whose virtual index (n - 1) * q, a float64 product as in numpy's 'linear' method, is k0 + g: EXACTLY
    (``exact``; not every n and k0 have such a double) or to within the product's rounding."""
    want = exact_float(Fraction(k0) + g)
    q = np.float64(float((Fraction(k0) + g) / (n - 1)))
    if not exact:
        got = Fraction(float(np.float64(n - 1) * q)) - k0
        if abs(got - g) < Fraction(1, 1 << 30):
            return float(q)
        raise NoSuchQuantile(f"({n} - 1) q is not near {want}")
    for steps in (0, 1, -1, 2, -2, 3, -3):
        cand = q
        for _ in range(abs(steps)):
            cand = np.nextafter(cand, np.float64(2.0 if steps > 0 else -1.0))
        if 0.0 <= cand <= 1.0 and np.float64(n - 1) * cand == want:
            return float(cand)
    raise NoSuchQuantile(f"no double q with ({n} - 1) q == {want}")


G_BELOW_HALF = Fraction(1, 2) - Fraction(1, 1 << 20)
ARMS = {"exact": Fraction(0), "below_half": G_BELOW_HALF, "half": Fraction(1, 2), "above_half": Fraction(3, 4),
        "quarter": Fraction(1, 4)}  # fmt: skip


def _query(n, k0, arm, x, position, route, depth) -> Query:
    if arm == "min":
        return Query(0.0, x, position, arm, route, depth)
    if arm == "max":
        return Query(1.0, x, position, arm, route, depth)
    q = quantile_for(n, k0, ARMS[arm], exact=arm in ("exact", "half"))
    return Query(q, x, position, "below_half" if arm == "quarter" else arm, route, depth)


def _start(groups, i: int) -> int:
    """Rank of the first copy of group i (the groups ascend)."""
    return sum(g.count for g in groups[:i])


def _index(groups, role: str) -> int:
    return [g.role for g in groups].index(role)


MAX_PAD = 24


def _fit(name: str, groups: list, make_specs, **kw) -> Scenario:
    """The scenario of ``groups`` and the queries ``make_specs(groups)`` asks for: (k0 or "min" / "max", arm, x,
    position, route, depth) each.  Not every (n, k0) has a double quantile whose virtual index is exactly k0 or
    k0 + 1/2, so a few more copies go to the smallest and to the largest value -- neither is ever what a case is
    about -- until all of them have one."""
    keep_n = kw.pop("keep_n", False)  # the number of values is what the case is about: the copies come from "a" and "b"
    for pad in range(MAX_PAD * MAX_PAD):
        padded = [Group(g.v, g.inverted, g.count, g.role) for g in groups]
        padded[0].count += pad % MAX_PAD
        padded[-1].count += pad // MAX_PAD
        if keep_n:
            ia = _index(padded, "a")
            padded[ia].count -= pad % MAX_PAD
            padded[ia + 1].count -= pad // MAX_PAD
        n = sum(g.count for g in padded)
        try:
            queries = [_query(n, k0 if isinstance(k0, int) else 0, *rest) for k0, *rest in make_specs(padded)]
        except NoSuchQuantile:
            continue
        return Scenario(name, padded, queries, **kw)
    raise NoSuchQuantile(name)

def _decoy(base_value: float, level: int, side: str):
    """A double that shares digits 0 .. level-1 with ``base_value`` and has a smaller (``below``) or larger digit at
    ``level``; zeros behind.  None where no admissible one exists."""
    d = digits(base_value)
    if side == "above":
        if d[level] + 2 > base() - 1:
            return None
        return from_digits(d[:level] + (d[level] + 2,))
    for lower in range(d[level] - 1, -1, -1):
        v = from_digits(d[:level] + (lower,))
        if v == 0.0 or v >= MIN_FREQ:
            return v
    return None


PLAIN_HALF, PLAIN_TINY = 0.5, MIN_FREQ


def rich_half() -> float:
    """In [0.5, 1): digit 0x80 at every level 0..6, so that a decoy can leave the path below it at every level."""
    return from_digits((0x80,) * 7)


def rich_tiny() -> float:
    """2^-55 with digit 0x80 at every level 7..13."""
    return from_digits(digits(MIN_FREQ)[:7] + (0x80,) * 7)


def pair_values(kind: str, L: int):
    """(a, b): the pair of depth L -- 0.5 and 0.5 + 2^-min(8(L+1), 53) for L = 0..6, 2^-55 and
    2^-55 + 2^-min(8(L+1), 107) for L = 7..13 (``plain``); the same steps on the bases with a nonzero digit at
    every level (``rich``)."""
    bits = constants()["kDigitBits"] * (L + 1)
    if L <= 6:
        a = PLAIN_HALF if kind == "plain" else rich_half()
        return a, exact_float(Fraction(a) + Fraction(1, 1 << min(bits, 53)))
    a = PLAIN_TINY if kind == "plain" else rich_tiny()
    return a, exact_float(Fraction(a) + Fraction(1, 1 << min(bits, 107)))


DECOY_COPIES_BELOW, DECOY_COPIES_ABOVE = 3, 2


def pair_scenario(kind: str, L: int, weight: str) -> Scenario:
    """Two doubles that share exactly L leading digits, ``heavy``: each more than kWaveCap times (the select tells
    them apart at level L and runs on to the last level, where the members of a bin are one number); ``light``: each
    fewer, both together more (the bin is gathered at level L).  Decoys leave the path at every earlier level."""
    cap = constants()["kWaveCap"]
    a, b = pair_values(kind, L)
    ca, cb = (cap + 1, cap + 44) if weight == "heavy" else (cap // 2 + 32, cap // 2 + 33)
    below, above = [], []
    for j in range(L):
        lo_v, hi_v = _decoy(a, j, "below"), _decoy(a, j, "above")
        if lo_v is not None:
            below.append((j, lo_v))
        if hi_v is not None:
            above.append((j, hi_v))
    groups = [Group(v, False, DECOY_COPIES_BELOW, f"below{j}") for j, v in below]
    groups += [Group(a, False, ca, "a"), Group(b, False, cb, "b")]
    groups += [Group(v, False, DECOY_COPIES_ABOVE, f"above{j}") for j, v in reversed(above)]  # level 0 is the farthest

    # claims, from the design: a decoy that left the path at level j sits in a bin of its own copies from level j on
    def decoy_claim(level):
        return (2, 0) if level == 0 else (3, level)

    if L == 0:
        on_path = (3, last_level()) if weight == "heavy" else (2, 0)
    else:
        on_path = (3, last_level() if weight == "heavy" else L)
    lowest = decoy_claim(min(j for j, _ in below)) if below else on_path
    highest = decoy_claim(min(j for j, _ in above)) if above else on_path

    def specs(gs):
        ia = _index(gs, "a")
        n_b, ca, cb = _start(gs, ia), gs[ia].count, gs[ia + 1].count
        first_a, last_a, mid_a, first_b, last_b = n_b, n_b + ca - 1, n_b + ca // 2, n_b + ca, n_b + ca + cb - 1
        out = [("min", "min", a, "first", *lowest), ("max", "max", b, "last", *highest), (first_a, "exact", a, "first", *on_path),
               (last_a, "below_half", a, "last", *on_path), (last_a, "half", b, "last", *on_path),
               (last_a, "above_half", a, "last", *on_path), (mid_a, "above_half", a, "interior", *on_path),
               (first_b, "quarter", b, "first", *on_path)]  # fmt: skip
        if above:  # the next order statistic behind the pair is the decoy that left the path last
            out += [(last_b, "quarter", b, "last", *on_path), (last_b, "above_half", gs[ia + 2].v, "last", *on_path),
                    (last_b, "exact", b, "last", *on_path)]  # fmt: skip
        if below:  # the largest value below the pair: the decoy that left the path last; the next order statistic is a
            out.append((n_b - 1, "half", a, "last", *decoy_claim(max(j for j, _ in below))))
        return out

    ulp = [(a, b)] if L in (6, 13) else []
    return _fit(f"{kind}{L}_{weight}", groups, specs, pairs=[(a, b, L)], ulp_pairs=ulp)


def _spread(rng, lo_digit: int, hi_digit: int, count: int):
    """``count`` values k / 2800 with first digits in [lo_digit, hi_digit], as (value, 1) groups."""
    k = np.arange(2801)
    v = k / np.float64(2800)
    d = np.array([digits(float(x))[0] for x in v])
    pool = v[(d >= lo_digit) & (d <= hi_digit)]
    return [float(x) for x in rng.choice(pool, size=count, replace=True)]


def _grouped(values, role):
    out: dict = {}
    for v in values:
        out[v] = out.get(v, 0) + 1
    return [Group(v, False, c, role) for v, c in sorted(out.items())]


def last_level_scenario(which: str) -> Scenario:
    """More than kWaveCap copies of one number: the only way to the last level."""
    cap, last = constants()["kWaveCap"], last_level()
    rng = _rng("last " + which)
    copies = cap + 30
    if which == "half":
        low, high = _grouped(_spread(rng, 3, 120, 110), "low"), _grouped(_spread(rng, 140, 250, 90), "high")
        groups = low + [Group(0.5, False, copies, "a")] + high
        nxt = high[0].v

        def specs(gs):
            s = _start(gs, _index(gs, "a"))
            return [(s, "exact", 0.5, "first", 3, last), (s + copies // 2, "above_half", 0.5, "interior", 3, last),
                    (s + copies - 1, "half", 0.5, "last", 3, last), (s + copies - 1, "quarter", nxt, "last", 3, last),
                    (s + copies - 1, "above_half", 0.5, "last", 3, last)]  # fmt: skip

    elif which == "one":
        low = _grouped(_spread(rng, 3, 250, 240), "low")
        groups = low + [Group(1.0, False, copies, "a")]
        top = low[-1].v

        def specs(gs):
            s, c = _start(gs, len(gs) - 1), gs[-1].count
            return [("max", "max", 1.0, "last", 3, last), (s, "exact", 1.0, "first", 3, last), (s + 7, "above_half", 1.0, "interior", 3, last),
                    (s + c - 2, "half", 1.0, "interior", 3, last), (s - 1, "above_half", top, "last", 2, 0),
                    (s - 1, "quarter", 1.0, "last", 2, 0)]  # fmt: skip

    else:  # tiny: 2^-55, with 0.0 below it (they part at level 6) and 2^-54 above
        high = _grouped(_spread(rng, 1, 250, 200), "high")
        groups = [Group(0.0, False, 5, "zero"), Group(MIN_FREQ, False, copies, "a"), Group(2.0**-54, False, 4, "next")] + high

        def specs(gs):
            z = gs[0].count
            return [("min", "min", MIN_FREQ, "first", 3, 6), (z - 1, "half", 0.0, "last", 3, 6), (z, "exact", MIN_FREQ, "first", 3, last),
                    (z + copies // 2, "above_half", MIN_FREQ, "interior", 3, last), (z + copies - 1, "half", MIN_FREQ, "last", 3, last),
                    (z + copies - 1, "quarter", 2.0**-54, "last", 3, last), (z + copies, "exact", 2.0**-54, "first", 3, 6),
                    (z + copies + 3, "above_half", 2.0**-54, "last", 3, 6)]  # fmt: skip

    return _fit(f"last_{which}", groups, specs)


def bin_members_scenario(members: int) -> Scenario:
    """The first-level bin of digit 100 holds ``members`` values, eight distinct ones that part at level 1: at kWaveCap
    the bin is gathered (route 2), at kWaveCap + 1 the select starts and gathers at level 1."""
    rng = _rng(f"bin members {members}")
    inside = [from_digits((100, 32 * j)) for j in range(8)]
    per = [members // 8 + (1 if j < members % 8 else 0) for j in range(8)]
    low, high = _grouped(_spread(rng, 2, 90, 150), "low"), _grouped(_spread(rng, 104, 250, 190), "high")
    groups = low + [Group(v, False, c, f"in{j}") for j, (v, c) in enumerate(zip(inside, per))] + high
    route, depth = (2, 0) if members <= constants()["kWaveCap"] else (3, 1)
    # route 2 gathers the whole first-level bin, route 3 the level-1 bin of one of the eight values
    pos = (lambda whole, part: whole) if route == 2 else (lambda whole, part: part)
    nxt = high[0].v

    def specs(gs):
        s = _start(gs, _index(gs, "in0"))
        return [(s, "exact", inside[0], "first", route, depth), (s + per[0] - 1, "half", inside[1], pos("interior", "last"), route, depth),
                (s + per[0] + 3, "above_half", inside[1], "interior", route, depth),
                (s + members - 1, "quarter", inside[7], "last", route, depth), (s + members - 1, "half", nxt, "last", route, depth),
                (s + members - 1, "above_half", inside[7], "last", route, depth), (s + members - 1, "exact", nxt, "last", route, depth),
                ("min", "min", gs[0].v, "first", 2, 0), ("max", "max", gs[-1].v, "last", 2, 0)]  # fmt: skip

    return _fit(f"bin_{members}", groups, specs)


def gap_scenario(next_digit: int) -> Scenario:
    """The wanted rank is the last member of the bin of digit 100; the next occupied bin is ``next_digit`` (256: every
    larger value is exactly 1.0)."""
    rng = _rng(f"gap {next_digit}")
    low = _grouped(_spread(rng, 2, 99, 230), "low")
    mine = _grouped(_spread(rng, 100, 100, 40), "mine")
    if next_digit == base():
        high = [Group(1.0, False, 90, "one")]
    else:
        high = [Group(from_digits((next_digit, 0, 7)), False, 2, "next")] + _grouped(_spread(rng, next_digit + 1, 250, 120), "high")
    groups = low + mine + high
    n_mine, top, nxt = sum(g.count for g in mine), mine[-1].v, high[0].v

    def specs(gs):
        first = _start(gs, _index(gs, "mine"))
        k_last = first + n_mine - 1  # the bin's last rank: a copy of the bin's largest value
        return [(k_last, "quarter", top, "last", 2, 0), (k_last, "half", nxt, "last", 2, 0), (k_last, "above_half", top, "last", 2, 0),
                (k_last, "exact", nxt, "last", 2, 0), (k_last, "below_half", top, "last", 2, 0), (first, "above_half", mine[0].v, "first", 2, 0),
                (k_last + 1, "half", nxt, "first", 2, 0), ("max", "max", gs[-1].v, "last", 2, 0)]  # fmt: skip

    return _fit(f"gap_to_{next_digit}", groups, specs)


def ownership_scenario(first: int) -> Scenario:
    """Occupied first digits ``first`` .. ``first + 3`` (clipped at 256) with ranks wanted in each: lane l of bin_of_rank owns
    bins 5 l .. 5 l + 4, so 4 | 5 and 254 | 255 | 256 are read by different lanes."""
    rng = _rng(f"ownership {first}")
    ds = [d for d in range(first, first + 4) if d <= base()]
    groups = []
    for d in ds:
        groups += [Group(1.0, False, 70, f"d{d}")] if d == base() else _grouped(_spread(rng, d, d, 70), f"d{d}")

    def specs(gs):
        by_rank = np.concatenate([np.full(g.count, g.v) for g in gs])
        n, out = by_rank.size, []
        for d in ds:
            mine = [i for i, g in enumerate(gs) if g.role == f"d{d}"]
            s, e = _start(gs, mine[0]), _start(gs, mine[-1] + 1)
            out.append((s, "above_half", float(by_rank[s]), "first", 2, 0))
            if e < n:
                out += [(e - 1, "half", float(by_rank[e]), "last", 2, 0), (e - 1, "quarter", float(by_rank[e - 1]), "last", 2, 0)]
            out.append(((s + e) // 2, "above_half", float(by_rank[(s + e) // 2]), "interior", 2, 0))
        return out + [("min", "min", float(by_rank[0]), "first", 2, 0), ("max", "max", float(by_rank[-1]), "last", 2, 0)]

    return _fit(f"own_{first}", groups, specs)


def arms_scenario() -> Scenario:
    """Eight values three binades apart from 2^-22 up, some 40 copies each, the wanted rank on the last copy of one:
    x1 - x0 and its products with g and 1 - g are inexact, which is what tells the two arms of numpy's lerp apart.
    The values are drawn until the arms differ (x0 + d g != x1 - d (1 - g)) for at least four of the queries.  The
    five values below 2^-8 share the first-digit bin 0."""
    for attempt in range(200):
        rng = _rng(f"arms {attempt}")
        values = [float(np.ldexp(1.0 + rng.random(), -1 - 3 * (7 - i))) for i in range(8)]
        groups = [Group(float(v), False, 38 + i, f"v{i}") for i, v in enumerate(values)]

        def specs(gs):
            out = []
            for i in range(len(gs) - 1):
                k_last = _start(gs, i + 1) - 1
                ends_bin = digits(gs[i].v)[0] != digits(gs[i + 1].v)[0]
                out += [(k_last, "above_half", gs[i].v, "last" if ends_bin else "interior", 2, 0),
                        (k_last, "half", gs[i + 1].v, "last" if ends_bin else "interior", 2, 0)]  # fmt: skip
            return out + [(_start(gs, 6), "quarter", gs[6].v, "first", 2, 0)]

        sc = _fit("arms", groups, specs)
        s, differ = sc.sorted_eff(), 0
        for q in sc.queries:
            v = np.float64(sc.n - 1) * np.float64(q.quantile)
            k0 = int(np.floor(v))
            differ += _lerp(s[k0], s[k0 + 1], v, np.floor(v)) != _lerp(s[k0], s[k0 + 1], v, np.floor(v), first_arm_only=True)
        if differ >= 4:
            return sc
    raise AssertionError("no values found")


def direct_scenario(n_cond: int) -> Scenario:
    """Route 1: at most kWaveCap values (``n_cond`` exactly), among them 2/3 and its upper neighbour."""
    rng = _rng(f"direct {n_cond}")
    a = 2.0 / 3.0
    b = float(np.nextafter(np.float64(a), np.float64(1.0)))
    share = n_cond // 5
    low, high = _grouped(_spread(rng, 2, 160, n_cond - 3 * share), "low"), _grouped(_spread(rng, 180, 256, share), "high")
    groups = low + [Group(a, False, share, "a"), Group(b, False, share, "b")] + high

    def specs(gs):
        ia = _index(gs, "a")
        first_a = _start(gs, ia)
        last_a, last_b = first_a + gs[ia].count - 1, first_a + gs[ia].count + gs[ia + 1].count - 1
        return [("min", "min", a, "first", 1, None), ("max", "max", b, "last", 1, None), (first_a, "exact", a, "interior", 1, None),
                (last_a, "below_half", a, "interior", 1, None), (last_a, "half", b, "interior", 1, None),
                (last_a, "above_half", a, "interior", 1, None), (last_b, "above_half", b, "interior", 1, None),
                (last_b, "quarter", gs[ia + 2].v, "interior", 1, None)]  # fmt: skip

    sc = _fit(f"direct_{n_cond}", groups, specs, ulp_pairs=[(a, b)], keep_n=True)
    assert sc.n == n_cond
    return sc


def inverted_third_scenario(weight: str) -> Scenario:
    """1/3 with the inverted bit up next to a plain 2/3: 1 - 1/3 is the double after 2/3, they part at level 6."""
    cap, last = constants()["kWaveCap"], last_level()
    a, third = 2.0 / 3.0, 1.0 / 3.0
    b = float(np.float64(1.0) - np.float64(third))
    ca, cb = (cap + 9, cap + 1) if weight == "heavy" else (cap // 2 + 40, cap // 2 + 41)
    groups = [Group(0.75, True, 3, "below0"), Group(from_digits(digits(a)[:3] + (2,)), False, 3, "below3"), Group(a, False, ca, "a"),
              Group(third, True, cb, "b"), Group(exact_float(1 - Fraction(from_digits(digits(a)[:2] + (200,)))), True, 2, "above2"),
              Group(0.125, True, 2, "above0")]  # fmt: skip
    depth = last if weight == "heavy" else 6

    def specs(gs):
        n_b = _start(gs, _index(gs, "a"))
        return [("min", "min", a, "first", 2, 0), ("max", "max", b, "last", 2, 0), (n_b, "exact", a, "first", 3, depth),
                (n_b + ca - 1, "below_half", a, "last", 3, depth), (n_b + ca - 1, "half", b, "last", 3, depth),
                (n_b + ca - 1, "above_half", a, "last", 3, depth), (n_b + ca // 2, "above_half", a, "interior", 3, depth),
                (n_b + ca, "quarter", b, "first", 3, depth), (n_b + ca + cb - 1, "quarter", b, "last", 3, depth),
                (n_b + ca + cb - 1, "above_half", gs[4].eff, "last", 3, depth), (n_b - 1, "half", a, "last", 3, 3)]  # fmt: skip

    return _fit(f"inverted_third_{weight}", groups, specs, pairs=[(a, b, 6)], ulp_pairs=[(a, b)])


def inverted_zero_scenario() -> Scenario:
    """0.0 with the inverted bit up lands in bin 256 next to a plain 1.0."""
    cap, last = constants()["kWaveCap"], last_level()
    rng = _rng("inverted zero")
    low = _grouped(_spread(rng, 3, 250, 240), "low")
    c0 = cap // 2 + 20
    groups = low + [Group(0.0, True, c0, "flipped zero"), Group(1.0, False, cap // 2 + 25, "one")]
    top = low[-1].v

    def specs(gs):
        s = _start(gs, _index(gs, "flipped zero"))
        return [("max", "max", top, "last", 3, last), (s, "exact", 1.0, "first", 3, last), (s + c0, "above_half", 1.0, "interior", 3, last),
                (s - 1, "above_half", top, "last", 2, 0), (s - 1, "quarter", 1.0, "last", 2, 0)]  # fmt: skip

    return _fit("inverted_zero", groups, specs)


DEPTHS = tuple(range(14))


@lru_cache(maxsize=None)
def scenarios() -> tuple:
    cap = constants()["kWaveCap"]
    out = [pair_scenario(kind, L, weight) for kind in ("plain", "rich") for L in DEPTHS for weight in ("heavy", "light")]
    out += [last_level_scenario(w) for w in ("half", "one", "tiny")]
    out += [bin_members_scenario(cap), bin_members_scenario(cap + 1), gap_scenario(107), gap_scenario(base())]
    out += [ownership_scenario(3), ownership_scenario(253), arms_scenario()]
    out += [direct_scenario(cap), direct_scenario(40)]
    out += [inverted_third_scenario("heavy"), inverted_third_scenario("light"), inverted_zero_scenario()]
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def scenario(name: str) -> Scenario:
    return {s.name: s for s in scenarios()}[name]


# ---- layouts: a scenario in one of the four ways ---------------------------------------------------------

REGION = 30 * TILE  # sites a window's region takes of the block
WINDOWS = ((1, 1700), (63, 1700), (0, 26 * TILE))  # (offset of lo inside the region, length): lo and hi inside a tile twice
TRIVIAL = ("light", "empty", "flipped")  # the other sets of a call


@dataclass
class Call:
    """One sai_window_stats call and what it was built from."""

    n_sites: int
    tgt_freq: np.ndarray  # float64 [n_sites]: a tile's stored frequencies packed in its first slots, NaN elsewhere
    planes: np.ndarray  # int64 [n_tiles][PLANES_PER_SET * n_sets]
    sets: list  # dict(x, quantile, anc)
    query: list  # per set: index into the scenario's queries, or a name of TRIVIAL
    lo: np.ndarray  # int32 [n_windows]
    hi: np.ndarray
    pos: np.ndarray  # int32 [n_sites]
    cond: np.ndarray  # bool [n_sets][n_sites]
    inv: np.ndarray  # bool [n_sets][n_sites]
    any: np.ndarray  # bool [n_sites]
    v_site: np.ndarray  # float64 [n_sites]: the stored value of a site some set selects, NaN elsewhere

    @property
    def n_sets(self) -> int:
        return len(self.sets)

    @property
    def with_inv(self) -> bool:
        return any(not s["anc"] for s in self.sets)

    @property
    def used(self) -> int:
        return 1 + self.n_sets * (2 if self.with_inv else 1)

    def values(self, s: int, w: int) -> np.ndarray:
        """The float64 effective values of set s in window w, in site order."""
        lo, hi = int(self.lo[w]), int(self.hi[w])
        m = self.cond[s, lo:hi]
        v = self.v_site[lo:hi][m]
        return np.where(self.inv[s, lo:hi][m], np.float64(1.0) - v, v)


@dataclass
class Case:
    name: str
    scenario: Scenario
    way: str
    calls: list


def _pack(any_bits, v_site, cond, inv, with_inv):
    n_sets, n_sites = cond.shape
    n_tiles = n_sites // TILE
    tgt = np.full(n_sites, np.nan)
    planes = np.zeros((n_tiles, PLANES_PER_SET * n_sets), dtype=np.uint64)
    weights = np.uint64(1) << np.arange(TILE, dtype=np.uint64)
    word = lambda bits: (bits.reshape(n_tiles, TILE).astype(np.uint64) * weights).sum(axis=1, dtype=np.uint64)  # noqa: E731
    planes[:, 0] = word(any_bits)
    for s in range(n_sets):
        planes[:, 1 + s] = word(cond[s])
        if with_inv:
            planes[:, 1 + n_sets + s] = word(inv[s])
    for t in range(n_tiles):
        stored = np.flatnonzero(any_bits[t * TILE : (t + 1) * TILE])
        tgt[t * TILE : t * TILE + stored.size] = v_site[t * TILE + stored]
    return tgt, planes.view(np.int64)


def _trivial_sets(rng, free, lo, hi):
    """sites, stored values and inverted flags of the trivial sets in one window: ``light`` five values, ``empty`` none,
    ``flipped`` six values of 0.25 of which three are inverted."""
    sites = rng.choice(free, size=11, replace=False)
    light, flipped = np.sort(sites[:5]), np.sort(sites[5:])
    return dict(light=(light, np.array([0.25, 0.75, 0.5, 0.125, 1.0]), np.zeros(5, bool)), empty=(light[:0], np.zeros(0), np.zeros(0, bool)),
                flipped=(flipped, np.full(6, 0.25), np.arange(6) % 2 == 0))  # fmt: skip


def _layout(sc: Scenario, way: str, set_plan: list, dense_any: bool, tag: str) -> Call:
    """set_plan: per set (query index or trivial name, anc)."""
    rng = _rng(f"{sc.name}/{way}/{tag}")
    n_sites = REGION * len(WINDOWS)
    n_sets = len(set_plan)
    cond, inv = np.zeros((n_sets, n_sites), bool), np.zeros((n_sets, n_sites), bool)
    v_site = np.full(n_sites, np.nan)
    any_bits = np.zeros(n_sites, bool)
    eff_v = np.concatenate([np.full(g.count, g.v) for g in sc.groups])
    eff_i = np.concatenate([np.full(g.count, g.inverted) for g in sc.groups])
    main = [s for s, (what, _) in enumerate(set_plan) if not isinstance(what, str)]
    los, his = [], []
    for w, (off, length) in enumerate(WINDOWS):
        lo = w * REGION + off
        hi = lo + length
        sites = np.sort(rng.choice(np.arange(lo, hi), size=sc.n, replace=False))
        order = rng.permutation(sc.n)
        v_site[sites], main_inv = eff_v[order], eff_i[order]
        outside = [p for p in (lo - 1, hi) if w * REGION <= p < (w + 1) * REGION]  # condition sites next to the window
        v_site[outside] = 0.999
        for s in main:
            cond[s, sites] = True
            inv[s, sites] = main_inv
            cond[s, outside] = True
        free = np.setdiff1d(np.arange(lo, hi), sites)
        triv = _trivial_sets(rng, free, lo, hi)
        for s, (what, _) in enumerate(set_plan):
            if isinstance(what, str):
                t_sites, t_v, t_inv = triv[what]
                cond[s, t_sites], inv[s, t_sites], v_site[t_sites] = True, t_inv, t_v
        # "any" is a strict superset of the conditions: further sites of the window's tiles whose slots hold NaN
        extra = rng.choice(np.setdiff1d(free, np.concatenate([t[0] for t in triv.values()])), size=40, replace=False)
        any_bits[extra] = True
        los.append(lo)
        his.append(hi)
    inv &= cond
    selected = cond.any(axis=0)
    v_site[~selected] = np.nan
    any_bits |= selected
    if dense_any:
        any_bits[:] = True
    sets = []
    for what, anc in set_plan:
        if isinstance(what, str):
            sets.append(dict(x=0.3, quantile=0.5, anc=anc))
        else:
            sets.append(dict(x=sc.queries[what].x, quantile=sc.queries[what].quantile, anc=anc))
    with_inv = any(not a for _, a in set_plan)
    assert with_inv or not inv.any()
    tgt, planes = _pack(any_bits, v_site, cond, inv, with_inv)
    pos = (7 + 3 * np.arange(n_sites)).astype(np.int32)
    return Call(n_sites, tgt, planes, sets, [what for what, _ in set_plan], np.array(los, np.int32), np.array(his, np.int32), pos,
                cond, inv, any_bits, v_site)  # fmt: skip


MAX_SETS = 20  # SAI_MAX_SETS


@lru_cache(maxsize=64)
def case(name: str, way: str) -> Case:
    sc = scenario(name)
    waves = constants()["kWinWaves"]
    nq = len(sc.queries)
    flipped_anc = False  # the set that carries inverted sites of its own never has ancestral alleles
    if way == "wave":
        per = waves - 1
        calls = []
        for c0 in range(0, nq, per):
            plan = [(i, not sc.inverted) for i in range(c0, min(c0 + per, nq))]
            plan += [("light", not sc.inverted)] * (per - len(plan))
            calls.append(_layout(sc, way, plan, False, f"call{c0}"))
    elif way == "list":
        plan = [(i, not sc.inverted) for i in range(nq)] + [("light", not sc.inverted), ("empty", not sc.inverted)]
        if sc.inverted:
            plan.append(("flipped", flipped_anc))
        calls = [_layout(sc, way, plan, False, "call")]
    elif way == "freq_global":
        # 1 + 2 n words per row: beyond 17 sets the rows of these windows no longer fit kRowWords
        plan = [(i, not sc.inverted) for i in range(nq)] + [("flipped", flipped_anc), ("light", True), ("empty", True)][: max(17 - nq, 1)]
        calls = [_layout(sc, way, plan, True, "call")]
    elif way == "rows_global":
        plan = [(i, False) for i in range(nq)]
        plan += [(TRIVIAL[j % 3], False) for j in range(MAX_SETS - nq)]
        calls = [_layout(sc, way, plan, False, "call")]
    else:
        raise KeyError(way)
    return Case(f"{name}-{way}", sc, way, calls)


def case_ids() -> list:
    return [(s.name, way) for s in scenarios() for way in WAYS]


# ---- the statement: numpy ---------------------------------------------------------------------------------


@dataclass
class Expected:
    n_sites: np.ndarray  # int64 [n_sets][n_windows]
    n_cond: np.ndarray
    u_count: np.ndarray
    n_cdd_q: np.ndarray
    q: np.ndarray  # float64, NaN for a set without a condition site in the window
    u_lists: list  # [set][window] -> int32 positions in site order
    q_lists: list


def statement(call: Call) -> Expected:
    n_s, n_w = call.n_sets, int(call.lo.size)
    shape = (n_s, n_w)
    out = Expected(np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(shape, np.int64),
                   np.full(shape, np.nan), [[None] * n_w for _ in range(n_s)], [[None] * n_w for _ in range(n_s)])  # fmt: skip
    for s, p in enumerate(call.sets):
        for w in range(n_w):
            lo, hi = int(call.lo[w]), int(call.hi[w])
            values = call.values(s, w)
            site_pos = call.pos[lo:hi][call.cond[s, lo:hi]]
            out.n_sites[s, w], out.n_cond[s, w] = hi - lo, values.size
            in_u = values > p["x"]
            out.u_count[s, w], out.u_lists[s][w] = int(in_u.sum()), site_pos[in_u]
            if values.size:
                q = np.quantile(values, p["quantile"])
                in_q = values >= q
                out.q[s, w], out.n_cdd_q[s, w], out.q_lists[s][w] = q, int(in_q.sum()), site_pos[in_q]
            else:
                out.q_lists[s][w] = site_pos[:0]
    return out


# ---- the route, restated without floating point -----------------------------------------------------------


def virtual_index(n: int, quantile: float):
    """(k0, take_max, g) of numpy's 'linear' method: the virtual index (n - 1) q is a float64 product."""
    v = np.float64(n - 1) * np.float64(quantile)
    if v >= n - 1:
        return n - 1, True, Fraction(0)
    k0 = int(np.floor(v))
    return k0, False, Fraction(float(v)) - k0


def _bin_of_rank(counts: dict, k: int):
    """counts: digit -> members.  (digit, rank inside the bin, members) of the bin that holds rank k."""
    before = 0
    for d in sorted(counts):
        if k < before + counts[d]:
            return d, k - before, counts[d]
        before += counts[d]
    raise AssertionError("rank beyond the values")


@dataclass
class Route:
    route: int
    depth: int | None
    rank_in_bin: int
    members: int
    k0: int
    take_max: bool
    g: Fraction


def route_of_values(values: np.ndarray, quantile: float) -> Route:
    """Route, depth and the place of the wanted rank in the bin that is gathered, from exact digits."""
    cap = constants()["kWaveCap"]
    n = int(values.size)
    k0, take_max, g = virtual_index(n, quantile)
    if n <= cap:
        return Route(1, None, k0, n, k0, take_max, g)
    uniq, cnt = np.unique(values, return_counts=True)
    alive = [(digits(float(v)), int(c)) for v, c in zip(uniq, cnt)]
    k = k0
    for level in range(constants()["kMaxLevels"]):
        counts: dict = {}
        for d, c in alive:
            counts[d[level]] = counts.get(d[level], 0) + c
        digit, k, members = _bin_of_rank(counts, k)
        if members <= cap or level == last_level():
            return Route(2 if level == 0 else 3, level, k, members, k0, take_max, g)
        alive = [(d, c) for d, c in alive if d[level] == digit]
    raise AssertionError("not reached")


def value_source(call: Call, s: int, w: int) -> str:
    c = constants()
    if call.n_sets < c["kWinWaves"]:
        return "wave"
    lo, hi = int(call.lo[w]), int(call.hi[w])
    t0, t1 = lo // TILE, (hi + TILE - 1) // TILE
    nt = t1 - t0
    if nt > c["kLdsTiles"] or nt * call.used > c["kRowWords"]:
        return "rows_global"
    if int(call.any[t0 * TILE : t1 * TILE].sum()) > c["kFreqCap"]:
        return "freq_global"
    return "list" if int(call.cond[s, lo:hi].sum()) <= c["kListCap"] else "lds_walk"


def route_of(call: Call, s: int, w: int):
    """(route, depth, value source) of set s in window w."""
    r = route_of_values(call.values(s, w), call.sets[s]["quantile"])
    return r.route, r.depth, value_source(call, s, w)


# ---- the select in exact arithmetic, and broken variants of it -----------------------------------------------

VARIANTS = ("digits_cut_after_level_2", "prefix_never_rejects", "next_always_m_gt", "lerp_first_arm")


def _lerp(x0, x1, v, fl_v, first_arm_only=False):
    x0, x1 = np.float64(x0), np.float64(x1)
    g = np.float64(v) - np.float64(fl_v)
    d = x1 - x0
    if g >= 0.5 and not first_arm_only:
        return x1 - d * (np.float64(1.0) - g)
    return x0 + d * g


def _digit_on_path(code: tuple, path: tuple, never_reject: bool):
    """Digit len(path) of a value with digits ``code``, -1 when it left ``path`` earlier.  ``never_reject``: the check is
    skipped, and floor(s 256) - 256 prefix of a value off the path ends up in the histogram's first or last bin."""
    level = len(path)
    if code[:level] == path:
        return code[level]
    if not never_reject:
        return -1
    b = base()
    num = lambda ds: sum(d * b ** (len(ds) - 1 - i) for i, d in enumerate(ds))  # noqa: E731
    return int(min(max(num(code[: level + 1]) - num(path) * b, 0), b))


def _select_kth(values: np.ndarray, k: int, variant):
    """wave_select_kth on the values in site order."""
    cap = constants()["kWaveCap"]
    cut = 2 if variant == "digits_cut_after_level_2" else -1
    never = variant == "prefix_never_rejects"
    codes = [digits(float(v), cut) for v in values]
    path: tuple = ()
    for level in range(constants()["kMaxLevels"]):
        ds = [_digit_on_path(c, path, never) for c in codes]
        counts: dict = {}
        for d in ds:
            if d >= 0:
                counts[d] = counts.get(d, 0) + 1
        digit, k, members = _bin_of_rank(counts, k)
        if members <= cap or level == last_level():
            gathered = [float(v) for v, d in zip(values, ds) if d == digit]
            return gathered[0] if members > cap else sorted(gathered)[k]
        path = path + (digit,)
    raise AssertionError("not reached")


def model_quantile(values: np.ndarray, quantile: float, variant=None):
    """(Q, n_cdd_q) as wave_set puts them together, route by route; ``variant`` breaks one step."""
    assert variant is None or variant in VARIANTS
    cap = constants()["kWaveCap"]
    values = np.asarray(values, dtype=np.float64)
    n = int(values.size)
    v = np.float64(n - 1) * np.float64(quantile)
    take_max = bool(v >= n - 1)
    fl_v = np.floor(v)
    k0 = n - 1 if take_max else int(fl_v)
    first_arm = variant == "lerp_first_arm"
    if n <= cap:
        s = np.sort(values)
        q = s[k0] if take_max else _lerp(s[k0], s[k0 + 1], v, fl_v, first_arm)
        return float(q), int((values >= q).sum())
    first = np.array([digits(float(e))[0] for e in values])
    counts = {int(d): int(c) for d, c in zip(*np.unique(first, return_counts=True))}
    digit, r, members = _bin_of_rank(counts, k0)
    if members <= cap:
        mine = np.sort(values[first == digit])
        above = values[first > digit]
        x1 = mine[r + 1] if r + 1 < members else (above.min() if above.size else np.inf)
        if variant == "next_always_m_gt":
            greater = values[values > mine[r]]
            x1 = greater.min() if greater.size else np.inf
        with np.errstate(invalid="ignore"):
            q = mine[r] if take_max else _lerp(mine[r], x1, v, fl_v, first_arm)
        return float(q), n - (k0 - r) - members + int((mine >= q).sum())
    x0 = np.float64(_select_kth(values, k0, variant))
    q = x0
    if not take_max:
        n_le = int((values <= x0).sum())
        greater = values[values > x0]
        m_gt = greater.min() if greater.size else np.inf
        x1 = x0 if n_le > k0 + 1 and variant != "next_always_m_gt" else m_gt
        with np.errstate(invalid="ignore"):
            q = _lerp(x0, x1, v, fl_v, first_arm)
    return float(q), int((values >= q).sum())
