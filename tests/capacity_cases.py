"""Deterministic inputs that sit exactly on, and one past, the internal capacities of the windows stage
(sai_amd/csrc/windows.hip) and of the streaming accumulators (stream_loops.hpp, site_pass.hip,
site_pass_dd.hip, dd.hip).  Plain numpy; the capacities are read out of the sources (``constants``), every
case is derived from them, and every window case states what it claims to reach -- test_capacity_cases_cpu.py
recomputes the claims from the matrices with the oracle, test_capacity_edges_device.py runs the kernels.

Window cases use a controllable design instead of random selection:
  * the reference population is all zeros (frequency 0 < w) -- except at the sites a case wants INVERTED, where it
    is all ones and the set's switch is off, so that without ancestral alleles the mirror condition holds, the site
    is flipped (reference 1 -> 0) and its target frequency enters as 1 - f;
  * one diploid one-individual source per "switch" (two of them): dosage 2 meets ("=", 1.0), dosage 0 does not; a
    set listens to one switch and lets the other pass with (">=", 0.0);
  * the target population carries the allele in its first k haplotypes: frequency k / (2 n) exactly.
"""

from __future__ import annotations

import re
import zlib
from dataclasses import dataclass, field
from functools import lru_cache
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "sai_amd" / "csrc"
TILE = 64
DIGITS = 256  # first radix digit of a value in [0, 1]: floor(v * 256), 256 for exactly 1.0

_WANTED = {
    "windows.hip": ["kWaveCap", "kFreqCap", "kLdsTiles", "kRowWords", "kListCap", "kWinWaves"],
    "stream_loops.hpp": ["kChunkIters", "kUnroll"],
    "site_eval.hpp": ["kTableFromSets"],
}


def parse_constants(text: str) -> dict:
    """Every ``constexpr int kName = <integer expression of earlier names>;`` of a source text."""
    out: dict = {}
    for name, expr in re.findall(r"^\s*constexpr\s+int\s+(k\w+)\s*=\s*([^;]+);", text, flags=re.M):
        expr = re.sub(r"\bk\w+\b", lambda m: str(out[m.group(0)]) if m.group(0) in out else "?", expr)
        if re.fullmatch(r"[\d\s()+\-*/<]+", expr):
            out[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}))  # noqa: S307 - digits and operators only
    return out


@lru_cache(maxsize=None)
def constants() -> dict:
    """The capacities the cases are built from, by name, from the sources that define them."""
    out = {}
    for unit, names in _WANTED.items():
        found = parse_constants((CSRC / unit).read_text())
        for n in names:
            if n not in found:
                raise KeyError(f"{unit} no longer defines constexpr int {n}")
            out[n] = found[n]
    return out


def first_digit(e):
    return np.minimum((np.asarray(e, dtype=np.float64) * DIGITS).astype(np.int64), DIGITS)


def rank_of_quantile(n: int, q: float):
    """(k0, take_max) of numpy's 'linear' quantile over n values: virtual index (n - 1) * q in f64."""
    v = np.float64(n - 1) * np.float64(q)
    if v >= n - 1:
        return n - 1, True
    return int(np.floor(v)), False


def rank_claims(values: np.ndarray, q: float) -> dict:
    """k0, the members of the first-digit bin that holds rank k0, and how many bins further the next order
    statistic lies (0: same bin, 2: an empty bin between; None where there is no next one)."""
    n = int(values.size)
    if n == 0:
        return dict(k0=None, members=None, gap=None)
    d = first_digit(np.sort(values))
    k0, take_max = rank_of_quantile(n, q)
    gap = None if take_max or k0 + 1 >= n else int(d[k0 + 1] - d[k0])
    return dict(k0=k0, members=int((d == d[k0]).sum()), gap=gap)


@dataclass
class WindowCase:
    name: str
    mats: list  # ref, tgt, switch 0, switch 1 (int8 [n_sites][n_ind])
    ploidy: list
    pos: np.ndarray
    specs: list  # dict(w, x, quantile, y_list, anc)
    ranges: list  # (lo, hi) site range of every window
    windows: list  # inclusive (start, end) positions of every window
    claims: list  # per window: nt, row_words, stored, n_cond[set], k0[set], members[set], gap[set]
    pins: list = field(default_factory=list)  # (quantity, window, set or None, the value the case is about)

    @property
    def used(self) -> int:
        return 1 + len(self.specs) * (1 if all(s["anc"] for s in self.specs) else 2)


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _pick(rng, lo: int, hi: int, count: int, exclude=()) -> np.ndarray:
    pool = np.setdiff1d(np.arange(lo, hi), np.asarray(list(exclude), dtype=np.int64))
    if count > pool.size:
        raise ValueError(f"{count} sites wanted, {pool.size} free in [{lo}, {hi})")
    return np.sort(rng.choice(pool, size=count, replace=False))


def _assemble(name, n_tgt, k, on, inv, set_groups, set_anc, quantiles, xs, ranges, pins) -> WindowCase:
    """k[site] = allele count of the target (frequency k / (2 n_tgt)); on[g][site] = switch g up (a direct site);
    inv[site] = g: the site is an inverted one of switch g (-1: none).  Claims come from this design, not from
    the matrices."""
    k = np.asarray(k, dtype=np.int64)
    n_sites = k.size
    inv = np.asarray(inv, dtype=np.int64)
    on = np.asarray(on, dtype=bool) & (inv < 0)
    if k.min() < 0 or k.max() > 2 * n_tgt:
        raise ValueError("allele count outside 0 .. 2 n")
    ref = np.zeros((n_sites, 3), dtype=np.int8)
    ref[inv >= 0] = 2
    tgt = np.clip(k[:, None] - 2 * np.arange(n_tgt)[None, :], 0, 2).astype(np.int8)
    srcs = []
    for g in range(2):
        s = np.where(on[g], 2, 0)
        s = np.where(inv >= 0, np.where(inv == g, 0, 2), s)
        srcs.append(s.astype(np.int8)[:, None])
    pos = 5 + 2 * np.arange(n_sites, dtype=np.int64)
    specs = []
    for g, anc, q, x in zip(set_groups, set_anc, quantiles, xs):
        y = [(">=", 0.0), (">=", 0.0)]
        y[g] = ("=", 1.0)
        specs.append(dict(w=0.5, x=float(x), quantile=float(q), y_list=y, anc=bool(anc)))
    f = k.astype(np.float64) / np.float64(2 * n_tgt)
    eff = np.where(inv >= 0, 1.0 - f, f)
    conds = [(on[g] | ((inv == g) & (not anc))) for g, anc in zip(set_groups, set_anc)]
    union = np.any(conds, axis=0)
    used = 1 + len(specs) * (1 if all(set_anc) else 2)
    claims, windows = [], []
    for lo, hi in ranges:
        if not (0 <= lo < hi <= n_sites):
            raise ValueError(f"window [{lo}, {hi}) outside the block of {n_sites} sites")
        t0, t1 = lo // TILE, (hi + TILE - 1) // TILE
        per_set = [rank_claims(eff[lo:hi][c[lo:hi]], s["quantile"]) for c, s in zip(conds, specs)]
        claims.append(dict(nt=t1 - t0, row_words=(t1 - t0) * used, stored=int(union[t0 * TILE : t1 * TILE].sum()),
                           n_cond=[int(c[lo:hi].sum()) for c in conds], k0=[r["k0"] for r in per_set],
                           members=[r["members"] for r in per_set], gap=[r["gap"] for r in per_set]))  # fmt: skip
        windows.append((int(pos[lo]) - 1, int(pos[hi - 1]) + 1))
    return WindowCase(name, [ref, tgt, *srcs], [2, 2, 2, 2], pos, specs, list(ranges), windows, claims, list(pins))


OFFSETS = (0, 1, 63)  # where a window starts inside its first tile
_FIVE = dict(set_groups=[0, 1, 0, 1, 0], set_anc=[True] * 5, quantiles=[0.95, 0.5, 0.3, 1.0, 0.0], xs=[0.5, 0.2, 0.0, 0.9, 0.5])


def ks_of_digit(d: int, n_tgt: int) -> np.ndarray:
    k = np.arange(2 * n_tgt + 1)
    return k[first_digit(k / np.float64(2 * n_tgt)) == d]


# ---- n_cond at kWaveCap ------------------------------------------------------------------------


def ncond_case(target: int) -> WindowCase:
    """A set with exactly ``target`` condition sites per window (rank counting up to kWaveCap, the digit
    histogram beyond), 1 000 target individuals: nearly every value distinct.  Sets 0, 2 and 4 listen to that
    switch (in the shared form one wave answers sets 0 and 4 from the same LDS slice), sets 1 and 3 to a light one."""
    name = f"ncond_{target}"
    rng = _rng(name)
    region = 10 * TILE
    length = 2 * target + 6
    n_sites = region * len(OFFSETS)
    on, ranges, pins = np.zeros((2, n_sites), bool), [], []
    for r, off in enumerate(OFFSETS):
        base = r * region
        lo, hi = base + off, base + off + length
        on[0, _pick(rng, lo, hi, target)] = True
        on[1, _pick(rng, lo, hi, 40)] = True
        if off:
            on[0, base] = True  # in the edge tile, before the window
        on[0, hi] = True  # in the last tile, behind the window
        ranges.append((lo, hi))
        pins.append(("n_cond", r, 0, target))
    k = rng.integers(0, 2001, n_sites)
    return _assemble(name, 1000, k, on, np.full(n_sites, -1), ranges=ranges, pins=pins, **_FIVE)


# ---- stored frequencies at kFreqCap --------------------------------------------------------------


def freqcap_case(variant: str, total: int) -> WindowCase:
    """The tiles a window spans hold exactly ``total`` stored frequencies (candidates mode: the union of the sets'
    condition sites, the edge tiles' sites outside [lo, hi) included).  ``heavy``: one switch carries all of them
    (n_cond = the list capacity at the limit); ``union``: no set exceeds 600; ``inverted``: no ancestral alleles,
    half of the values enter as 1 - v."""
    name = f"freqcap_{variant}_{total}"
    rng = _rng(name)
    length, region = 28 * TILE, 32 * TILE
    n_sites = region * len(OFFSETS)
    on, inv = np.zeros((2, n_sites), bool), np.full(n_sites, -1)
    ranges, pins = [], []
    for r, off in enumerate(OFFSETS):
        base = r * region
        lo, hi = base + off, base + off + length
        t_end = (hi + TILE - 1) // TILE * TILE
        outside = np.concatenate([_pick(rng, base, lo, min(2, lo - base)), _pick(rng, hi, t_end, min(2, t_end - hi))]).astype(np.int64)
        inside = _pick(rng, lo, hi, total - outside.size)
        if variant == "union":
            g0 = rng.choice(inside, size=600, replace=False)
            rest = np.setdiff1d(inside, g0)
            g1 = np.concatenate([rest, rng.choice(g0, size=600 - rest.size, replace=False)])
            on[0, g0] = True
            on[1, g1] = True
            on[1, outside] = True
        else:
            on[0, inside] = True
            on[0, outside] = True
            if variant == "inverted":
                flipped = rng.choice(inside, size=inside.size // 2, replace=False)
                inv[flipped] = 0
                inv[outside[:1]] = 0
            on[1, rng.choice(np.setdiff1d(inside, np.flatnonzero(inv >= 0)), size=300, replace=False)] = True
        ranges.append((lo, hi))
        pins.append(("stored", r, None, total))
    k = rng.integers(0, 101, n_sites)
    anc = variant != "inverted"
    return _assemble(name, 50, k, on, inv, [0, 1, 0, 1], [anc] * 4, [0.95, 0.5, 0.0, 1.0], [0.5, 0.2, 0.0, 0.9], ranges, pins)


# ---- tiles and row words ---------------------------------------------------------------------------


def tiles_case(n_sets: int, anc: bool) -> WindowCase:
    """Windows of exactly the number of tiles whose rows still fit (kLdsTiles rows, kRowWords words of ``used``
    per row) and one more, aligned and starting mid-tile; a window of nt_at * 64 sites that starts mid-tile spans
    nt_at + 1 tiles."""
    c = constants()
    used = 1 + n_sets * (1 if anc else 2)
    nt_at = min(c["kLdsTiles"], c["kRowWords"] // used)
    name = f"tiles_{n_sets}sets_{'anc' if anc else 'noanc'}"
    rng = _rng(name)
    n_tiles = nt_at + 2
    n_sites = n_tiles * TILE
    on = np.zeros((2, n_sites), bool)
    for t in range(n_tiles):
        on[0, _pick(rng, t * TILE, (t + 1) * TILE, 3)] = True
        if t % 3 == 0:
            on[1, _pick(rng, t * TILE, (t + 1) * TILE, 1)] = True
    w = nt_at * TILE
    ranges = [(0, w), (0, w + TILE), (1, w), (63, w), (1, 1 + w), (63, 63 + w)]
    want_nt = [nt_at, nt_at + 1, nt_at, nt_at, nt_at + 1, nt_at + 1]
    pins = [("nt", i, None, v) for i, v in enumerate(want_nt)] + [("row_words", i, None, v * used) for i, v in enumerate(want_nt)]
    cyc_q, cyc_x = [0.95, 0.5, 0.0, 1.0, 0.3, 0.777], [0.5, 0.2, 0.0, 0.9]
    k = rng.integers(0, 17, n_sites)
    return _assemble(name, 8, k, on, np.full(n_sites, -1), [s % 2 for s in range(n_sets)], [anc] * n_sets,
                     [cyc_q[s % 6] for s in range(n_sets)], [cyc_x[s % 4] for s in range(n_sets)], ranges, pins)  # fmt: skip


# ---- members of the bin that holds rank k0 -----------------------------------------------------------


def _region_len() -> int:
    # a window of these cases spans at most kFreqCap / 64 tiles also when it starts mid-tile: a dense pass (64
    # stored frequencies per tile) still fits them into LDS
    return (constants()["kFreqCap"] // TILE - 1) * TILE


def binmember_case(variant: str, members: int) -> WindowCase:
    """About 600 condition sites; the first-digit bin that holds the wanted rank has exactly ``members`` members.
    ``distinct``: eight distinct values in the bin (the select separates them at the next level); ``onevalue``: all
    members are one number (the select runs to its last level); ``ends``: the bins of 0.0 and of exactly 1.0 hold
    ``members`` each and quantiles 0.0 and 1.0 want them."""
    name = f"binmembers_{variant}_{members}"
    rng = _rng(name)
    n_tgt, digit = 1000, 100
    length = _region_len()
    region = length + 2 * TILE
    n_sites = region * len(OFFSETS)
    on, k = np.zeros((2, n_sites), bool), np.zeros(n_sites, dtype=np.int64)
    ranges, pins = [], []
    in_bin = ks_of_digit(digit, n_tgt)
    for r, off in enumerate(OFFSETS):
        lo = r * region + off
        hi = lo + length
        if variant == "ends":
            n_mid = 86
            sites = rng.permutation(_pick(rng, lo, hi, 2 * members + n_mid))
            low, high, mid = sites[:members], sites[members : 2 * members], sites[2 * members :]
            k[low] = np.where(np.arange(members) < members - 21, 0, rng.choice(ks_of_digit(0, n_tgt), size=members))
            k[high] = 2 * n_tgt
            k[mid] = rng.integers(ks_of_digit(0, n_tgt).max() + 1, ks_of_digit(DIGITS - 1, n_tgt).max() + 1, n_mid)
            pins += [("members", r, 0, members), ("members", r, 1, members)]
        else:
            n_below, n_above = 200, 600 - 200 - members
            sites = rng.permutation(_pick(rng, lo, hi, 600))
            below, mine, above = sites[:n_below], sites[n_below : n_below + members], sites[n_below + members :]
            k[below] = rng.integers(0, in_bin.min() - 50, n_below)
            k[mine] = rng.choice(in_bin, size=members) if variant == "distinct" else in_bin[in_bin.size // 2]
            k[above] = rng.integers(in_bin.max() + 50, 2 * n_tgt + 1, n_above)
            pins.append(("members", r, 0, members))
        on[0, sites] = True
        on[1, sites[::9]] = True
        ranges.append((lo, hi))
    if variant == "ends":
        qs = [0.0, 1.0, 0.5, 0.999, 0.001]
    else:
        qs = [0.5, 0.4, 0.5, 0.7, (200 + members - 1) / 599]
    return _assemble(name, n_tgt, k, on, np.full(n_sites, -1), [0, 0, 1, 0, 0], [True] * 5, qs, [0.5, 0.2, 0.0, 0.9, 0.39], ranges, pins)


# ---- the wanted rank is the last member of its bin -----------------------------------------------------


def rank_end_case(n_cond: int) -> WindowCase:
    """``n_cond`` condition sites (n_cond - 1 a power of two: the virtual index (n - 1) q is exact): rank
    k0 = (n_cond - 1) / 2 is the LAST member of its bin, the bin behind it is empty, rank k0 + 1 opens the one after
    (sets 0, 2, 4: g = 0.25, 0, 0.75); the mirror sets 1, 3, 5 want ranks k0 - 1 and k0, both inside the bin."""
    name = f"rank_end_{n_cond}"
    rng = _rng(name)
    n_tgt, digit = 1000, 100
    k0 = (n_cond - 1) // 2
    in_bin, behind = ks_of_digit(digit, n_tgt), ks_of_digit(digit + 2, n_tgt)
    length = _region_len()
    region = length + 2 * TILE
    n_sites = region * len(OFFSETS)
    on, k = np.zeros((2, n_sites), bool), np.zeros(n_sites, dtype=np.int64)
    ranges = []
    for r, off in enumerate(OFFSETS):
        lo = r * region + off
        hi = lo + length
        sites = rng.permutation(_pick(rng, lo, hi, n_cond))
        n_bin = 40
        k[sites[: k0 + 1 - n_bin]] = rng.integers(0, in_bin.min() - 50, k0 + 1 - n_bin)
        k[sites[k0 + 1 - n_bin : k0 + 1]] = rng.choice(in_bin, size=n_bin)
        k[sites[k0 + 1 :]] = rng.integers(behind.min(), 2 * n_tgt + 1, n_cond - k0 - 1)
        k[sites[k0 + 1]] = behind.min()  # rank k0 + 1 opens the bin behind the empty one
        on[0, sites] = True
        on[1, sites[::7]] = True
        ranges.append((lo, hi))
    n1 = n_cond - 1
    qs = [(k0 + 0.25) / n1, (k0 - 1 + 0.75) / n1, k0 / n1, (k0 - 1 + 0.25) / n1, (k0 + 0.75) / n1, (k0 - 1) / n1]
    pins = []
    for r in range(len(OFFSETS)):
        for s in range(6):
            pins += [("k0", r, s, k0 - s % 2), ("gap", r, s, 0 if s % 2 else 2)]
        pins.append(("n_cond", r, 0, n_cond))
    return _assemble(name, n_tgt, k, on, np.full(n_sites, -1), [0] * 6, [True] * 6, qs, [0.5, 0.2, 0.0, 0.9, 0.39, 0.4], ranges, pins)


def rank_end_small_case() -> WindowCase:
    """Windows of two condition sites (in bins with an empty one between, and in one bin) and of one, for
    quantiles with g < 0.5, g >= 0.5 and g == 0 (and the maximum)."""
    name = "rank_end_small"
    n_tgt, digit = 1000, 100
    in_bin, behind = ks_of_digit(digit, n_tgt), ks_of_digit(digit + 2, n_tgt)
    region = 3 * TILE
    values = [(in_bin[0], behind[0]), (in_bin[0], in_bin[1]), (in_bin[0],)]
    n_sites = region * len(values) * len(OFFSETS)
    on, k = np.zeros((2, n_sites), bool), np.zeros(n_sites, dtype=np.int64)
    ranges, pins = [], []
    for i, vals in enumerate(values):
        for j, off in enumerate(OFFSETS):
            w = i * len(OFFSETS) + j
            lo = w * region + off
            hi = lo + 70
            sites = [lo, hi - 1][: len(vals)]  # the window's first and last site
            k[sites] = vals[::-1]  # the larger value first: site order is not rank order
            on[0, sites] = True
            on[0, hi] = True  # behind the window
            ranges.append((lo, hi))
            pins.append(("n_cond", w, 0, len(vals)))
            if len(vals) == 2:
                pins += [("gap", w, 0, 2 if i == 0 else 0), ("k0", w, 0, 0), ("k0", w, 2, 0), ("k0", w, 4, 1)]
    return _assemble(name, n_tgt, k, on, np.full(n_sites, -1), [0] * 5, [True] * 5, [0.25, 0.75, 0.0, 0.5, 1.0],
                     [0.5, 0.2, 0.0, 0.9, 0.39], ranges, pins)  # fmt: skip


# ---- the last tile of the block is a partial one -------------------------------------------------------


def block_edge_case(rest: int) -> WindowCase:
    """n_sites % 64 = ``rest``; windows that end at n_sites, the last site a condition site, kWaveCap + 1 of them."""
    name = f"block_edge_{rest}"
    rng = _rng(name)
    target = constants()["kWaveCap"] + 1
    n_sites = 9 * TILE + rest
    on = np.zeros((2, n_sites), bool)
    on[0, n_sites - 1] = True
    on[0, _pick(rng, 63, n_sites - 1, target - 1)] = True
    on[0, _pick(rng, 0, 63, 5)] = True
    on[1, _pick(rng, 0, n_sites, 40)] = True
    ranges = [(0, n_sites), (1, n_sites), (63, n_sites)]
    pins = [("n_cond", 2, 0, target)]
    return _assemble(name, 1000, rng.integers(0, 2001, n_sites), on, np.full(n_sites, -1), ranges=ranges, pins=pins, **_FIVE)


@lru_cache(maxsize=None)
def window_cases() -> tuple:
    c = constants()
    cap = c["kWaveCap"]
    out = [ncond_case(t) for t in (cap - 1, cap, cap + 1)]
    out += [freqcap_case(v, t) for v in ("heavy", "union", "inverted") for t in (c["kFreqCap"], c["kFreqCap"] + 1)]
    out += [tiles_case(7, True), tiles_case(4, False), tiles_case(20, False), tiles_case(20, True)]
    out += [binmember_case(v, m) for v in ("distinct", "onevalue", "ends") for m in (cap, cap + 1)]
    out += [rank_end_case(2 * cap + 1), rank_end_case(cap + 1), rank_end_small_case()]
    out += [block_edge_case(1), block_edge_case(63)]
    return tuple(out)


# ---- stream cases ----------------------------------------------------------------------------------


def stream_sizes() -> list:
    """Population sizes around the switch to the form that widens its packed fields several times
    (16 * kChunkIters individuals = kChunkIters rows per lane) and around twice that."""
    m = 16 * constants()["kChunkIters"]
    return [m - 16, m - 1, m, m + 1, m + 16, m + 17, m + 64, m + 65, 2 * m, 2 * m + 1]


STREAM_SITES = 130  # two full tiles and a tail of two sites
STREAM_PATTERNS = ("all 127", "all -128", "all -1", "all 63", "127 / -128", "-128 / 127", "127, missing at 0",
                   "127, missing at 15", "127, missing at 16", "127, missing at the last")  # fmt: skip


def stream_pattern_of_site(site: int) -> int:
    """Tile 0 cycles through the patterns, tile 1 is 63 everywhere (a whole tile below 64 takes the bytewise
    group sums), the tail holds an all-127 and an alternating row."""
    if site < TILE:
        return site % len(STREAM_PATTERNS)
    if site < 2 * TILE:
        return 3
    return (0, 4)[site - 2 * TILE]


def stream_rows(n_ind: int) -> np.ndarray:
    """int8 [STREAM_SITES][n_ind] of adversarial rows."""
    g = np.empty((STREAM_SITES, n_ind), dtype=np.int8)
    even = np.arange(n_ind) % 2 == 0
    for site in range(STREAM_SITES):
        p = stream_pattern_of_site(site)
        if p in (4, 5):
            g[site] = np.where(even == (p == 4), 127, -128)
        else:
            g[site] = (127, -128, -1, 63, 0, 0, 127, 127, 127, 127)[p]
            if p >= 6:
                g[site, min((0, 15, 16, n_ind - 1)[p - 6], n_ind - 1)] = -1
    return g


def stream_sources(n_src: int) -> np.ndarray:
    """int8 [STREAM_SITES][n_src]: a constant 127, a constant -128, and one that alternates site by site -- against
    the all -128 / all 127 rows every individual's |a - b| is 255."""
    s = np.empty((STREAM_SITES, 3), dtype=np.int8)
    s[:, 0], s[:, 1] = 127, -128
    s[:, 2] = np.where(np.arange(STREAM_SITES) % 2 == 1, 127, -128)
    return s[:, :n_src].copy()


def packed_rows(n_ind: int) -> np.ndarray:
    """Rows the 2-bit layout holds: all 2, all missing, 2 / missing alternating in both parities, all 1, all 0."""
    g = np.empty((STREAM_SITES, n_ind), dtype=np.int8)
    even = np.arange(n_ind) % 2 == 0
    for site in range(STREAM_SITES):
        p = site % 6 if site < TILE else (0 if site < 2 * TILE else (1, 2)[site - 2 * TILE])
        g[site] = (2, -1, 0, 0, 1, 0)[p]
        if p in (2, 3):
            g[site] = np.where(even == (p == 2), 2, -1)
    return g


def counts_reference(g: np.ndarray):
    """(dosage sum, called) per site in int64."""
    g = g.astype(np.int64)
    present = g >= 0
    return np.where(present, g, 0).sum(axis=1), present.sum(axis=1)


def absdiff_reference(g: np.ndarray, s: np.ndarray) -> np.ndarray:
    """int64 [n_src][n_sites]: sum over the individuals of |s - g| on the raw values."""
    return np.abs(s.astype(np.int64).T[:, :, None] - g.astype(np.int64)[None, :, :]).sum(axis=2)
