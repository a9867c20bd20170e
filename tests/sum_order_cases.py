"""Deterministic inputs for the two implementations of np.sum's addition order -- ``wave_numpy_sum`` (fourpop.hip, one
wavefront; fd / df / Danc / Dplus) and ``numpy_sum`` / ``PairwiseNode`` (numpy_sum.hpp, serial; DD's mean over the source
individuals) -- at the sizes where numpy's tree changes shape: the leaf limit, every depth up to the seven levels of
7689..8191 elements, the 8192-element piece and beyond it.  Plain numpy, no GPU: the sizes and limits are read out of
the sources (``constants``), the expectations are numpy's own (np.sum, np.mean), and three WRONG orders are restated in
plain Python so that test_sum_order_cases_cpu.py can show that the inputs tell them from numpy's;
test_sum_order_device.py runs the kernels on the same inputs.
"""

from __future__ import annotations

import re
from functools import lru_cache
from pathlib import Path

import numpy as np

from capacity_cases import parse_constants

CSRC = Path(__file__).resolve().parent.parent / "sai_amd" / "csrc"


def _one(values, what: str) -> int:
    found = {int(v) for v in values}
    if len(found) != 1:
        raise KeyError(f"{what}: expected one value, found {sorted(found)}")
    return found.pop()


@lru_cache(maxsize=None)
def constants() -> dict:
    """kMaxLeaves, kMaxDepth, kSumWaves, kPatternSlots of fourpop.hip; the leaf limit (128), the piece (8192) and the
    unrolled depth (7) as BOTH sources spell them -- a source that changes one of them moves the cases, two sources that
    disagree fail here."""
    four = (CSRC / "fourpop.hip").read_text()
    serial = (CSRC / "numpy_sum.hpp").read_text()
    named = parse_constants(four)
    out = {}
    for n in ("kMaxLeaves", "kMaxDepth", "kSumWaves", "kPatternSlots"):
        if n not in named:
            raise KeyError(f"fourpop.hip no longer defines constexpr int {n}")
        out[n] = named[n]
    leaf = [*re.findall(r"if \(len <= (\d+)\)", four), *re.findall(r"if \(n <= (\d+)\) return pairwise_leaf", serial)]
    piece = []
    for text in (four, serial):
        steps, caps = re.findall(r"o \+= (\d+)\)", text), re.findall(r"min\((\d+), n - o\)", text)
        if not steps or not caps:
            raise KeyError("the loop over np.sum's pieces is no longer spelled `o += N` / `min(N, n - o)`")
        piece += steps + caps
    if len(leaf) != 2:
        raise KeyError(f"expected one leaf limit in list_leaves and one in PairwiseNode, found {leaf}")
    out["leaf"] = _one(leaf, "leaf limit of fourpop.hip and numpy_sum.hpp")
    out["piece"] = _one(piece, "piece size of fourpop.hip and numpy_sum.hpp")
    out["node_depth"] = _one(re.findall(r"PairwiseNode<(\d+), E>::run\(e, off \+ o", serial), "depth numpy_sum unrolls to")
    return out


# ---- numpy's tree, restated ----------------------------------------------------------------------------


def list_leaves(off: int, n: int, leaf: int | None = None):
    """fourpop.hip's list_leaves, statement for statement: ([(offset, length, depth)] left to right, the highest stack
    index written)."""
    leaf = constants()["leaf"] if leaf is None else leaf
    stack = [(off, n, 0)]
    out, top = [], 0
    while stack:
        a, ln, d = stack.pop()
        if ln <= leaf:
            out.append((a, ln, d))
        else:
            n2 = ln // 2
            n2 -= n2 % 8
            stack.append((a + n2, ln - n2, d + 1))
            stack.append((a, n2, d + 1))
            top = max(top, len(stack) - 1)
    return out, top


def replay(leaf_sums, depths, max_depth: int) -> float:
    """wave_numpy_sum's rebuild of the tree from the leaves' depths (``pend`` / ``waiting``), statement for statement."""
    pend = [0.0] * max_depth
    waiting = 0
    piece = 0.0
    for v, d in zip(leaf_sums, depths):
        v = float(v)
        for lv in range(max_depth - 1, 0, -1):
            if d == lv and (waiting >> lv) & 1:
                v = pend[lv] + v
                waiting ^= 1 << lv
                d = lv - 1
        if d > 0:
            pend[d] = v
            waiting |= 1 << d
        else:
            piece = v
    return piece


def tree_depth(n: int) -> int:
    return max(d for _, _, d in list_leaves(0, n)[0])


@lru_cache(maxsize=None)
def first_size_of_depth(depth: int) -> int:
    """The smallest piece whose tree is ``depth`` levels deep (7689 for seven)."""
    return next(n for n in range(1, constants()["piece"] + 1) if tree_depth(n) == depth)


def _sizes() -> tuple:
    c = constants()
    leaf, piece = c["leaf"], c["piece"]
    seven = first_size_of_depth(c["node_depth"])
    return (1, 2, 7, 8, 9, 15, 16, 17, leaf - 1, leaf, leaf + 1, leaf + 7, leaf + 8, 2 * leaf - 1, 2 * leaf, 2 * leaf + 1,
            2 * leaf + 7, 1000, 2001, piece // 2 + 1, seven - 1, seven, seven + 4, piece - 1, piece, piece + 1, piece + 8,
            2 * piece + seven + 11)  # fmt: skip


SIZES = _sizes()
SEVEN_LEVEL = range(first_size_of_depth(constants()["node_depth"]), constants()["piece"])  # 7689..8191


# ---- plain Python: numpy's order and three wrong ones ------------------------------------------------------


def _leaf_sum(a: list, lo: int, n: int) -> float:
    if n < 8:
        res = 0.0
        for i in range(lo, lo + n):
            res += a[i]
        return res
    r = a[lo : lo + 8]
    body = n - n % 8
    for i in range(lo + 8, lo + body, 8):
        for j in range(8):
            r[j] += a[i + j]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(lo + body, lo + n):
        res += a[i]
    return res


def _node(a: list, lo: int, n: int, leaf: int, levels_left) -> float:
    if n <= leaf or levels_left == 0:
        return _leaf_sum(a, lo, n)
    n2 = n // 2
    n2 -= n2 % 8
    nxt = None if levels_left is None else levels_left - 1
    return _node(a, lo, n2, leaf, nxt) + _node(a, lo + n2, n - n2, leaf, nxt)


def tree_sum(a, leaf=None, levels=None, piece=0) -> float:
    """Pairwise sum of a sequence of doubles in Python floats.  The defaults are np.sum's order (the sources' leaf limit
    and piece); ``levels`` stops the halving after that many levels (whatever is left is one leaf), ``piece=None`` runs
    one tree over everything."""
    a = [float(v) for v in a]
    leaf = constants()["leaf"] if leaf is None else leaf
    piece = constants()["piece"] if piece == 0 else piece
    if piece is None:
        return _node(a, 0, len(a), leaf, levels)
    res = 0.0
    for o in range(0, len(a), piece):
        res += _node(a, o, min(piece, len(a) - o), leaf, levels)
    return res


def left_to_right(a) -> float:
    res = 0.0
    for v in a:
        res += float(v)
    return res


def six_levels(a) -> float:
    """The tree that stops six levels down: a 129..135-element node there is summed as one leaf (the bug the
    four-population kernel once had at 7689..8191 elements)."""
    return tree_sum(a, levels=constants()["node_depth"] - 1)


def no_pieces(a) -> float:
    """One pairwise tree over the whole array, without np.sum's 8192-element pieces."""
    return tree_sum(a, piece=None)


def wide_leaf(a) -> float:
    """Leaves of up to 136 elements instead of 128."""
    return tree_sum(a, leaf=constants()["leaf"] + 8)


def wrong_orders_for(n: int) -> list:
    """(name, function) of every wrong order that CAN differ from numpy's at ``n`` elements."""
    c = constants()
    out = []
    if n >= c["leaf"]:
        out.append(("left_to_right", left_to_right))
    if n in SEVEN_LEVEL:
        out.append(("six_levels", six_levels))
    if n > c["piece"]:
        out.append(("no_pieces", no_pieces))
    if c["leaf"] < n <= c["leaf"] + 8:
        out.append(("wide_leaf", wide_leaf))
    return out


# ---- windows over a 256-site block -------------------------------------------------------------------------

DD_SITES = 256
N_REF, N_TGT = 7, 3  # not powers of two: the per-individual differences have full mantissas
FIXED_WINDOWS = ((0, 256), (0, 63), (0, 64), (0, 65), (63, 129), (5, 5), (100, 37), (-9, 70), (150, 400))
N_RANDOM_WINDOWS = 40


def _random_windows(count: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 201, count)
    ln = rng.integers(1, 57, count)
    return [(int(a), int(a + b)) for a, b in zip(lo, ln)]


WINDOWS = (*FIXED_WINDOWS, *_random_windows(N_RANDOM_WINDOWS, 20261019))


def windows_of_count(count: int) -> tuple:
    """``count`` windows: WINDOWS first, further seeded ones after them."""
    more = _random_windows(max(0, count - len(WINDOWS)), 77)
    return (*WINDOWS, *more)[:count]


def clamp(windows, n_sites: int):
    """The kernels' clamp, min(max(v, 0), n_sites), of both ends; a reversed window becomes an empty one."""
    w = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    lo = np.clip(w[:, 0], 0, n_sites)
    hi = np.maximum(np.clip(w[:, 1], 0, n_sites), lo)
    return lo, hi


# ---- DD ----------------------------------------------------------------------------------------------


def dd_inputs(n: int):
    """uint32 [n][256] per-site terms of ``n`` source individuals against N_REF reference and N_TGT target individuals
    (|a - b| <= 255 per pair)."""
    rng = np.random.default_rng([4, n])
    ad_ref = rng.integers(0, 255 * N_REF + 1, size=(n, DD_SITES), dtype=np.uint32)
    ad_tgt = rng.integers(0, 255 * N_TGT + 1, size=(n, DD_SITES), dtype=np.uint32)
    return ad_ref, ad_tgt


def window_totals(ad: np.ndarray, windows) -> np.ndarray:
    """int64 [n_windows][n]: exact sums of the terms over every window."""
    c = np.zeros((ad.shape[0], ad.shape[1] + 1), dtype=np.int64)
    np.cumsum(ad, axis=1, dtype=np.int64, out=c[:, 1:])
    lo, hi = clamp(windows, ad.shape[1])
    return np.ascontiguousarray((c[:, hi] - c[:, lo]).T)


def dd_expected(ad_ref, ad_tgt, windows, n_ref: int = N_REF, n_tgt: int = N_TGT):
    """(d f64 [n_windows][n], dd f64 [n_windows]) as numpy forms them: exact integer totals, one division each, np.mean
    over the individuals."""
    tr, tt = window_totals(ad_ref, windows), window_totals(ad_tgt, windows)
    d = np.ascontiguousarray(tr.astype(np.float64) / n_ref - tt.astype(np.float64) / n_tgt)
    return d, np.array([np.mean(row) for row in d], dtype=np.float64)


def unsigned_inputs():
    """Three source individuals whose reference terms sit at and around 255 * 2^24 (the largest term of 2^24 reference
    individuals) and around 2^31 and 2^32 - 1; the target terms stay small.  Returns (ad_ref, ad_tgt) as uint32
    [3][256], n_ref_ind, n_tgt_ind."""
    top = 255 << 24
    rng = np.random.default_rng(9)
    around = np.array([top, top - 1, top - 2, top - 255, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, top + 1], dtype=np.uint32)
    ad_ref = np.empty((3, DD_SITES), dtype=np.uint32)
    ad_ref[0] = top
    ad_ref[1] = around[rng.integers(0, around.size, DD_SITES)]
    ad_ref[2] = rng.integers(1 << 31, 1 << 32, DD_SITES, dtype=np.uint64).astype(np.uint32)
    ad_tgt = rng.integers(0, 255 * N_TGT + 1, size=(3, DD_SITES), dtype=np.uint32)
    return ad_ref, ad_tgt, 1 << 24, N_TGT


def unsigned_expected(ad_ref, ad_tgt, n_ref: int, n_tgt: int, windows):
    """The same expectation from Python integers (no array dtype anywhere near the totals)."""
    lo, hi = clamp(windows, ad_ref.shape[1])
    r, t = ad_ref.tolist(), ad_tgt.tolist()
    d = [[float(sum(r[s][a:b])) / float(n_ref) - float(sum(t[s][a:b])) / float(n_tgt) for s in range(len(r))] for a, b in zip(lo.tolist(), hi.tolist())]
    totals = [[sum(r[s][a:b]) for s in range(len(r))] for a, b in zip(lo.tolist(), hi.tolist())]
    d = np.array(d, dtype=np.float64)
    return d, np.array([np.mean(row) for row in d], dtype=np.float64), totals


# ---- four populations ------------------------------------------------------------------------------------

SLOTS = ("abba", "baba", "bbaa", "baaa", "abaa", "abba_d", "baba_d")
FP_SITES = 30011
FP_NAN_REGION = 160  # the last sites of the block: the only ones with NaN frequencies
FP_OFFSETS = (0, 1, 7)  # lo % 8 of the windows of every size


def fourpop_freqs(n_src: int, has_out: bool, n_sites: int = FP_SITES, nan_region: int = FP_NAN_REGION) -> np.ndarray:
    """f64 [2 + n_src + has_out][n_sites]: arbitrary doubles in [0, 1) with full mantissas, some exact 0.0 and 1.0, some
    sites with tgt == src, and -- in the last ``nan_region`` sites only -- NaN in one population at a time (offsets 5,
    45, 85, 125: the second source (or the only one), tgt, ref, the outgroup (or the last source))."""
    rng = np.random.default_rng([11, n_src, int(has_out), n_sites])
    n_pops = 2 + n_src + int(has_out)
    f = rng.random((n_pops, n_sites)) ** 3
    for p in range(n_pops):
        f[p, rng.choice(n_sites, n_sites // 50, replace=False)] = 0.0
        f[p, rng.choice(n_sites, n_sites // 50, replace=False)] = 1.0
    same = rng.choice(n_sites, n_sites // 40, replace=False)
    for k, sites in enumerate(np.array_split(same, n_src)):
        f[2 + k, sites] = f[1, sites]
    if nan_region:
        base = n_sites - nan_region
        f[2 + min(1, n_src - 1), base + 5] = np.nan
        f[1, base + 45] = np.nan
        f[0, base + 85] = np.nan
        f[n_pops - 1, base + 125] = np.nan
    return f


@lru_cache(maxsize=None)
def fourpop_windows(extra_seven_level: int = 12) -> tuple:
    """Windows over FP_SITES sites: every length of SIZES at lo % 8 = 0, 1 and 7 (the seven-level lengths at
    ``extra_seven_level`` more starts: one node in sixty-five decides there), clear of the NaN sites; then the empty,
    the reversed and the clamped windows and those over the NaN sites."""
    rng = np.random.default_rng(3)
    free = FP_SITES - FP_NAN_REGION
    out = []
    for ln in SIZES:
        for r in FP_OFFSETS:
            k = int(rng.integers(0, (free - ln - r) // 8 + 1))
            out.append((8 * k + r, 8 * k + r + ln))
        if ln in SEVEN_LEVEL:
            out += [(int(a), int(a) + ln) for a in rng.integers(0, free - ln + 1, extra_seven_level)]
    out += [(5, 5), (100, 37), (-9, 70)]
    out += [(free - 30, free + 20), (free + 10, free + 40), (free + 30, free + 60), (free + 70, free + 100), (free + 110, FP_SITES + 50)]
    return tuple(out)


def pattern_products(r, t, s, o) -> np.ndarray:
    """f64 [7][n]: the per-site products of all seven slots, each built as oracle.pattern_sum builds it (ones, then
    ``prod *= f`` or ``prod *= 1 - f`` in population order); the donor slots put np.maximum(t, s) in both places."""
    d = np.maximum(t, s)
    rows = []
    for pops, pattern in (((r, t, s, o), "abba"), ((r, t, s, o), "baba"), ((r, t, s, o), "bbaa"), ((r, t, s, o), "baaa"),
                          ((r, t, s, o), "abaa"), ((r, d, d, o), "abba"), ((r, d, d, o), "baba")):  # fmt: skip
        prod = np.ones_like(r)
        for f, c in zip(pops, pattern):
            prod *= (1 - f) if c == "a" else f
        rows.append(prod)
    return np.stack(rows)


def window_products(freqs, n_src: int, has_out: bool, src: int, lo: int, hi: int) -> np.ndarray:
    n_sites = freqs.shape[1]
    (a,), (b,) = clamp([(lo, hi)], n_sites)
    sl = slice(int(a), int(b))
    o = freqs[2 + n_src, sl] if has_out else np.zeros(int(b - a))
    return pattern_products(freqs[0, sl], freqs[1, sl], freqs[2 + src, sl], o)


def ratios(sums) -> list:
    """fd, df, Danc, Dplus of seven sums, as oracle.four_pop_stats forms them (Python floats, oracle._ratio)."""
    from oracle.sai_oracle import _ratio

    abba, baba, bbaa, baaa, abaa, abba_d, baba_d = (float(v) for v in sums)
    return [_ratio(abba - baba, abba_d - baba_d), _ratio(abba - baba, abba + baba + 2 * bbaa), _ratio(baaa - abaa, baaa + abaa),
            _ratio(abba - baba + baaa - abaa, abba + baba + baaa + abaa)]  # fmt: skip


def fourpop_expected(freqs, n_src: int, has_out: bool, windows):
    """(sums f64 [n_windows][n_src][7], stats f64 [n_windows][n_src][4]): np.sum of the products, the ratios of those."""
    sums = np.empty((len(windows), n_src, len(SLOTS)), dtype=np.float64)
    stats = np.empty((len(windows), n_src, 4), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for w, (lo, hi) in enumerate(windows):
            for k in range(n_src):
                sums[w, k] = [np.sum(row) for row in window_products(freqs, n_src, has_out, k, lo, hi)]
                stats[w, k] = ratios(sums[w, k])
    return sums, stats


def launch_shapes() -> list:
    """(workgroups, n_windows, n_src): item counts that make window_pattern_sums launch 1, 7, 8, 9, 17 and 43
    workgroups -- below eight (xcd_contiguous is the identity), exactly eight, and above eight with a remainder --
    each with a partial last workgroup where the source count allows one."""
    waves = constants()["kSumWaves"]
    out = []
    for wg, n_src in ((1, 3), (7, 3), (8, 6), (9, 3), (17, 6), (43, 3)):
        n_w = -(-((wg - 1) * waves + 1) // n_src)  # the fewest windows that need ``wg`` workgroups
        if -(-n_w * n_src // waves) != wg:
            raise ValueError(f"no window count gives {wg} workgroups of {waves} items with {n_src} sources")
        out.append((wg, n_w, n_src))
    return out


SHAPE_SITES = 701


def shape_windows(n_windows: int) -> tuple:
    rng = np.random.default_rng([5, n_windows])
    lo = rng.integers(0, SHAPE_SITES - 300, n_windows)
    ln = rng.integers(1, 300, n_windows)
    return tuple((int(a), int(a + b)) for a, b in zip(lo, ln))


def zero_denominator_case():
    """(freqs [5][300], n_src 2, has_out, windows): sites 0..99 have tgt = src = 0 (only baaa is not zero: fd and df are
    0 / 0), sites 100..199 have ref = tgt = 1 (only bbaa is not zero: fd, Danc and Dplus are 0 / 0), sites 200..299
    are ordinary."""
    f = fourpop_freqs(2, True, n_sites=300, nan_region=0)
    f[1:4, :100] = 0.0
    f[0:2, 100:200] = 1.0
    return f, 2, True, ((0, 100), (10, 90), (33, 34), (100, 200), (120, 137), (200, 300), (0, 300), (90, 110))


# ---- site frequencies --------------------------------------------------------------------------------------


def freq_counts(n_pops: int, n_sites: int):
    """(counts uint32 [n_pops][n_sites][2] = (allele count, called individuals), ploidies): seeded small counts,
    sites where nobody is called (count 0, called 0), and sites with 2^24 called individuals of ploidy 255."""
    rng = np.random.default_rng([6, n_pops, n_sites])
    ploidy = [int(v) for v in rng.integers(1, 7, n_pops)]
    ploidy[0] = 255
    counts = np.zeros((n_pops, n_sites, 2), dtype=np.uint32)
    for p in range(n_pops):
        called = rng.integers(0, 400, n_sites).astype(np.int64)
        called[rng.random(n_sites) < 0.1] = 0
        if p == 0:
            called[::3] = 1 << 24
            called[0] = 1 << 24
        x = (rng.random(n_sites) * (called * ploidy[p] + 1)).astype(np.int64)
        x = np.minimum(x, called * ploidy[p])
        if p == 0:
            x[0] = called[0] * ploidy[0]  # frequency exactly 1 with a denominator of 255 * 2^24
        counts[p, :, 0] = x
        counts[p, :, 1] = called
    return counts, ploidy


def freq_expected(counts: np.ndarray, ploidy) -> np.ndarray:
    x = counts[:, :, 0].astype(np.float64)
    den = (counts[:, :, 1].astype(np.int64) * np.asarray(ploidy, dtype=np.int64)[:, None]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / den
