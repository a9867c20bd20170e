"""Shared inputs of the ``.pgen`` export tests: matrices of hard-call codes with the int8 blocks they come from.

A case is ``Case(name, family, codes uint8 [rows][n], ploidies, block int8 [rows][n], want)``: ``ploidies`` is 2, 1 or
one value per slot; ``block`` holds the dosages the readers would leave for ``codes``; ``want`` names what the case
exists for (the record types its rows must take, entry counts, group counts, index widths, varint widths) and
``tests/test_pgen_export_cpu.py`` proves it with ``pgen_builder`` for every case, so that a case cannot silently stop
exercising its boundary.  ``reference(case)`` is the test writer's answer -- per row the type
``argmin over (0, 1, 4, 6, 7) of (len(pgen_builder.encode(row, k)), k)`` and its bytes -- computed once per case."""

from collections import namedtuple

import numpy as np

import pgen_builder

Case = namedtuple("Case", "name family codes ploidies block want")

WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2002]
ROW_COUNTS = (1, 17, 130)
KINDS = (0, 1, 4, 6, 7)
BAD_INDEX = 0x7FFFFFFF
# every value that does not fit, with the ploidy it is planted at (those of the .bed export's tests)
UNFIT = [(-128, 2), (-3, 2), (-1, 2), (-2, 1), (2, 1), (3, 2), (4, 2), (127, 2), (3, 1), (4, 1), (127, 1), (-128, 1)]
DOSAGE = {2: np.array([0, 1, 2, -2], dtype=np.int8), 1: np.array([0, 99, 1, -1], dtype=np.int8)}  # code -> dosage; no het at ploidy 1


def block_of(codes, ploidies):
    """The int8 block whose encoding is ``codes``."""
    codes = np.asarray(codes, dtype=np.uint8)
    pl = np.broadcast_to(np.asarray(ploidies), (codes.shape[1],))
    block = np.where((pl == 2)[None, :], DOSAGE[2][codes], DOSAGE[1][codes]).astype(np.int8)
    assert not (block == 99).any(), "a heterozygous code in a haploid slot"
    return block


def sparse_row(rng, n, fill, n_entries, others=None):
    """``fill`` everywhere but at ``n_entries`` random samples, which take the other codes in turn."""
    others = [c for c in range(4) if c != fill] if others is None else others
    row = np.full(n, fill, dtype=np.uint8)
    where = np.sort(rng.choice(n, size=n_entries, replace=False))
    row[where] = [others[k % len(others)] for k in range(n_entries)]
    return row


def two_code_row(rng, n, lo, hi, n_entries):
    """Half ``lo``, half ``hi``, and ``n_entries`` samples of the two other codes."""
    row = rng.choice(np.array([lo, hi], dtype=np.uint8), size=n)
    others = [c for c in range(4) if c not in (lo, hi)]
    where = rng.choice(n, size=min(n_entries, n), replace=False)
    row[where] = [others[k % 2] for k in range(len(where))]
    return row


def random_rows(rng, n_rows, n, haploid=None):
    """Rows of every style in turn: dense, sparse against each constant, two codes, constant."""
    rows = []
    for r in range(n_rows):
        style = (r + int(rng.integers(8))) % 8
        if style == 0:
            row = rng.integers(0, 4, n).astype(np.uint8)
        elif style in (1, 2, 3):
            row = sparse_row(rng, n, (0, 2, 3)[style - 1], int(rng.integers(0, max(1, n // 12) + 1)))
        elif style == 4:
            lo, hi = sorted(rng.choice(4, size=2, replace=False).tolist())
            row = two_code_row(rng, n, lo, hi, int(rng.integers(0, max(1, n // 40) + 1)))
        elif style == 5:
            row = np.full(n, int(rng.integers(4)), dtype=np.uint8)
        elif style == 6:
            row = sparse_row(rng, n, 0, min(n, int(rng.integers(0, 4))))
        else:
            row = rng.choice(np.array([0, 0, 0, 0, 0, 0, 1, 2, 3], dtype=np.uint8), size=n)
        if haploid is not None:  # no heterozygous code in a haploid slot
            row[haploid & (row == 1)] = 2
        rows.append(row)
    return np.stack(rows)


def _case(name, family, codes, ploidies=2, **want):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    return Case(name, family, codes, ploidies, block_of(codes, ploidies), want)


def build_cases():
    cases = []
    # widths: every width at 1, 17 and 130 rows
    for n in WIDTHS:
        for n_rows in ROW_COUNTS:
            rng = np.random.default_rng(1000 * n + n_rows)
            cases.append(_case(f"width {n} x {n_rows}", "widths", random_rows(rng, n_rows, n), w=pgen_builder.index_width(n)))
    # type choices
    rng = np.random.default_rng(7)
    n = 400
    five = [rng.integers(0, 4, n), two_code_row(rng, n, 0, 2, 6), sparse_row(rng, n, 0, 9), sparse_row(rng, n, 2, 9), sparse_row(rng, n, 3, 9)]
    cases.append(_case("each of the five types", "types", np.stack(five), types=[0, 1, 4, 6, 7]))
    pairs = [(lo, hi) for lo in range(4) for hi in range(lo + 1, 4)]
    cases.append(_case("the six pairs of type 1", "types", np.stack([two_code_row(rng, n, lo, hi, 5) for lo, hi in pairs]), types=[1] * 6, pairs=pairs))
    tie = np.array([3] * 190 + [0] * 20 + [1] * 20, dtype=np.uint8)  # second and third tie: the pair is (1, 3)
    tie_top = np.array([0] * 100 + [2] * 100 + [1] * 3, dtype=np.uint8)  # first and second tie
    tie_all = np.array([0, 1, 2, 3] * 50, dtype=np.uint8)
    # A tie of the second and third counts never shows in a chosen record: the third code's samples are then entries,
    # as many as the second code has, and the list against the first code alone is smaller than one bit per sample
    # plus half of it.  The rows are sized with the tie all the same, and a tie of the first two is written.
    cases.append(_case("count ties: second and third", "types", tie[None, :], tie_pair=(1, 3)))
    cases.append(_case("count ties: first and second", "types", tie_top[None, :], tie_pair=(0, 2), types=[1]))
    cases.append(_case("count ties: all four", "types", tie_all[None, :], tie_pair=(2, 3)))
    cases.append(_case("constant rows", "types", np.stack([np.full(100, c, dtype=np.uint8) for c in (0, 2, 3, 1)]), types=[4, 6, 7, 1], L=0))
    for n in (1, 2, 3, 4):
        cases.append(_case(f"size ties at n = {n}", "types", np.stack([np.full(n, c, dtype=np.uint8) for c in (0, 2, 3, 1)]), types=[0, 0, 0, 0]))
    # entry counts
    for L in (0, 1, 63, 64, 65, 127, 128, 129):
        rng = np.random.default_rng(L)
        rows = [sparse_row(rng, 2002, fill, L) for fill in (0, 2, 3)] + [two_code_row(rng, 2002, 0, 2, L)]
        cases.append(_case(f"L = {L}", "entries", np.stack(rows), types=[4, 6, 7, 1], L=L, G=-(-L // 64)))
    # wide rows, the entries drawn evenly from the three other codes
    for L in (4095, 4096, 4097):
        rng = np.random.default_rng(L)
        cases.append(_case(f"40 000 samples, L = {L}", "wide", np.stack([sparse_row(rng, 40000, fill, L) for fill in (0, 3)]), types=[4, 7], L=L, G=-(-L // 64), w=2))
    rng = np.random.default_rng(70)
    far = np.zeros((3, 70000), dtype=np.uint8)
    far[0, [5, 30000, 69999]] = [1, 2, 3]
    far[1, [0, 16385, 32770]] = [3, 1, 2]
    far[2] = sparse_row(rng, 70000, 2, 300)
    cases.append(_case("70 000 samples, three entries far apart", "wide", far, types=[4, 4, 6], w=3, delta_bytes=3))
    rng = np.random.default_rng(100)
    cases.append(_case("100 000 samples, L = 16 384", "wide", np.stack([sparse_row(rng, 100000, fill, 16384) for fill in (0, 2)]), types=[4, 6], L=16384,
                       G=256, w=3, varint_L=3))  # fmt: skip
    for n in (16383, 16384, 16385):
        rng = np.random.default_rng(n)
        rows = [sparse_row(rng, n, 0, 700), rng.integers(0, 4, n).astype(np.uint8), two_code_row(rng, n, 0, 2, 90), sparse_row(rng, n, 3, 5)]
        for row in rows:  # something at both sides of the tile's edge
            row[n - 1] = 1
            row[min(n - 1, 16383)] = 1
            row[16382] = 1
        cases.append(_case(f"the LDS tile edge: {n} samples", "wide", np.stack(rows), types=[4, 0, 1, 7], w=2))
    # mixed ploidies
    for n in (5, 37, 2002):
        rng = np.random.default_rng(n)
        pl = rng.integers(1, 3, n).astype(np.int32)
        pl[0], pl[n - 1] = 1, 2
        cases.append(_case(f"per-slot ploidies, {n} slots", "ploidies", random_rows(rng, 17, n, haploid=pl == 1), ploidies=pl))
        cases.append(_case(f"ploidy 1, {n} slots", "ploidies", random_rows(rng, 7, n, haploid=np.ones(n, dtype=bool)), ploidies=1))
    return cases


CASES = build_cases()
CASE_IDS = [c.name for c in CASES]


def unfit_cases():
    """(name, block, ploidies, codes, status): a value that does not fit at the first, a middle and the last slot of
    the middle row of three, a second one behind it; and ploidies of 0 and 3."""
    out = []
    for n in (1, 5, 37, 2002):
        rng = np.random.default_rng(900 + n)
        for value, ploidy in UNFIT:
            for where in sorted({0, n // 2, n - 1}):
                mixed = np.where(np.arange(n) == where, ploidy, rng.integers(1, 3, n)).astype(np.int32)
                for label, ploidies in (("uniform", ploidy), ("mixed", mixed)):
                    pl = np.broadcast_to(np.asarray(ploidies), (n,))
                    codes = random_rows(rng, 3, n, haploid=pl == 1)
                    block = block_of(codes, ploidies)
                    block[1, where], codes[1, where] = value, 3
                    if where + 2 < n and pl[n - 1] == ploidy:  # a second one behind it: the lowest slot is reported
                        block[1, n - 1], codes[1, n - 1] = value, 3
                    out.append((f"{value} at ploidy {ploidy}, slot {where} of {n}, {label}", block, ploidies, codes, [0, n - where, 0]))
    for n in (5, 37):
        rng = np.random.default_rng(n)
        for bad in (0, 3):
            for where in sorted({0, n // 2, n - 1}):
                pl = rng.integers(1, 3, n).astype(np.int32)
                codes = random_rows(rng, 3, n, haploid=pl == 1)
                block = block_of(codes, pl)
                pl[where] = bad
                codes[:, where] = 3
                out.append((f"ploidy {bad} at slot {where} of {n}", block, pl, codes, [BAD_INDEX] * 3))
    return out


_reference = {}


def reference_of(key, codes):
    """(types [rows], records [rows] of bytes) by the test writer's rule, once per ``key``."""
    if key not in _reference:
        types, records = [], []
        for row in codes:
            options = {k: pgen_builder.encode(row, k) for k in KINDS}
            kind = min(KINDS, key=lambda k: (len(options[k]), k))
            types.append(kind)
            records.append(options[kind])
        _reference[key] = (types, records)
    return _reference[key]


def reference(case):
    return reference_of(case.name, case.codes)
