"""Shared inputs of the LD-compressed ``.pgen`` export tests (``sai convert --out-pfile --ld-compress``): matrices of
hard-call codes whose rows resemble earlier rows, with the int8 blocks they come from.

A case is ``pgen_export_cases.Case(name, family, codes, ploidies, block, want)``; ``want`` names what the case exists
for (the record types its rows must take, entry counts, ties) and ``tests/test_pgen_ld_cpu.py`` proves it with
``pgen_builder`` for every case.  ``reference(case)`` is the test writer's answer by the rule of the issue: run
``build_pgen(types=None)`` on each segment of 16 rows by itself, which gives the type list ``T``; the file is
``build_pgen(codes, types=T, len_bytes=LB)`` -- computed once per case."""

import numpy as np

import pgen_builder
from pgen_export_cases import Case, block_of, random_rows

SEGMENT = 16
ROW_COUNTS = (1, 15, 16, 17, 31, 32, 33)
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385)
WIDE = (40000, 65537)


def ld_panel(rng, n_rows, n, p_new=0.25, flips=2, p_swap=0.1, miss=0.005):
    """Blocks of near-copied rows: a row is drawn afresh with probability ``p_new`` (a rare allele mostly), else it is
    the row before with up to ``flips`` calls redrawn, 0 and 2 exchanged with probability ``p_swap``; ``miss`` of the
    calls of every row are missing.  Synthetic: what DESIGN_INGEST.md's table of LD sizes was made with."""
    rows, cur = [], None
    for _ in range(n_rows):
        if cur is None or rng.random() < p_new:
            f = min(0.5, 1.0 / rng.integers(1, 200)) if rng.random() < 0.7 else rng.random()
            cur = rng.binomial(2, f, n).astype(np.uint8)
        else:
            cur = cur.copy()
            k = rng.integers(0, flips + 1)
            idx = rng.integers(0, n, k)
            cur[idx] = rng.integers(0, 3, k)
            if rng.random() < p_swap:
                cur = pgen_builder.swap02(cur)
        row = cur.copy()
        row[rng.random(n) < miss] = 3
        rows.append(row)
    return np.array(rows, dtype=np.uint8)


def changed(row, where, step=1):
    """``row`` with the codes at ``where`` moved on by ``step`` (mod 4): every one of them differs."""
    out = np.array(row, dtype=np.uint8)
    out[np.asarray(where, dtype=np.int64)] = (out[np.asarray(where, dtype=np.int64)] + step) % 4
    return out


def _case(name, family, codes, ploidies=2, **want):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    return Case(name, family, codes, ploidies, block_of(codes, ploidies), want)


def build_cases():
    cases = []
    # row counts: the chain at both sides of a segment's edge, the last segment short
    for n_rows in ROW_COUNTS:
        rng = np.random.default_rng(50 + n_rows)
        cases.append(_case(f"{n_rows} rows x 83", "rows", ld_panel(rng, n_rows, 83, p_new=0.2)))
    # widths: 19 rows (a whole segment and a short one), the widest with 5
    for n in WIDTHS:
        rng = np.random.default_rng(7000 + n)
        cases.append(_case(f"width {n} x {19 if n < 16000 else 5}", "widths", ld_panel(rng, 19 if n < 16000 else 5, n, p_new=0.3), w=pgen_builder.index_width(n)))
    for n in WIDE:
        rng = np.random.default_rng(n)
        cases.append(_case(f"width {n} x 4", "wide", ld_panel(rng, 4, n, p_new=0.3, flips=40), w=pgen_builder.index_width(n)))
    # the chain, by hand
    rng = np.random.default_rng(11)
    n = 400
    dense = rng.integers(0, 4, n).astype(np.uint8)
    other = rng.integers(0, 4, n).astype(np.uint8)
    cases.append(_case("a row equal to its anchor", "chain", np.stack([dense, dense]), types=[0, 2], L=[None, 0], lengths=[100, 1]))
    cases.append(_case("a row equal to swap02(anchor)", "chain", np.stack([dense, pgen_builder.swap02(dense)]), types=[0, 3], L=[None, 0], lengths=[100, 1]))
    odd = rng.choice(np.array([1, 3], dtype=np.uint8), size=n)
    cases.append(_case("a base without 0 and 2: types 2 and 3 tie", "chain", np.stack([odd, changed(odd, [7, 200, 399], 2)]), types=[1, 2], tie=(2, 3)))
    zeros = np.zeros(n, dtype=np.uint8)
    cases.append(_case("type 2 ties with type 4", "chain", np.stack([zeros, changed(zeros, [3, 90, 250])]), types=[4, 2], tie=(2, 4)))
    half = np.array([0, 2] * 16, dtype=np.uint8)  # 32 samples: a one-bit record of 6 bytes, a dense one of 8
    cases.append(_case("type 1 ties with type 2", "chain", np.stack([changed(half, [1, 9, 20, 30], 2), half]), types=[1, 1], tie=(1, 2)))
    near = changed(dense, [5, 77, 390])
    cases.append(_case("the base is the anchor, not the type 2 row before", "chain", np.stack([dense, near, dense, near]), types=[0, 2, 2, 2], L=[None, 3, 0, 3]))
    cases.append(_case("a later row of another type becomes the base", "chain", np.stack([dense, other, other, changed(other, [9]), dense]), types=[0, 0, 2, 2, 0],
                       L=[None, None, 0, 1, None]))  # fmt: skip
    for n in (17, 400, 16385):
        rng = np.random.default_rng(n)
        first = rng.integers(0, 4, n).astype(np.uint8)
        rows = [first, changed(first, [0, n - 1]), pgen_builder.swap02(changed(first, [0, n - 1]))]
        cases.append(_case(f"differences at sample 0 and {n - 1}", "chain", np.stack(rows), types=[0, 2, 3], L=[None, 2, 2]))
    for L in (63, 64, 65):
        rng = np.random.default_rng(L)
        first = rng.integers(0, 4, 2002).astype(np.uint8)
        where = np.sort(rng.choice(2002, size=L, replace=False))
        rows = [first, changed(first, where), pgen_builder.swap02(changed(first, where, 3))]
        cases.append(_case(f"L = {L} against the base", "entries", np.stack(rows), types=[0, 2, 3], L=[None, L, L], G=-(-L // 64)))
    for L in (4095, 4096, 4097):
        rng = np.random.default_rng(L)
        first = rng.integers(0, 4, 40000).astype(np.uint8)
        where = np.sort(rng.choice(40000, size=L, replace=False))
        rows = [first, changed(first, where), pgen_builder.swap02(changed(first, where, 2))]
        cases.append(_case(f"40 000 samples, L = {L} against the base", "entries", np.stack(rows), types=[0, 2, 3], L=[None, L, L], G=-(-L // 64)))
    # missing calls in a base and in a row that lists against it
    rng = np.random.default_rng(3)
    first = rng.integers(0, 3, 300).astype(np.uint8)
    first[[0, 150, 299]] = 3
    rows = [first, changed(first, [0, 10]), changed(first, [150, 151], 3), pgen_builder.swap02(first)]
    cases.append(_case("missing calls in the base and in the rows", "chain", np.stack(rows), types=[0, 2, 2, 3], L=[None, 2, 2, 0]))
    # mixed ploidies: no heterozygous code in a haploid slot
    for n in (5, 37, 2002):
        rng = np.random.default_rng(n)
        pl = rng.integers(1, 3, n).astype(np.int32)
        pl[0], pl[n - 1] = 1, 2
        codes = ld_panel(rng, 33, n, p_new=0.2)
        codes[:, pl == 1] = np.where(codes[:, pl == 1] == 1, 2, codes[:, pl == 1])
        cases.append(_case(f"per-slot ploidies, {n} slots", "ploidies", codes, ploidies=pl))
        cases.append(_case(f"ploidy 1, {n} slots", "ploidies", np.where(codes == 1, 0, codes), ploidies=1))
    # rows drawn independently: nothing to gain
    rng = np.random.default_rng(500)
    cases.append(_case("independent rows", "independent", np.array([rng.binomial(2, rng.random(), 500) for _ in range(48)], dtype=np.uint8)))
    cases.append(_case("rows of every style", "independent", random_rows(np.random.default_rng(8), 40, 257)))
    # the LD panel of DESIGN_INGEST.md's table
    for n in (200, 2002):
        cases.append(_case(f"the LD panel at {n} samples", "panel", ld_panel(np.random.default_rng(7 + n), 640, n)))
    return cases


CASES = build_cases()
CASE_IDS = [c.name for c in CASES]
SMALL = [c for c in CASES if c.family != "panel"]
SMALL_IDS = [c.name for c in SMALL]


def unfit_cases():
    """(name, block, ploidies, codes, status): a value that does not fit planted in an anchor, in the row behind it (a
    near copy) and in a row of the second segment -- its code is 3, and the rows behind list against that."""
    out = []
    for n in (5, 37, 2002):
        for value, ploidy in ((-1, 2), (3, 2), (127, 2), (2, 1), (-128, 1)):
            rng = np.random.default_rng(1000 * n + value + 7 * ploidy)
            codes = ld_panel(rng, 20, n, p_new=0.15, miss=0.02)
            if ploidy == 1:
                codes = np.where(codes == 1, 0, codes).astype(np.uint8)
            block = block_of(codes, ploidy)
            status = [0] * 20
            for row, where in ((0, n // 2), (1, n - 1), (5, 0), (17, n // 3)):
                block[row, where], codes[row, where] = value, 3
                status[row] = n - where
            out.append((f"{value} at ploidy {ploidy}, {n} slots", block, ploidy, codes, status))
    return out


_reference = {}


def reference_of(key, codes):
    """(types [rows], records [rows] of bytes, file bytes) by the rule of the issue, once per ``key``."""
    if key not in _reference:
        codes = np.asarray(codes, dtype=np.uint8)
        types = []
        for s0 in range(0, len(codes), SEGMENT):
            types += [entry[2] for entry in pgen_builder.build_pgen(codes[s0 : s0 + SEGMENT])[1]]
        lb = max(1, (-(-codes.shape[1] // 4)).bit_length() + 7 >> 3)
        data, table = pgen_builder.build_pgen(codes, types=types, len_bytes=lb)
        _reference[key] = (types, [data[at : at + ln] for at, ln, _, _ in table], data)
    return _reference[key]


def reference(case):
    return reference_of(case.name, case.codes)


def plain_sizes(codes):
    """Per row the bytes of the smallest of the types 0, 1, 4, 6 and 7: what the writer gives without the option."""
    return [min(len(pgen_builder.encode(row, k)) for k in (0, 1, 4, 6, 7)) for row in codes]
