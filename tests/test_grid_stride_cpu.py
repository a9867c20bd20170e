"""The cases of tests/test_grid_stride_device.py, proved on the host before a GPU sees them.

Eleven kernels cap their grid at a small multiple of the CU count and take the rest of their work in a grid-stride
loop; the device tests run each of them at the smallest work count at which every block (or wave) makes at least two
passes of that loop and some make three: ``2 * cap + a small odd remainder``.  The data stay small because the rows
are narrow and because many output rows point at few distinct inputs (``row_in_batch`` for .bed / .geno, the ``rec`` /
``base`` tables for .pgen).  The builders here take the cap as an argument.  This file runs them at a cap of 8
through the host decoders and asserts that the host output equals the expectation, which is a numpy statement
(``expected`` of test_pgen_cpu, ``expect`` of test_bed_pack2_cpu and test_pgen_pack2_cpu, a 4-entry table per (ploidy,
flip) for .bed / .geno) applied to the distinct inputs once and gathered to the row order with numpy indexing -- so a
wrong expectation cannot pass as a kernel bug.  It also asserts the condition on the order of the .pgen rows at the
small cap and at the cap of a 256-CU device."""

import ctypes as C

import numpy as np
import pytest

import pgen_builder as B
import test_pgen_device as PD
from conftest import same_f64
from test_bed_pack2_cpu import BAD_INDEX
from test_bed_pack2_cpu import expect as bed_pack2_expect
from test_bed_pack2_cpu import pack_host as bed_pack_host
from test_bed_pack2_cpu import pack_numpy, tile_words, word_index
from test_pgen_cpu import BAD_RECORD, decode_host, expected, tables_of
from test_pgen_pack2_cpu import expect as pgen_pack2_expect
from test_pgen_pack2_cpu import pack_host as pgen_pack_host

CAP_SMALL = 8  # the cap of the host runs
CAP_MI355X = 16 * 256  # 16 blocks per CU, 256 CUs
PGEN_EXTRA_ROWS = 37  # rows beyond 2 * cap
BLOCK_THREADS = 256  # kDecodeBlock / kGenoBlock: threads, and 16-byte chunks, per block of the .bed / .geno decoders
TEXT, PACKED = 1, 2  # SAI_EIGENSTRAT_TEXT, SAI_EIGENSTRAT_PACKED
# dosage by (ploidy, flipped) and code, as test_plink_device / test_eigenstrat_device ::
# test_kernel_restates_the_table_and_refuses_bad_indices state it; a het at ploidy 1 is flagged and written as 0
BED_TABLE = {(2, 0): [2, -2, 1, 0], (2, 1): [0, 4, 1, 2], (1, 0): [1, -1, 0, 0], (1, 1): [0, 2, 0, 1]}  # by code 00, 01, 10, 11
GENO_TABLE = {(2, 0): [2, 1, 0, -2], (2, 1): [0, 1, 2, 4], (1, 0): [1, 0, 0, -1], (1, 1): [0, 0, 1, 2]}  # by g = 0, 1, 2, missing
BED_HET, GENO_HET = 2, 1
COARSE = {0: "dense", 1: "one bit", 4: "constant", 6: "constant", 7: "constant", 2: "difference", 3: "difference", "damaged": "damaged"}


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


# ---- .pgen: about 80 distinct records, referenced by all rows ----


def pgen_records(n, seed=0):
    """The distinct records of ``sample_ct`` n: ``kernel_case`` of test_pgen_device (types 0, 1, 4, 6, 7, types 2 and 3
    on a base of each of them, difference lists from empty to the longest the row allows) and the two damaged records
    of its test (a reserved type, a dense record one byte short).  ``codes[k]`` = the genotypes of record k or None for
    a damaged one; ``kinds[k]`` = its type, (type, type of its base) for types 2 and 3, or "damaged"."""
    rng = np.random.default_rng(7000 + n + seed)
    matrix, types = PD.kernel_case(n, rng)
    data, table = B.build_pgen(matrix, types, wide_types=True, len_bytes=4)
    rec, base = tables_of(table)
    kinds = [(t[2] & 7, table[t[3]][2] & 7) if t[2] & 7 in (2, 3) else t[2] & 7 for t in table]
    assert rec[0][2] == 0 and rec[1][2] == 2
    rec = np.vstack([rec, [rec[1][0], rec[1][1], 5], [rec[0][0], max(0, rec[0][1] - 1), rec[0][2]]])
    base = np.vstack([base, [[-1] * 3] * 2])
    return dict(n=n, data=data, rec=rec, base=base, codes=list(matrix) + [None, None], kinds=kinds + ["damaged"] * 2)


def wide_pgen_records(n=16384 + 600):
    """A dozen distinct records of more than one LDS window of samples (``test_rows_wider_than_one_lds_window`` of
    test_pgen_pack2_device): dense, one-bit, constant and difference records whose lists cross sample 16 384, and the
    two damaged ones."""
    rng = np.random.default_rng(n)
    matrix, types = np.zeros((10, n), dtype=np.uint8), [0, 1, 2, 3, 4, 2, 6, 3, 7, 2]
    for r, kind in enumerate(types):
        if kind == 0:
            matrix[r] = rng.integers(0, 4, n)
            continue
        if kind == 1:
            matrix[r] = np.where(rng.random(n) < 0.3, 2, 0)
        elif kind in (2, 3):
            matrix[r] = matrix[r - 1] if kind == 2 else B.swap02(matrix[r - 1])
        else:
            matrix[r] = {4: 0, 6: 2, 7: 3}[kind]
        where = np.union1d(rng.choice(np.arange(16384 - 700, n), size=int(rng.integers(130, 400)), replace=False), rng.integers(0, n, size=20))
        matrix[r, where] = (matrix[r, where] + rng.integers(1, 4, len(where))) % 4
    data, table = B.build_pgen(matrix, types, wide_types=True, len_bytes=2)
    assert [t[2] & 7 for t in table] == types
    rec, base = tables_of(table)
    kinds = [(t[2] & 7, table[t[3]][2] & 7) if t[2] & 7 in (2, 3) else t[2] & 7 for t in table]
    rec = np.vstack([rec, [rec[1][0], rec[1][1], 5], [rec[8][0], rec[8][1] - 3, rec[8][2]]])  # a reserved type; a type 7 list cut short
    base = np.vstack([base, [[-1] * 3] * 2])
    return dict(n=n, data=data, rec=rec, base=base, codes=list(matrix) + [None, None], kinds=kinds + ["damaged"] * 2)


def every_pair_walk(k):
    """A walk over the kinds 0 .. k - 1 in which every ordered pair, a kind with itself included, is consecutive exactly
    once: k * k + 1 entries (an Euler circuit of the complete directed graph with loops)."""
    nxt, stack, walk = [0] * k, [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            nxt[v] += 1
            stack.append(nxt[v] - 1)
        else:
            walk.append(stack.pop())
    return walk[::-1]


def coarse_of(kind):
    return COARSE[kind[0] if isinstance(kind, tuple) else kind]


def pairs_at_stride(labels, g):
    return {(labels[r], labels[r + g]) for r in range(len(labels) - g)}


def pgen_row_order(kinds, rows, cap, seed):
    """-> (record of every row, "fine" or "coarse").  A block takes the rows r, r + g, r + 2 g, ... with g = min(rows,
    cap), so what one iteration leaves for the next is decided by the pairs (kind of row r, kind of row r + g).  There
    are rows - g such pairs.  Where that is enough for the square of the number of kinds (16: types 0, 1, 4, 6, 7, types
    2 and 3 on each of these bases, damaged) every ordered pair of kinds is laid along the strides -- "fine"; at the
    small cap of the host runs (45 pairs) it is every ordered pair of the five ways a row is expanded (dense, one bit,
    constant, difference from a base, damaged) -- "coarse".  The remaining rows are drawn at random."""
    rng = np.random.default_rng(seed)
    g = min(rows, cap)
    fine = sorted(set(kinds), key=str)
    level = "fine" if rows - g >= len(fine) ** 2 else "coarse"
    label = [k if level == "fine" else coarse_of(k) for k in kinds]
    names = sorted(set(label), key=str)
    members = {name: [k for k, lab in enumerate(label) if lab == name] for name in names}
    assert rows - g >= len(names) ** 2
    order = rng.integers(0, len(kinds), size=rows)
    walk, at = every_pair_walk(len(names)), 0
    for c in range(g):  # the chain of rows c, c + g, c + 2 g, ... continues the walk from the kind the chain before ended on
        chain = range(c, rows, g)
        for r in chain:
            if at < len(walk):
                order[r] = rng.choice(members[names[walk[at]]])
                at += 1
        if at >= len(walk):
            break
        at -= 1
    assert at >= len(walk)
    return order, level


def check_pgen_order(kinds, order, cap, level):
    """The condition of ``pgen_row_order``, asserted on the order it built."""
    g = min(len(order), cap)
    coarse = [coarse_of(kinds[k]) for k in order]
    names = set(COARSE.values())
    assert pairs_at_stride(coarse, g) == {(a, b) for a in names for b in names}
    assert ("damaged", "dense") in pairs_at_stride(coarse, g) and ("dense", "damaged") in pairs_at_stride(coarse, g)
    if level == "fine":
        fine = [kinds[k] for k in order]
        names = set(kinds)
        assert names == {0, 1, 4, 6, 7, "damaged"} | {(t, b) for t in (2, 3) for b in (0, 1, 4, 6, 7)}
        assert pairs_at_stride(fine, g) == {(a, b) for a in names for b in names}
        assert set(order.tolist()) == set(range(len(kinds)))  # every distinct record is some row, the longest lists too


def pgen_selection(n, n_slots, form, seed):
    """-> (cols, ploidies, first_col, uniform): "run 1" / "run 2" = the promised form (a run of consecutive columns at one
    ploidy), "list" = a permuted column list with repeats and mixed ploidies."""
    rng = np.random.default_rng(seed)
    if form == "list":
        return rng.integers(0, n, size=n_slots).astype(np.int32), rng.integers(1, 3, size=n_slots).astype(np.int32), -1, 0
    ploidy, first = int(form[-1]), min(3, n - n_slots)
    return np.arange(first, first + n_slots, dtype=np.int32), np.full(n_slots, ploidy, dtype=np.int32), first, ploidy


def pgen_decode_case(records, rows, cap, n_slots, form, seed):
    """Rows in the order of ``pgen_row_order``, flips mixed; ``want`` / ``want_status`` = ``expected`` on the distinct
    (record, flip) pairs, gathered."""
    codes, n = records["codes"], records["n"]
    order, level = pgen_row_order(records["kinds"], rows, cap, seed)
    flip = np.random.default_rng(seed + 1).integers(0, 2, size=rows).astype(np.uint8)
    cols, ploidies, first_col, uniform = pgen_selection(n, n_slots, form, seed + 2)
    sound = [k for k, c in enumerate(codes) if c is not None]
    table = np.zeros((2, len(codes), n_slots), dtype=np.int8)
    status = np.full(len(codes), BAD_RECORD, dtype=np.int32)
    for f in (0, 1):
        table[f, sound], status[sound] = expected(np.stack([codes[k] for k in sound]), cols, ploidies, [f] * len(sound))
    return dict(records, order=order, level=level, rec=records["rec"][order], base=records["base"][order], flip=flip, cols=cols,
                ploidies=ploidies, first_col=first_col, uniform=uniform, want=table[flip, order], want_status=status[order])  # fmt: skip


# ---- the packed2 layout, vectorised ----


def words_of_fields(fields):
    """uint8 [...][individuals] of 2-bit fields -> uint32 [...][ceil(individuals / 16)], field i in bits [2 (i % 16), +2)
    of word i / 16; padding individuals 0."""
    n_ind = fields.shape[-1]
    n_words = -(-n_ind // 16)
    padded = np.zeros(fields.shape[:-1] + (n_words * 16,), dtype=np.uint32)
    padded[..., :n_ind] = fields
    return np.bitwise_or.reduce(padded.reshape(fields.shape[:-1] + (n_words, 16)) << (2 * np.arange(16, dtype=np.uint32)), axis=-1)


def place_sites(block, site_words, lo, n_ind, n_sites=None):
    """Write the words of the sites [lo, lo + len(site_words)) into ``block`` (uint32, the layout of saihip.h through
    ``word_index`` of test_bed_pack2_cpu); with ``n_sites`` the padding sites of the last tile are set to all ones."""
    ind = 16 * np.arange(site_words.shape[1])[None, :]
    block[word_index(np.arange(lo, lo + len(site_words))[:, None], ind, n_ind)] = site_words
    if n_sites is not None and n_sites % 64:
        block[word_index(np.arange(n_sites, -(-n_sites // 64) * 64)[:, None], ind, n_ind)] = 0xFFFFFFFF


def pgen_pack2_case(records, rows, cap, n_ind, fast, ploidy, seed, out_row0=0):
    """The same records and orders into the packed2 layout; ``site_words`` / ``want_status`` / ``want_unfit`` = ``expect``
    of test_pgen_pack2_cpu on the distinct (record, flip) pairs, gathered."""
    codes, n = records["codes"], records["n"]
    order, level = pgen_row_order(records["kinds"], rows, cap, seed)
    rng = np.random.default_rng(seed + 1)
    flip = rng.integers(0, 2, size=rows).astype(np.uint8)
    first_col = min(5, n - n_ind) if fast else -1
    cols = np.arange(first_col, first_col + n_ind, dtype=np.int32) if fast else rng.integers(0, n, size=n_ind).astype(np.int32)
    parts = [pgen_pack2_expect(codes, [f] * len(codes), cols, ploidy) for f in (0, 1)]
    words = np.stack([words_of_fields(p[0]) for p in parts])
    status, unfit = np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts])
    return dict(records, order=order, level=level, rec=records["rec"][order], base=records["base"][order], flip=flip, cols=cols,
                first_col=first_col, ploidy=ploidy, n_ind=n_ind, out_row0=out_row0, n_sites=out_row0 + rows,
                site_words=words[flip, order], want_status=status[flip, order], want_unfit=unfit[flip, order])  # fmt: skip


def packed_block(case, fill=0xA5):
    """The whole block a call (or several) on ``case`` must leave: ``fill`` in the words of the sites before out_row0."""
    n_sites, n_ind = case["n_sites"], case["n_ind"]
    block = np.full(-(-n_sites // 64) * tile_words(n_ind), fill * 0x01010101, dtype=np.uint32)
    place_sites(block, case["site_words"], case["out_row0"], n_ind, n_sites)
    return block.view(np.uint8)


# ---- .bed / .geno into int8 ----


def decode_rows_for(n_chunks, n_slots, out_row0):
    """The fewest output rows from out_row0 on that take ``n_chunks`` aligned 16-byte chunks of the flat block."""
    chunks = lambda n_out: ((out_row0 + n_out) * n_slots + 15) // 16 - out_row0 * n_slots // 16  # noqa: E731 -- as the entry points count them
    n_out = max(1, (16 * n_chunks) // n_slots - 2)
    while chunks(n_out) < n_chunks:
        n_out += 1
    return n_out, chunks(n_out)


def decode_case(kind, n_slots, cap, form, seed, n_batch=173):
    """``kind`` = "bed", "packed" or "text"; 2 * cap * 256 + 5 chunks of 16 output bytes from 173 distinct batch rows,
    out_row0 such that the first chunk is shared with the rows before.  ``want`` / ``want_status`` = the 4-entry table of
    every (ploidy, flip) on the distinct rows, gathered; the lowest heterozygous ploidy-1 slot is the status."""
    rng = np.random.default_rng(seed)
    n_cols, out_row0 = n_slots + 9, 3
    assert (out_row0 * n_slots) % 16
    n_out, n_chunks = decode_rows_for(2 * cap * BLOCK_THREADS + 5, n_slots, out_row0)
    if kind == "text":
        record_bytes = n_cols + 1
        codes = rng.integers(0, 4, size=(n_batch, n_cols)).astype(np.uint8)
        records = np.concatenate([np.frombuffer(b"0129", dtype=np.uint8)[codes], np.full((n_batch, 1), 10, dtype=np.uint8)], axis=1).ravel()
    else:
        record_bytes = (n_cols + 3) // 4 if kind == "bed" else max(48, (n_cols + 3) // 4)
        records = rng.integers(0, 256, size=n_batch * record_bytes, dtype=np.uint8)  # any byte string is a valid row
        col = np.arange(n_cols)
        shift = 2 * (col % 4) if kind == "bed" else 6 - 2 * (col % 4)  # .geno: the first individual in the two most significant bits
        codes = (records.reshape(n_batch, record_bytes)[:, col // 4] >> shift.astype(np.uint8)) & 3
    if form == "list":
        cols, ploidies, first_col, uniform = rng.integers(0, n_cols, size=n_slots).astype(np.int32), rng.integers(1, 3, size=n_slots).astype(np.int32), -1, 0
    else:
        uniform, first_col = int(form[-1]), 5
        cols, ploidies = np.arange(first_col, first_col + n_slots, dtype=np.int32), np.full(n_slots, uniform, dtype=np.int32)
    table, het_code = (BED_TABLE, BED_HET) if kind == "bed" else (GENO_TABLE, GENO_HET)
    lut = np.array([[table[(pl, f)] for f in (0, 1)] for pl in (1, 2)], dtype=np.int8)  # [ploidy - 1][flip][code]
    picked = codes[:, cols]
    distinct = np.stack([lut[ploidies[None, :] - 1, f, picked] for f in (0, 1)])  # [flip][batch row][slot]
    het = (ploidies == 1)[None, :] & (picked == het_code)
    status = np.where(het.any(axis=1), n_slots - het.argmax(axis=1), 0).astype(np.int32)
    rib = rng.integers(0, n_batch, size=n_out).astype(np.int32)
    flip = rng.integers(0, 2, size=n_out).astype(np.uint8)
    return dict(kind=kind, encoding={"bed": 0, "text": TEXT, "packed": PACKED}[kind], records=records, record_bytes=record_bytes, n_batch=n_batch,
                n_cols=n_cols, n_slots=n_slots, cols=cols, ploidies=ploidies, first_col=first_col, uniform=uniform, out_row0=out_row0,
                rib=rib, flip=flip, n_chunks=n_chunks, want=distinct[flip, rib], want_status=status[rib])  # fmt: skip


# ---- .bed into packed2 ----


def bed_pack2_case(n_ind, n_tiles, fast, ploidy, seed, n_batch=41):
    """``n_tiles`` tiles of 64 sites, the last one partial, from 41 distinct batch rows; three ``row_in_batch`` entries are
    outside the batch (BAD_INDEX, a zero row).  ``site_words`` / ``want_status`` / ``want_unfit`` = ``expect`` of
    test_bed_pack2_cpu on the distinct (row, flip) pairs, gathered."""
    rng = np.random.default_rng(seed)
    n_cols = n_ind + 9
    row_bytes = (n_cols + 3) // 4
    n_sites = (n_tiles - 1) * 64 + 29
    rows = rng.integers(0, 256, size=n_batch * row_bytes, dtype=np.uint8)
    first_col = 5 if fast else -1
    cols = np.arange(5, 5 + n_ind, dtype=np.int32) if fast else rng.integers(0, n_cols, size=n_ind).astype(np.int32)
    parts = [bed_pack2_expect(rows, row_bytes, np.arange(n_batch), [f] * n_batch, n_cols, cols, ploidy) for f in (0, 1)]
    words = np.stack([words_of_fields(p[0]) for p in parts])
    status, unfit = np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts])
    rib = rng.integers(0, n_batch, size=n_sites).astype(np.int32)
    flip = rng.integers(0, 2, size=n_sites).astype(np.uint8)
    bad = np.array([7, n_sites // 2, n_sites - 1])
    ok = np.ones(n_sites, dtype=bool)
    ok[bad] = False
    safe = np.where(ok, rib, 0)
    site_words = np.where(ok[:, None], words[flip, safe], 0).astype(np.uint32)
    want_status, want_unfit = np.where(ok, status[flip, safe], BAD_INDEX).astype(np.int32), np.where(ok, unfit[flip, safe], 0).astype(np.int32)
    rib[bad] = [-1, n_batch, 2**31 - 1]
    return dict(rows=rows, row_bytes=row_bytes, rib=rib, flip=flip, n_cols=n_cols, cols=cols, first_col=first_col, ploidy=ploidy, n_ind=n_ind,
                n_sites=n_sites, out_row0=0, n_tiles=n_tiles, site_words=site_words, want_status=want_status, want_unfit=want_unfit)  # fmt: skip


def bed_pack2_tiles(n_ind, cap):
    """One wave per (tile, run of 8 groups), four waves per block.  3 individuals are one run per tile: 2 * 4 * cap + 3
    tiles.  513 individuals are nine groups = two runs: 4 * cap + 64 units, so every wave takes a second unit."""
    return 2 * 4 * cap + 3 if n_ind == 3 else (4 * cap + 64) // 2


# ---- the site family ----


def site_count(cap_tiles):
    return (2 * cap_tiles + 3) * 64 + 17


def site_mats(n_sites, sizes, raw, seed):
    """int8 [sites][individuals] per population: raw values over the whole range (DD's terms at their extremes), or
    dosages 0 .. 2 with 2 % missing calls (the decision has something to decide)."""
    rng = np.random.default_rng(seed)
    if raw:
        return [rng.integers(-128, 128, size=(n_sites, n)).astype(np.int8) for n in sizes]
    return [np.where(rng.random((n_sites, n)) < 0.02, -2, rng.integers(0, 3, size=(n_sites, n))).astype(np.int8) for n in sizes]


def absdiff_numpy(g, s):
    """int64 [individuals of s][sites]: sum over the individuals of g of |s - g|."""
    g64 = g.astype(np.int64)
    return np.stack([np.abs(g64 - s[:, j : j + 1].astype(np.int64)).sum(axis=1) for j in range(s.shape[1])])


def counts_numpy(mats):
    """int64 [populations][sites][2]: the sum of the called dosages and the number of called individuals."""
    return np.stack([np.stack([np.where(m >= 0, m, 0).sum(axis=1, dtype=np.int64), (m >= 0).sum(axis=1, dtype=np.int64)], axis=1) for m in mats])


def freq_numpy(counts, ploidy):
    """count / (ploidy * called) in float64, NaN where nothing is called."""
    alt, called = counts[:, 0].astype(np.float64), counts[:, 1] * ploidy
    out = np.full(len(alt), np.nan)
    np.divide(alt, called, out=out, where=called > 0)
    return out


def plane_words(bits):
    """bool [sites] -> uint64 [tiles], bit b of word t = site 64 t + b, spare bits 0."""
    padded = np.zeros(-(-len(bits) // 64) * 64, dtype=bool)
    padded[: len(bits)] = bits
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view("<u8").ravel()


def planes_numpy(n_sites, specs, decisions, candidates):
    """The flag planes of saihip.h, uint64 [tiles][3 * sets]: word 0 "any" (all ones from a dense pass, the OR of the
    conditions from a pass that stores candidates only), word 1 + s the condition of set s, word 1 + n + s site
    inverted -- those only when some set lacks ancestral alleles."""
    n = len(specs)
    words = np.zeros((-(-n_sites // 64), 3 * n), dtype=np.uint64)
    words[:, 0] = plane_words(np.any([d[0] for d in decisions], axis=0)) if candidates else np.uint64(0xFFFFFFFFFFFFFFFF)
    for s, (cond, inverted, _) in enumerate(decisions):
        words[:, 1 + s] = plane_words(cond)
        if not all(spec[3] for spec in specs):
            words[:, 1 + n + s] = plane_words(inverted)
    return words


def same_f64_all(a, b):
    """``same_f64`` of conftest on every pair of two float64 arrays: the same bits, or both NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    if a.shape != b.shape or not same.all():
        k = int(np.flatnonzero(~same.ravel())[0]) if a.shape == b.shape else -1
        assert a.shape == b.shape and same_f64(a.ravel()[k], b.ravel()[k]), (a.shape, b.shape, k)
    return True


def site_specs(n_src, n_sets):
    """(w, x, y_list, ancestral alleles available) per parameter set; one set: the one without ancestral alleles."""
    five = [(0.6, 0.3, [("=", 1.0), (">=", 0.5)], True), (0.9, 0.5, [("<=", 0.5), ("=", 0.0)], False), (1.0, 0.0, [(">=", 0.0), (">=", 0.0)], False),
            (0.3, 0.5, [(">=", 0.5), (">=", 0.5)], True), (0.5, 0.4, [("<", 1.0), (">", 0.0)], False)]  # fmt: skip
    picked = five if n_sets == 5 else five[1 : 1 + n_sets]
    return [(w, x, y[:n_src], anc) for w, x, y, anc in picked]


# ---- the host runs ----


@pytest.mark.parametrize("cap", [CAP_SMALL, CAP_MI355X])
@pytest.mark.parametrize("n", [70, 300])
def test_pgen_row_order_holds_every_pair_of_kinds_at_the_stride(n, cap):
    records = pgen_records(n)
    assert 60 <= len(records["codes"]) <= 90
    rows = 2 * cap + PGEN_EXTRA_ROWS
    order, level = pgen_row_order(records["kinds"], rows, cap, seed=n)
    assert level == ("coarse" if cap == CAP_SMALL else "fine") and rows > 2 * cap
    check_pgen_order(records["kinds"], order, cap, level)
    on_zero = [c for c, k in zip(records["codes"], records["kinds"]) if k == 4]  # a difference list against the constant 0 ...
    assert any(not c.any() for c in on_zero) and any(c.all() for c in on_zero)  # ... empty, and the longest: every sample


def test_every_pair_walk():
    for k in (1, 2, 5, 16):
        walk = every_pair_walk(k)
        assert len(walk) == k * k + 1 and set(zip(walk, walk[1:])) == {(a, b) for a in range(k) for b in range(k)}


@pytest.mark.parametrize("form", ["run 1", "run 2", "list"])
@pytest.mark.parametrize("n", [70, 300])
def test_pgen_decode_case_on_the_host(n, form):
    case = pgen_decode_case(pgen_records(n), 2 * CAP_SMALL + PGEN_EXTRA_ROWS, CAP_SMALL, n - 9, form, seed=n)
    out, status = decode_host(case["data"], case["rec"], case["base"], case["flip"], n, case["cols"], case["ploidies"])
    assert np.array_equal(out, case["want"]) and np.array_equal(status, case["want_status"])
    assert (status == BAD_RECORD).any() and (form != "run 1" or ((status > 0) & (status < BAD_RECORD)).any())
    check_pgen_order(case["kinds"], case["order"], CAP_SMALL, case["level"])


def test_wide_pgen_decode_case_on_the_host():
    records = wide_pgen_records()
    case = pgen_decode_case(records, CAP_SMALL + 41, CAP_SMALL, 300, "list", seed=5)
    assert (case["cols"] < 16384).any() and (case["cols"] >= 16384).any() and len(records["codes"]) == 12
    out, status = decode_host(case["data"], case["rec"], case["base"], case["flip"], case["n"], case["cols"], case["ploidies"])
    assert np.array_equal(out, case["want"]) and np.array_equal(status, case["want_status"]) and (status == BAD_RECORD).any()


@pytest.mark.parametrize("ploidy", [1, 2])
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "general"])
@pytest.mark.parametrize("n_ind", [3, 70, 300])
def test_pgen_pack2_case_on_the_host(n_ind, fast, ploidy):
    """One call from out_row0 = 64 k + 23 to the last site, and the same block in two calls cut inside a tile."""
    rows = 2 * CAP_SMALL + PGEN_EXTRA_ROWS
    case = pgen_pack2_case(pgen_records(300), rows, CAP_SMALL, n_ind, fast, ploidy, seed=n_ind, out_row0=64 + 23)
    want = packed_block(case)
    assert case["n_sites"] % 64 and (want[: 4 * tile_words(n_ind)] == 0xA5).all()  # the tile before out_row0 is nobody's
    for cuts in ([0, rows], [0, 30, rows]):
        got = np.full(want.size, 0xA5, dtype=np.uint8)
        for lo, hi in zip(cuts, cuts[1:]):
            st, uf = pgen_pack_host(case["data"], case["rec"][lo:hi], case["base"][lo:hi], case["flip"][lo:hi], 300, case["cols"], case["first_col"],
                                    ploidy, got, case["n_sites"], case["out_row0"] + lo)  # fmt: skip
            assert np.array_equal(st, case["want_status"][lo:hi]) and np.array_equal(uf, case["want_unfit"][lo:hi])
        assert np.array_equal(got, want)
    assert (case["want_status"] == BAD_RECORD).any() and (case["want_unfit"].any() == (ploidy == 2))


def host_decode(case):
    from sai_amd import _ffi, _ffi_eigenstrat, _ffi_plink

    n_out, n_slots = len(case["rib"]), case["n_slots"]
    out, status = np.full((n_out, n_slots), 99, dtype=np.int8), np.full(n_out, -7, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tail = (n_out, p(case["rib"]), p(case["flip"]), case["n_cols"], n_slots, p(case["cols"]), p(case["ploidies"]), p(out), p(status), 3)
    if case["kind"] == "bed":
        _ffi.check(_ffi_plink.load_host().sai_plink_decode_host(p(case["records"]), case["n_batch"], case["record_bytes"], *tail))
    else:
        _ffi.check(_ffi_eigenstrat.load_host().sai_eigenstrat_decode_host(case["encoding"], p(case["records"]), case["n_batch"],
                                                                          case["record_bytes"], 0, *tail))  # fmt: skip
    return out, status


@pytest.mark.parametrize("form", ["run 1", "run 2", "list"])
@pytest.mark.parametrize("n_slots", [2002, 17])
@pytest.mark.parametrize("kind", ["bed", "packed", "text"])
def test_decode_case_on_the_host(kind, n_slots, form):
    case = decode_case(kind, n_slots, CAP_SMALL, form, seed=n_slots)
    assert case["n_chunks"] >= 2 * CAP_SMALL * BLOCK_THREADS + 5
    out, status = host_decode(case)
    assert np.array_equal(out, case["want"]) and np.array_equal(status, case["want_status"])
    assert status.any() == (form != "run 2") and set(case["flip"].tolist()) == {0, 1}
    assert n_slots != 17 or len(set(case["rib"].tolist())) == 173  # 3 861 rows: every batch row is used


@pytest.mark.parametrize("ploidy", [1, 2])
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "general"])
@pytest.mark.parametrize("n_ind", [3, 513])
def test_bed_pack2_case_on_the_host(n_ind, fast, ploidy):
    case = bed_pack2_case(n_ind, bed_pack2_tiles(n_ind, CAP_SMALL), fast, ploidy, seed=n_ind)
    want = packed_block(case)
    got = np.full(want.size, 0xA5, dtype=np.uint8)
    st, uf = bed_pack_host(case["rows"], case["row_bytes"], case["rib"], case["flip"], case["n_cols"], case["cols"], case["first_col"], ploidy, got,
                           case["n_sites"], 0)  # fmt: skip
    assert np.array_equal(st, case["want_status"]) and np.array_equal(uf, case["want_unfit"]) and np.array_equal(got, want)
    assert (st == BAD_INDEX).sum() == 3 and case["n_sites"] % 64 and tile_words(513) == 8 * 256 + 64


def test_the_vectorised_layout_is_the_layout_of_pack_numpy():
    rng = np.random.default_rng(1)
    for n_ind in (1, 3, 16, 17, 70, 300, 513):
        for n_sites in (1, 64, 130):
            fields = rng.integers(0, 4, size=(n_sites, n_ind)).astype(np.uint8)
            block = np.zeros(-(-n_sites // 64) * tile_words(n_ind), dtype=np.uint32)
            place_sites(block, words_of_fields(fields), 0, n_ind, n_sites)
            assert np.array_equal(block.view(np.uint8), pack_numpy(fields))


def test_site_statements():
    """The numpy statements the site-family tests compare with, on a block small enough to restate them cell by cell."""
    assert site_count(CAP_MI355X) == 524_497 and site_count(CAP_MI355X) // 64 + 1 == 2 * CAP_MI355X + 4
    mats = site_mats(130, (5, 23, 1, 2), raw=True, seed=1)
    ad = absdiff_numpy(mats[1], mats[3])
    assert ad.shape == (2, 130) and ad[1, 77] == sum(abs(int(mats[3][77, 1]) - int(v)) for v in mats[1][77])
    dos = site_mats(130, (5, 23), raw=False, seed=2)
    dos[0][3] = -2
    counts = counts_numpy(dos)
    assert counts.shape == (2, 130, 2) and counts[1, 9].tolist() == [sum(int(v) for v in dos[1][9] if v >= 0), sum(1 for v in dos[1][9] if v >= 0)]
    freq = freq_numpy(counts[0], 2)
    assert np.isnan(freq[3]) and same_f64(freq[9], counts[0, 9, 0] / (2 * counts[0, 9, 1]))
    bits = np.random.default_rng(3).random(130) < 0.5
    words = plane_words(bits)
    assert words.dtype == np.uint64 and len(words) == 3 and [(int(words[s // 64]) >> (s % 64)) & 1 for s in range(130)] == bits.astype(int).tolist()
    assert int(words[2]) >> 2 == 0
    a = np.array([0.0, -0.0, np.nan, 1.5, 0.1 + 0.2])
    assert same_f64_all(a, a.copy())
    for k, other in enumerate([-0.0, 0.0, 1.0, np.nan, 0.3]):
        b = a.copy()
        b[k] = other
        with pytest.raises(AssertionError):
            same_f64_all(a, b)
