"""The planners that cut a read into batches -- ``_ingest.row_batches``, ``_ingest.span_batches`` and the transposed
branch of ``eigenstrat._Index.batches`` -- at EVERY buffer size from one byte below the smallest legal one to one above
the whole stream, on the indexes of tests/batch_sweep_cases.py and on seeded synthetic ones.  Pure numpy: the file is a
function of the offset, the buffer is rebuilt from a batch's ``reads``, and every row (and every base) must hold its
own bytes where the batch's table says it lies.  The cover conditions at the end of each test keep the sweep from
silently no longer reaching the cases it is written for."""

import numpy as np
import pytest

import batch_sweep_cases as S
import pgen_builder

HUGE = 1 << 40


def file_bytes(offsets):
    """The fake file: its byte at offset o."""
    o = np.asarray(offsets, dtype=np.int64)
    return ((o * 131 + (o >> 8) * 7 + (o >> 3)) % 251).astype(np.uint8)


def rebuild(reads, nbytes):
    """The staging buffer of a batch, and the check that its reads lie inside it and apart from each other."""
    buf = np.full(nbytes, 0xFD, dtype=np.uint8)  # 253: no byte of the fake file
    taken = np.zeros(nbytes, dtype=bool)
    for at, off, n in reads:
        assert 0 <= at and n >= 0 and at + n <= nbytes and off >= 0, (at, off, n, nbytes)
        assert not taken[at : at + n].any(), "two reads overlap in the buffer"
        taken[at : at + n] = True
        buf[at : at + n] = file_bytes(off + np.arange(n))
    return buf


def partition(batches, n_rows):
    at = 0
    for b in batches:
        assert b[0] == at and b[1] >= b[0], "the batches do not follow each other"
        at = b[1]
    assert at == n_rows


# ---- row_batches -------------------------------------------------------------------------------------------------


def row_plan(file_row, rb, data_offset, cap, read_through):
    from sai_amd.utils._ingest import row_batches

    return list(row_batches(file_row, rb, data_offset, cap, read_through, "FILE", "INDEX"))


def check_row_batches(file_row, rb, data_offset, cap, batches):
    partition(batches, len(file_row))
    for k0, k1, rib, n_batch_rows, reads in batches:
        assert 0 < n_batch_rows * rb <= cap and rib.dtype == np.int32 and len(rib) == k1 - k0
        assert sum(r[2] for r in reads) == n_batch_rows * rb  # the ranges lie back to back: no byte of the buffer is stale
        buf = rebuild(reads, n_batch_rows * rb).reshape(n_batch_rows, rb)
        assert ((rib >= 0) & (rib < n_batch_rows)).all()
        want = file_bytes(data_offset + file_row[k0:k1, None] * rb + np.arange(rb)[None, :])
        assert np.array_equal(buf[rib], want), (cap, k0, k1)


def sweep_row_batches(file_row, rb, data_offset, read_through):
    """Every cap from rb - 1 to one above the stream; the full check wherever the plan changes.  -> the plans"""
    file_row = np.asarray(file_row, dtype=np.int64)
    with pytest.raises(ValueError, match=rf"^SAI_AMD_INGEST_BUFFER of {rb - 1} bytes is smaller than one row of FILE \({rb} bytes\)$"):
        row_plan(file_row, rb, data_offset, rb - 1, read_through)
    plans, before = [], None
    whole = (int(file_row[-1] - file_row[0]) + 1) * rb
    for cap in range(rb, whole + 2):
        batches = row_plan(file_row, rb, data_offset, cap, read_through)
        key = S.plan_key(batches)
        assert all(b[3] * rb <= cap for b in batches)
        if key != before:
            check_row_batches(file_row, rb, data_offset, cap, batches)
            plans.append(batches)
        before = key
    assert len(plans[-1]) == 1
    return plans


@pytest.mark.parametrize("name", S.REQUESTS)
def test_row_planner_on_the_case_indexes(name):
    rows = S.selection(name)[0]
    n = len(rows)
    for rb, data_offset in ((12, 3), (46, 0)):  # a .bed and a text .geno of 45 samples
        for read_through in (0, rb, HUGE):
            if rb == 46 and read_through != HUGE:
                continue
            plans = sweep_row_batches(rows, rb, data_offset, read_through)
            firsts, lasts, empty = S.boundaries(plans)
            assert firsts == set(range(n)) and lasts == set(range(n))  # a boundary before and behind every selected row
            if read_through == 0:
                assert empty == 0  # nothing is read along, so no batch is without a row
            elif name == "sparse":
                assert empty > 0  # a batch of read-through rows only: a kernel call with zero rows
            assert max(len(p) for p in plans) >= min(n, 3)


@pytest.mark.parametrize("seed", range(36))
def test_row_planner_on_seeded_indexes(seed):
    rng = np.random.default_rng(seed)
    n, rb = int(rng.integers(1, 25)), int(rng.integers(1, 10))
    rows = np.cumsum(rng.choice([1, 1, 1, 2, 3, 7], size=n)) + int(rng.integers(0, 5))
    read_through = (0, rb, HUGE)[seed % 3]
    plans = sweep_row_batches(rows, rb, int(rng.integers(0, 50)), read_through)
    firsts, lasts, _ = S.boundaries(plans)
    assert firsts == set(range(n)) and lasts == set(range(n))


def test_row_planner_refuses_an_index_out_of_order():
    with pytest.raises(ValueError, match="INDEX: the index is not in file order"):
        row_plan(np.array([3, 5, 5]), 4, 0, 64, 0)
    assert row_plan(np.array([], dtype=np.int64), 4, 0, 64, 0) == []


# ---- span_batches ------------------------------------------------------------------------------------------------


def span_plan(rec, base, cap, read_through):
    from sai_amd.utils._ingest import span_batches

    return list(span_batches(rec, base, cap, read_through, "FILE"))


def check_span_batches(rec, base, cap, batches):
    partition(batches, len(rec))
    refetched = shared = 0
    for k0, k1, rows, bases, n_bytes, reads in batches:
        assert k1 > k0 and 0 < n_bytes <= cap, (cap, k0, k1, n_bytes)
        buf = rebuild(reads, n_bytes)
        assert np.array_equal(rows[:, 1:], rec[k0:k1, 1:]) and np.array_equal(bases[:, 1:], base[k0:k1, 1:])  # lengths and types as they were
        for r, k in enumerate(range(k0, k1)):
            at, n = int(rows[r, 0]), int(rec[k, 1])
            assert 0 <= at and at + n <= n_bytes
            assert np.array_equal(buf[at : at + n], file_bytes(rec[k, 0] + np.arange(n))), (cap, k)
            if base[k, 0] < 0:
                assert bases[r, 0] == -1
                continue
            at, n = int(bases[r, 0]), int(base[k, 1])
            assert 0 <= at and at + n <= n_bytes
            assert np.array_equal(buf[at : at + n], file_bytes(base[k, 0] + np.arange(n))), (cap, k, "base")
        if base[k0, 0] >= 0 and reads[0][:2] == (0, int(base[k0, 0])) and bases[0, 0] == 0 and rows[0, 0] == base[k0, 1]:
            refetched += 1  # the base of the first row lies before the batch: it is read to the front of the buffer
            shared += int((bases[:, 0] == 0).sum() >= 2)
    return refetched, shared


def smallest_span_cap(rec, base):
    return int((rec[:, 1] + np.where(base[:, 0] >= 0, base[:, 1], 0)).max())


def sweep_span_batches(rec, base, read_through):
    """-> (plans, batches with a re-fetched base, such batches with two or more rows that point at it)."""
    low = smallest_span_cap(rec, base)
    k = int(np.flatnonzero(rec[:, 1] + np.where(base[:, 0] >= 0, base[:, 1], 0) == low)[0])
    front = f" and its base of {int(base[k, 1])}" if base[k, 0] >= 0 else ""
    from sai_amd.utils._ingest import span_batches

    plan = span_batches(rec, base, low - 1, read_through, "FILE")
    with pytest.raises(ValueError, match=rf"^SAI_AMD_INGEST_BUFFER of {low - 1} bytes is smaller than one record of FILE \({int(rec[k, 1])} bytes{front}\)$"):
        next(plan)  # before anything is yielded, whichever row it is that does not fit
    wanted = np.unique(np.concatenate([rec[:, 0], base[base[:, 0] >= 0, 0]]))
    whole = int(rec[-1, 0] + rec[-1, 1] - wanted[0])
    plans, before, refetched, shared = [], None, 0, 0
    for cap in range(low, whole + 2):
        batches = span_plan(rec, base, cap, read_through)
        key = S.plan_key(batches)
        assert all(b[4] <= cap for b in batches)
        if key != before:
            r, s = check_span_batches(rec, base, cap, batches)
            refetched, shared = refetched + r, shared + s
            plans.append(batches)
        before = key
    assert len(plans[-1]) == 1
    return plans, refetched, shared


@pytest.mark.parametrize("name", S.REQUESTS)
def test_span_planner_on_the_case_index(name):
    m = S.matrix()
    data, table = pgen_builder.build_pgen(m.codes, m.types)
    assert {t[2] for t in table} == {0, 1, 2, 3, 4, 6, 7}
    rows = S.selection(name)[0]
    rec, base = S.pgen_tables(table, rows)
    ld = np.flatnonzero(base[:, 0] >= 0)
    selected = set(rec[:, 0].tolist())
    runs = [sum(1 for t in table if t[3] == b) for b in sorted({t[3] for t in table if t[3] >= 0})]
    assert sum(1 for r in runs if r >= 3) >= 2  # the file: two runs of three or more difference rows behind one base
    assert any(int(off) not in selected for off in base[ld, 0])  # a base that is itself no selected row
    for read_through in (0, 12, HUGE) if name == "sparse" else (HUGE,):
        plans, refetched, shared = sweep_span_batches(rec, base, read_through)
        firsts, lasts, empty = S.boundaries(plans)
        assert firsts == set(range(len(rec))) and lasts == set(range(len(rec))) and empty == 0
        assert set(ld.tolist()) <= firsts  # every difference row opens a batch: its base is fetched again
        assert refetched >= len(ld) and shared >= 2
        assert max(len(p) for p in plans) >= 3


@pytest.mark.parametrize("seed", range(36))
def test_span_planner_on_seeded_indexes(seed):
    """Records of 1 .. 40 bytes with gaps between them; a difference record's base is the last record before it that is
    none itself, as in a .pgen; any subset selected."""
    rng = np.random.default_rng(1000 + seed)
    n_file = int(rng.integers(2, 17))
    lengths = rng.integers(1, 41, n_file)
    offsets = 100 + np.cumsum(np.concatenate([[0], lengths[:-1] + rng.choice([0, 0, 0, 3, 50], n_file - 1)]))
    is_ld = rng.random(n_file) < 0.5
    is_ld[0] = False
    last_base = np.maximum.accumulate(np.where(~is_ld, np.arange(n_file), -1))
    picked = np.flatnonzero(rng.random(n_file) < 0.7)
    if picked.size == 0:
        picked = np.array([n_file - 1])
    rec = np.stack([offsets[picked], lengths[picked], np.where(is_ld[picked], 2, 0)], axis=1).astype(np.int64)
    b = last_base[picked]
    base = np.where(is_ld[picked, None], np.stack([offsets[b], lengths[b], np.zeros_like(b)], axis=1), -1).astype(np.int64)
    plans, _, _ = sweep_span_batches(rec, base, (0, 3, HUGE)[seed % 3])
    assert len(plans[0]) >= len(plans[-1]) == 1  # which rows can open a batch depends on the lengths: the properties are the test


def test_span_planner_refusals():
    rec = np.array([[10, 4, 0], [20, 4, 2]], dtype=np.int64)
    with pytest.raises(ValueError, match="FILE: a record's base does not lie before it"):
        span_plan(rec, np.array([[-1] * 3, [20, 4, 0]], dtype=np.int64), 64, 0)
    with pytest.raises(ValueError, match="FILE: records overlap"):
        span_plan(rec, np.array([[-1] * 3, [8, 4, 0]], dtype=np.int64), 64, 0)
    with pytest.raises(ValueError, match="FILE: the index is not in file order"):
        span_plan(rec[::-1], np.full((2, 3), -1, dtype=np.int64), 64, 0)
    assert span_plan(rec[:0], rec[:0], 64, 0) == []


# ---- the transposed .geno ----------------------------------------------------------------------------------------


def transposed_index(file_row, lines, n_snp, data_offset=48):
    """An ``eigenstrat._Index`` of a transposed file without a file: what ``batches`` reads of it."""
    from sai_amd.utils import eigenstrat

    idx = eigenstrat._Index.__new__(eigenstrat._Index)
    idx.prefix, idx.geno = "SET", "SET.geno"
    idx.file_row = np.asarray(file_row, dtype=np.int64)
    idx.n_rows, idx.transposed, idx.encoding = len(idx.file_row), True, eigenstrat.TRANSPOSED
    idx.col_of_slot = np.asarray(lines, dtype=np.int32)
    idx.n_slots = len(lines)
    idx.staged_lines, idx.staged_of_slot = np.unique(idx.col_of_slot, return_inverse=True)
    idx.n_cols = len(idx.staged_lines)
    idx.record_bytes, idx.data_offset = max(48, -(-n_snp // 4)), data_offset
    return idx


def check_transposed(idx, cap, batches):
    partition([(b.k0, b.k1) for b in batches], idx.n_rows)
    n_staged = idx.n_cols
    for b in batches:
        assert b.k1 > b.k0 and b.stride % 16 == 0 and b.nbytes == n_staged * b.stride
        assert b.nbytes <= max(cap, 16 * n_staged)  # a staged record is at least one aligned word: the documented minimum
        assert idx.staging_bytes(cap) >= b.nbytes
        s0 = int(idx.file_row[b.k0])
        assert b.first_code == s0 & 3 and b.n_batch == int(idx.file_row[b.k1 - 1]) + 1 - s0
        assert b.first_code + b.n_batch <= 4 * b.stride and len(b.reads) == n_staged
        assert np.array_equal(b.row_in_batch, idx.file_row[b.k0 : b.k1] - s0) and b.row_in_batch.dtype == np.int32
        buf = rebuild(b.reads, b.nbytes)
        for d, line in enumerate(idx.staged_lines):  # the byte that holds variant v of individual d, where the kernel looks for it
            at = d * b.stride + (b.first_code + b.row_in_batch) // 4
            want = file_bytes(idx.data_offset + int(line) * idx.record_bytes + idx.file_row[b.k0 : b.k1] // 4)
            assert np.array_equal(buf[at], want), (cap, b.k0, d)


def sweep_transposed(idx):
    n_staged = idx.n_cols
    sentence = rf"^SAI_AMD_INGEST_BUFFER of {n_staged - 1} bytes is smaller than one byte for each of the {n_staged} requested individuals of SET.geno$"
    with pytest.raises(ValueError, match=sentence):
        next(idx.batches(n_staged - 1))
    plans, before = [], None
    span = int(idx.file_row[-1] - idx.file_row[0]) + 1
    whole = 16 * n_staged * (-(-(span + 3) // 64) + 1)
    for cap in range(n_staged, whole + 2):
        batches = list(idx.batches(cap))
        key = tuple((b.k0, b.k1, b.stride, b.first_code, tuple(b.reads)) for b in batches)
        if key != before:
            check_transposed(idx, cap, batches)
            plans.append(batches)
        before = key
    assert len(plans[-1]) == 1
    return plans


@pytest.mark.parametrize("name", S.REQUESTS)
def test_transposed_planner_on_the_case_index(name):
    n_here = S.N_LONG  # seven batches at the smallest stride: 61 variants each
    m, req = S.matrix(n_here), S.request(name, n_here=n_here)
    plans = sweep_transposed(transposed_index(S.selection(name, n_here)[0], req.cols, m.n))
    starts = {b.first_code for p in plans for b in p}
    assert starts == {0, 1, 2, 3}  # a batch's first variant at each of the four positions in its byte
    assert max(len(p) for p in plans) >= 4 and len(plans) >= 4


@pytest.mark.parametrize("seed", range(24))
def test_transposed_planner_on_seeded_indexes(seed):
    rng = np.random.default_rng(2000 + seed)
    n = int(rng.integers(1, 400))
    rows = np.cumsum(rng.choice([1, 1, 1, 2, 5], size=n)) + int(rng.integers(0, 9))
    lines = rng.integers(0, 12, size=int(rng.integers(1, 9)))
    plans = sweep_transposed(transposed_index(rows, lines, int(rows[-1]) + 1 + int(rng.integers(0, 7)), data_offset=int(rng.integers(0, 99))))
    assert all(b.k1 > b.k0 for p in plans for b in p)
