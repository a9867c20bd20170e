"""tests/scan_cases.py says what it claims: its vectorised statement of the windows stage equals the oracle window
by window (missing calls included), every record count gives the scan grid it is listed with, every capacity class
occurs, the writer-side statement of the list buffers follows the contract of windows.hip's header, and the line
cases have the block counts they are named after.  No GPU."""

import numpy as np
import pytest

import scan_cases as sc
from conftest import same_f64
from oracle import sai_oracle as O

NAMES = sc.window_case_names()
LARGE = [n for n in NAMES if sc.window_case(n).records > 100_000]


@pytest.mark.parametrize("name", [sc.SMALL_CLEAN, sc.SMALL_MISSING, "r1_1x1", "r1_4x1", "r1023_11x93"])
def test_statement_equals_the_oracle_window_by_window(name):
    case = sc.window_case(name)
    ref = sc.reference(case)
    mats = [m.astype(np.int64) for m in case.blk.mats]
    r = 0
    for spec in case.specs:
        for lo, hi in zip(case.lo.tolist(), case.hi.tolist()):
            kw = dict(ref_gts=mats[0][lo:hi], tgt_gts=mats[1][lo:hi], src_gts_list=[m[lo:hi] for m in mats[2:]], ref_ploidy=2,
                      tgt_ploidy=2, src_ploidy_list=[2, 2], pos=case.blk.pos[lo:hi], w=spec["w"], y_list=spec["y_list"],
                      anc_allele_available=spec["anc"])  # fmt: skip
            u, q = O.u_stat(x=spec["x"], **kw), O.q_stat(quantile=spec["quantile"], **kw)
            _, _, cond = O.matching_loci(mats[0][lo:hi], mats[1][lo:hi], [m[lo:hi] for m in mats[2:]], spec["w"], spec["y_list"],
                                         list(sc.PLOIDY), spec["anc"])  # fmt: skip
            where = (name, r)
            assert ref.n_sites[r] == hi - lo and ref.n_cond[r] == int(cond.sum()), where
            assert ref.u_count[r] == u["value"] and ref.n_cdd_q[r] == len(q["cdd_pos"]), where
            assert same_f64(ref.q[r], q["value"]), where
            assert ref.list_of(0, r).tolist() == u["cdd_pos"].tolist(), where
            assert ref.list_of(1, r).tolist() == np.asarray(q["cdd_pos"]).astype(np.int64).tolist(), where
            r += 1
    assert r == case.records


def test_the_small_case_with_missing_calls_has_what_it_is_for():
    case = sc.window_case(sc.SMALL_MISSING)
    ref = sc.reference(case)
    assert any((m < 0).any() for m in case.blk.mats) and not case.large
    assert np.isnan(ref.q).any() and (ref.n_cond == 0).any() and (ref.n_cond > 0).any()
    assert any(not s["anc"] for s in case.specs) and case.form == "shared"
    assert sc.window_case(sc.SMALL_CLEAN).form == "wave"


def test_record_counts_and_scan_grids():
    assert sc.scan_block() == 1024 and sc.scan_threads() == 256
    assert set(sc.COUNTS) == set(sc.GRIDS)
    for want in (1, 1023, 1024, 1025, 4096, 4097, 262144, 262145, 263168, 263169):
        assert want in sc.COUNTS
    assert max(sc.COUNTS) > 264_000
    for count, forms in sc.COUNTS.items():
        assert len(forms) == 2
        for (n_sets, n_w), form in zip(forms, ("wave", "shared")):
            case = sc.window_case(f"r{count}_{n_sets}x{n_w}")
            assert case.form == form and (1 <= n_sets <= 3 if form == "wave" else 4 <= n_sets <= sc.MAX_SETS)
            assert case.records == n_sets * n_w == (count if count > 1 or form == "wave" else 4)
            assert case.grid == -(-case.records // 1024) == sc.GRIDS[count], (count, form)
            assert case.lo.min() == 0 and (case.hi.max() == sc.N_SITES or n_w == 1) and np.all(case.hi - case.lo == sc.K)
    # a thread of window_scan_apply adds a second partial from workgroup 257 on: a grid of 258.  263 168 records are
    # 257 full workgroups, the largest count that stays below; three counts lie above
    assert sc.scan_threads() + 2 == sc.SECOND_PARTIAL_GRID
    assert sc.GRIDS[263168] == sc.SECOND_PARTIAL_GRID - 1
    assert sorted(c for c, g in sc.GRIDS.items() if g >= sc.SECOND_PARTIAL_GRID) == [263169, 264020, 265220]
    assert len(NAMES) == len(set(NAMES)) == 2 * len(sc.COUNTS)


@pytest.mark.parametrize("name", LARGE[:2] + LARGE[-4:] + ["r4097_17x241", "r1025_1x1025"])
def test_large_cases_have_condition_sites_everywhere_and_varied_counts(name):
    case = sc.window_case(name)
    ref = sc.reference(case)
    assert case.large and not any((m < 0).any() for m in case.blk.mats)
    assert ref.n_cond.min() >= 1 and not np.isnan(ref.q).any() and ref.n_cdd_q.min() >= 1
    for which in (0, 1):
        c = ref.counts(which)
        assert len(np.unique(c)) >= 4 and np.count_nonzero(np.diff(c)) > c.size // 20, (name, which)
        assert ref.flat(which).size == ref.need(which)
        # sums of whole workgroups differ as well: a partial taken from the wrong workgroup shows
        assert len(np.unique(sc.expected_partials(c))) > 1 or case.grid == 1


def test_set_pool():
    qs = {s["quantile"] for s in sc.POOL}
    assert {0.0, 0.5, 1.0} <= qs and len({s["x"] for s in sc.POOL}) >= 10
    loose = [s for s in sc.POOL if s["w"] == 1.0 and s["y_list"] == list(sc.LOOSE) and s["anc"]]
    assert len(loose) >= 14 and sum(s["w"] < 1.0 for s in sc.POOL) == 4 and sum(not s["anc"] for s in sc.POOL) == 1


def test_every_capacity_class_occurs():
    seen_u, seen_q, zero_behind, exact = set(), set(), 0, 0
    for name in NAMES:
        ref = sc.reference(sc.window_case(name))
        pairs = sc.capacity_pairs(ref)
        if sc.window_case(name).records >= 1023:
            assert len(pairs) == len(sc.PAIRS), name  # every class exists on both sides
        for a, b, cap_u, cap_q in pairs:
            seen_u.add(a)
            seen_q.add(b)
            for which, cls, cap in ((0, a, cap_u), (1, b, cap_q)):
                counts = ref.counts(which)
                off = sc.expected_offsets(counts, cap)
                total = ref.need(which)
                assert cap >= 0
                if cls in ("total", "ample"):
                    assert (off >= 0).all() and cap - total == (0 if cls == "total" else sc.AMPLE_EXTRA)
                    exact += cls == "total" and total > 0
                if cls == "total_minus_1":
                    assert (off < 0).any() and cap == total - 1
                if cls in ("mid", "boundary"):
                    first = int(np.flatnonzero(off < 0)[0])
                    start = int(counts[:first].sum())
                    assert 0 < cap < total and (off >= 0).any()
                    assert (start < cap < start + counts[first]) if cls == "mid" else (start == cap and counts[first] > 0)
                    zero_behind += int(np.any((counts[first:] == 0) & (off[first:] < 0)))
                if cls == "zero":
                    assert np.array_equal(off >= 0, (counts == 0) & (np.cumsum(counts) == 0))
    assert seen_u == seen_q == set(sc.CLASSES)
    assert zero_behind > 0 and exact > 0
    assert ("mid", "ample") in sc.PAIRS and ("ample", "mid") in sc.PAIRS and sc.PAIRS[-1] == ("ample", "ample")


def _contract_writer(ref, cap_u, cap_q, guard):
    """The header of windows.hip taken literally, record by record: offsets, totals and one joined list buffer
    [guard | U | Q | guard] that starts out as canaries."""
    buf = np.full(guard + cap_u + cap_q + guard, sc.CANARY, dtype=np.int32)
    n = ref.u_count.size
    off = np.zeros((n, 2), dtype=np.int64)
    run = [0, 0]
    for r in range(n):
        for which, base, cap in ((0, guard, cap_u), (1, guard + cap_u, cap_q)):
            lst = ref.list_of(which, r)
            if run[which] + len(lst) <= cap:
                off[r, which] = run[which]
                buf[base + run[which] : base + run[which] + len(lst)] = lst
            else:
                off[r, which] = -1
            run[which] += len(lst)
    return off, run, buf


@pytest.mark.parametrize("name", [sc.SMALL_CLEAN, sc.SMALL_MISSING])
def test_expected_buffers_follow_the_contract(name):
    ref = sc.reference(sc.window_case(name))
    pairs = sc.capacity_pairs(ref)
    assert len(pairs) == len(sc.PAIRS)
    for _, _, cap_u, cap_q in pairs:
        off, run, buf = _contract_writer(ref, cap_u, cap_q, 8)
        assert run == [ref.need(0), ref.need(1)]
        assert np.array_equal(off[:, 0], sc.expected_offsets(ref.counts(0), cap_u))
        assert np.array_equal(off[:, 1], sc.expected_offsets(ref.counts(1), cap_q))
        want = np.concatenate([np.full(8, sc.CANARY, np.int32), sc.expected_region(ref.u_flat, ref.counts(0), cap_u),
                               sc.expected_region(ref.q_flat, ref.counts(1), cap_q), np.full(8, sc.CANARY, np.int32)])  # fmt: skip
        assert np.array_equal(buf, want)
    assert sc.CANARY < 0 and sc.CANARY not in ref.u_flat and np.int32(sc.CANARY) == sc.CANARY


def test_expected_partials():
    counts = np.arange(2500, dtype=np.int64) % 7
    got = sc.expected_partials(counts)
    assert got.tolist() == [int(counts[:1024].sum()), int(counts[1024:2048].sum()), int(counts[2048:].sum())]


# ---- line cases ---------------------------------------------------------------------------------------


def test_line_scan_constants_match_the_source():
    text = (sc.CSRC / "lines.hip").read_text()
    consts = sc.parse_constants(text)
    assert consts["kBlockBytes"] == consts["kScanMax"] == sc.LINE_BLOCK
    assert f"part[{sc.LINE_SCAN_THREADS}]" in text and f"(a.n_blocks + {sc.LINE_SCAN_THREADS - 1}) / {sc.LINE_SCAN_THREADS}" in text


@pytest.mark.parametrize("mis", sc.LINE_MIS)
@pytest.mark.parametrize("n_blocks", sc.LINE_BLOCKS)
def test_line_cases_have_the_stated_blocks(n_blocks, mis):
    case = sc.line_case(n_blocks, mis)
    n = len(case.text)
    assert sc.line_blocks(n, mis) == n_blocks and sc.line_blocks(n + 1, mis) == n_blocks + (1 if mis == 0 else 0)
    assert sc.line_blocks(n - 1, mis) == n_blocks - (0 if mis == 0 else 1)
    assert case.text[-1:] != b"\n" and case.starts[-1] < n  # ends inside a line
    per = -(-n_blocks // sc.LINE_SCAN_THREADS)
    assert per == (1 if n_blocks <= 1024 else 2 if n_blocks <= 2048 else 3)
    idle = sum(1 for t in range(sc.LINE_SCAN_THREADS) if t * per > n_blocks)  # threads whose range starts beyond the end
    assert (idle > 0) == (n_blocks in (1025, 1536, 2049, 3001))
    assert case.n_lines == case.text.count(b"\n") and 1500 * n_blocks // 1024 > case.n_lines > 700 * n_blocks // 1024
    per_block = np.bincount((case.starts[1:] - 1 + mis) // sc.LINE_BLOCK, minlength=n_blocks)
    assert per_block.max() >= 2 and (per_block == 0).sum() > n_blocks // 10 and (per_block == 1).sum() > n_blocks // 4


def test_line_words_on_every_kind_of_line():
    case = sc.line_case(1024, 0)
    lines = [case.text[a : b - 1] for a, b in zip(case.starts[:-1], case.starts[1:])]
    kinds = set()
    for line, word in zip(lines, case.words.tolist()):
        cr, fixed = word >> 31, word & 0x7FFFFFFF
        assert cr == line.endswith(b"\r")
        line = line[:-1] if cr else line
        tabs = [k for k, ch in enumerate(line[: sc.LINE_BLOCK]) if ch == 9]  # as test_line_table_kernels states it
        if not line or line.startswith(b"#"):
            want, kind = 1, "empty" if not line else "comment"
        elif len(tabs) >= 9:
            want, kind = tabs[8] + 1, "record"
        elif len(line) <= sc.LINE_BLOCK:
            want, kind = len(line) + 1, "few columns"
        else:
            want, kind = sc.LINE_BLOCK + 1, "out of reach" if line.count(b"\t") >= 9 else "few columns, long"
        assert fixed == want, line[:40]
        kinds.add((kind, bool(cr)))
    assert {k for k, _ in kinds} == {"empty", "comment", "record", "few columns", "out of reach", "few columns, long"}
    assert ("record", True) in kinds and ("record", False) in kinds
    sizes = np.diff(case.starts)
    assert np.median(sizes) > 2048 and sizes.max() <= 6146
    heads = case.heads()
    assert heads.shape == (case.n_lines, sc.HEAD_BYTES)
    for i in (0, 1, 2, len(lines) - 1) + tuple(np.flatnonzero(sizes < sc.HEAD_BYTES)[:6]):
        chunk = case.text[case.starts[i] : min(case.starts[i] + sc.HEAD_BYTES, case.starts[i + 1])]
        assert heads[i].tobytes() == chunk + b"\n" * (sc.HEAD_BYTES - len(chunk))
    assert (sizes < sc.HEAD_BYTES).any()
