"""The list bookkeeping of sai_window_stats against its numpy statement (tests/scan_cases.py; test_scan_cases_cpu.py
pins that statement to the oracle): offsets, -1 marks, totals and lists at record counts on both sides of every
step of the two scan kernels (one workgroup, several, more than 256 partial sums), in the wave form and the shared
form, at capacities from 0 (NULL lists) over the exact fit to ample, for U and Q independently.

The test lays the buffers out itself: ONE int32 tensor [guard | U | Q | guard] filled with a canary -- Q directly
behind U, as in the joined layout of Engine.alloc_window_bufs -- and canary words behind the records, the offsets
and the scan's scratch.  Every word the contract does not give to a record that fits must still hold the canary.
All comparisons are exact."""

import ctypes as C

import numpy as np
import pytest

import scan_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 64  # int32 words in front of the U list and behind the Q list
TAIL = -77  # filler behind the offsets and the totals
REC_TAIL = 0xA5  # filler behind the records


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


_BLOCKS: dict = {}


def device_block(eng, blk):
    """(tiled populations, counts, positions) of a block, uploaded once."""
    import torch

    if id(blk) not in _BLOCKS:
        pops = [eng.tile(m) for m in blk.mats]
        _BLOCKS[id(blk)] = (pops, eng.site_counts(pops), torch.as_tensor(blk.pos.astype(np.int32)).to(eng.device))
    return _BLOCKS[id(blk)]


def make_sets(case):
    from sai_amd import _ffi

    return [_ffi.make_params(s["w"], s["x"], s["quantile"], s["y_list"], s["anc"]) for s in case.specs]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {i}: got {got.reshape(-1)[i]}, want {want.reshape(-1)[i]}")


class Run:
    """One case on the device: the per-site arrays (site_flags once) and the test's own output buffers."""

    def __init__(self, eng, case):
        import torch

        from sai_amd.engine import RECORD_DTYPE

        self.eng, self.case, self.ref = eng, case, sc.reference(case)
        _, counts, self.pos = device_block(eng, case.blk)
        self.sets = make_sets(case)
        self.tgt_freq, self.planes, _ = eng.site_flags(counts, list(sc.PLOIDY), self.sets)
        dev = eng.device
        self.lo, self.hi = torch.as_tensor(case.lo).to(dev), torch.as_tensor(case.hi).to(dev)
        n = self.n = case.records
        self.rec_bytes = n * RECORD_DTYPE.itemsize
        self.records = torch.full((self.rec_bytes + 48,), REC_TAIL, dtype=torch.uint8, device=dev)
        self.offsets = torch.full((2 * n + 8,), TAIL, dtype=torch.int64, device=dev)
        self.words = int(eng.lib.sai_window_total_words(case.n_sets, case.n_windows))
        assert self.words == 2 + 2 * case.grid
        self.totals = torch.full((self.words + 16,), TAIL, dtype=torch.int64, device=dev)
        self.need = (self.ref.need(0), self.ref.need(1))
        self.lists = torch.full((2 * GUARD + sum(self.need) + 2 * sc.AMPLE_EXTRA,), sc.CANARY, dtype=torch.int32, device=dev)

    def call(self, cap_u, cap_q, refill=True):
        import torch

        from sai_amd import _ffi

        eng, case = self.eng, self.case
        assert GUARD + cap_u + cap_q + GUARD <= self.lists.numel()
        if refill:
            self.lists.fill_(sc.CANARY)
        u, q = self.lists[GUARD : GUARD + cap_u], self.lists[GUARD + cap_u : GUARD + cap_u + cap_q]
        records, offsets = self.records[: self.rec_bytes], self.offsets[: 2 * self.n]
        if cap_u and cap_q:
            eng.window_stats_async(self.tgt_freq, self.planes, self.sets, self.lo, self.hi, self.pos, (records, offsets, u, q, self.totals))
        else:  # capacity 0: NULL for that list, straight through the C entry
            p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            pl_ptr, pl_stride = eng._planes_arg(self.planes, case.n_sets, int(self.tgt_freq.numel()))
            _ffi.check(
                eng.lib.sai_window_stats(
                    eng.ctx, int(self.tgt_freq.numel()), p(self.tgt_freq), pl_ptr, pl_stride, case.n_sets, eng._params_array(self.sets),
                    case.n_windows, p(self.lo), p(self.hi), p(self.pos), p(records), p(offsets), p(u) if cap_u else None, cap_u,
                    p(q) if cap_q else None, cap_q, p(self.totals), eng._stream(),
                )
            )  # fmt: skip
        torch.cuda.synchronize()

    def check(self, cap_u, cap_q, tag):
        from sai_amd.engine import RECORD_DTYPE

        ref, n, name = self.ref, self.n, self.case.name
        raw = self.records.cpu().numpy()
        rec = raw[: self.rec_bytes].view(RECORD_DTYPE)
        for field, want in (("n_sites", ref.n_sites), ("n_cond", ref.n_cond), ("u_count", ref.u_count), ("n_cdd_q", ref.n_cdd_q)):
            same(rec[field].astype(np.int64), want.astype(np.int64), (name, tag, field))
        got_q = np.ascontiguousarray(rec["q"])
        same(np.isnan(got_q), np.isnan(ref.q), (name, tag, "q is NaN"))
        same(np.where(np.isnan(got_q), 0.0, got_q).view(np.uint64), np.where(np.isnan(ref.q), 0.0, ref.q).view(np.uint64), (name, tag, "q bits"))
        assert (raw[self.rec_bytes :] == REC_TAIL).all(), (name, tag, "bytes behind the records")
        off = self.offsets.cpu().numpy()
        same(off[: 2 * n].reshape(n, 2)[:, 0], sc.expected_offsets(ref.counts(0), cap_u), (name, tag, "U offsets"))
        same(off[: 2 * n].reshape(n, 2)[:, 1], sc.expected_offsets(ref.counts(1), cap_q), (name, tag, "Q offsets"))
        assert (off[2 * n :] == TAIL).all(), (name, tag, "words behind the offsets")
        tot = self.totals.cpu().numpy()
        assert tot[:2].tolist() == list(self.need), (name, tag, "totals", tot[:2].tolist(), self.need)
        assert (tot[self.words :] == TAIL).all(), (name, tag, "words behind the scan scratch")
        lists = self.lists.cpu().numpy()
        want = np.full(lists.size, sc.CANARY, dtype=np.int32)
        want[GUARD : GUARD + cap_u] = sc.expected_region(ref.u_flat, ref.counts(0), cap_u)
        want[GUARD + cap_u : GUARD + cap_u + cap_q] = sc.expected_region(ref.q_flat, ref.counts(1), cap_q)
        same(lists[:GUARD], want[:GUARD], (name, tag, "guard in front of U"))
        same(lists[GUARD : GUARD + cap_u], want[GUARD : GUARD + cap_u], (name, tag, "U region"))
        same(lists[GUARD + cap_u : GUARD + cap_u + cap_q], want[GUARD + cap_u : GUARD + cap_u + cap_q], (name, tag, "Q region"))
        same(lists[GUARD + cap_u + cap_q :], want[GUARD + cap_u + cap_q :], (name, tag, "guard behind Q"))
        # an overflow on one side leaves the other side's lists complete
        if cap_u >= self.need[0]:
            same(lists[GUARD : GUARD + self.need[0]], ref.u_flat, (name, tag, "all U lists"))
        if cap_q >= self.need[1]:
            same(lists[GUARD + cap_u : GUARD + cap_u + self.need[1]], ref.q_flat, (name, tag, "all Q lists"))


NAMES = sc.window_case_names() + [sc.SMALL_CLEAN, sc.SMALL_MISSING]


@pytest.mark.parametrize("name", NAMES)
def test_offsets_totals_and_lists_at_every_capacity(eng, name):
    """Every pair of capacities of the case, one call each into the SAME records, offsets and scratch (only the list
    buffer gets its canaries back): after all the overflows the last call, ample on both sides, gives the full answer."""
    case = sc.window_case(name)
    run = Run(eng, case)
    pairs = sc.capacity_pairs(run.ref)
    assert pairs and pairs[-1][:2] == ("ample", "ample")
    if case.records >= 1023:
        assert len(pairs) == len(sc.PAIRS)
    for a, b, cap_u, cap_q in pairs:
        run.call(cap_u, cap_q)
        run.check(cap_u, cap_q, f"U {a} = {cap_u}, Q {b} = {cap_q}")


@pytest.mark.parametrize("name", ["r263169_3x87723", "r4097_17x241", sc.SMALL_MISSING])
def test_second_call_into_untouched_buffers_after_an_overflow(eng, name):
    """Nothing is put back between the calls, the list buffer included.  The first call overflows U and has NULL for Q,
    so all it leaves are U entries at the places they keep; the second, ample on both sides, must give the full answer
    and leave every other word as it was."""
    case = sc.window_case(name)
    run = Run(eng, case)
    caps = sc.capacity_classes(run.ref.counts(0)), sc.capacity_classes(run.ref.counts(1))
    run.call(caps[0]["mid"], 0)  # Q is NULL: only U entries, at the places they keep
    run.check(caps[0]["mid"], 0, "first call")
    run.call(caps[0]["ample"], caps[1]["ample"], refill=False)
    run.check(caps[0]["ample"], caps[1]["ample"], "second call")


# ---- through the owners of the contract ---------------------------------------------------------------


def check_results(res, case, ref, tag):
    n_s, n_w = case.n_sets, case.n_windows
    assert res.records.shape == (n_s, n_w)
    rec = res.records.reshape(-1)
    for field, want in (("n_sites", ref.n_sites), ("n_cond", ref.n_cond), ("u_count", ref.u_count), ("n_cdd_q", ref.n_cdd_q)):
        same(rec[field].astype(np.int64), want.astype(np.int64), (tag, field))
    got_q = np.ascontiguousarray(rec["q"])
    same(np.isnan(got_q), np.isnan(ref.q), (tag, "q is NaN"))
    same(got_q[~np.isnan(got_q)].view(np.uint64), ref.q[~np.isnan(ref.q)].view(np.uint64), (tag, "q bits"))
    for s in range(n_s):
        for w in range(n_w):
            r = s * n_w + w
            assert res.u_list(s, w).tolist() == ref.list_of(0, r).tolist(), (tag, "U list", s, w)
            assert res.q_list(s, w).tolist() == ref.list_of(1, r).tolist(), (tag, "Q list", s, w)
    assert res.cdd_u.size == ref.need(0) and res.cdd_q.size == ref.need(1), tag


def small_scorer(eng, case, cap_u, cap_q, fetch_lists):
    from sai_amd.resident import ResidentBlock, ResidentScorer

    pops, _, pos = device_block(eng, case.blk)
    windows = [(int(case.blk.pos[lo]), int(case.blk.pos[hi - 1])) for lo, hi in zip(case.lo.tolist(), case.hi.tolist())]
    return ResidentScorer(eng, ResidentBlock(pops, list(sc.PLOIDY), pos), windows, make_sets(case), cap_u=cap_u, cap_q=cap_q,
                          fetch_lists=fetch_lists)  # fmt: skip


@pytest.mark.parametrize("layout", ["separate", "joined"])
def test_resident_scorer_one_entry_short_and_exact(eng, layout):
    """ResidentScorer one entry short on both lists: results() and row_layout() raise and name the need,
    results(grow=True) gives the reference's lists; built at exactly the need it does not grow.  fetch_lists below the
    capacity keeps the lists in allocations of their own, at least the capacity puts Q directly behind U."""
    case = sc.window_case(sc.SMALL_MISSING)
    ref = sc.reference(case)
    need_u, need_q = ref.need(0), ref.need(1)
    assert min(need_u, need_q) > 16
    fetch = 8 if layout == "separate" else max(need_u, need_q)
    scorer = small_scorer(eng, case, need_u - 1, need_q - 1, fetch)
    try:
        assert scorer.chunks[0].joined == (layout == "joined")
        scorer.step()
        with pytest.raises(RuntimeError, match=f"need {need_u}/{need_q}"):
            scorer.results()
        with pytest.raises(RuntimeError, match=f"need {need_u}/{need_q}"):
            scorer.row_layout()
        # the first pass kept its word: the last U and the last Q record that has entries are marked, nothing else
        off = scorer.host_offsets.numpy().reshape(-1, 2)
        same(off[:, 0], sc.expected_offsets(ref.counts(0), need_u - 1), "U offsets one short")
        same(off[:, 1], sc.expected_offsets(ref.counts(1), need_q - 1), "Q offsets one short")
        check_results(scorer.results(grow=True), case, ref, f"grown, {layout}")
        assert (scorer.cap_u, scorer.cap_q) == (need_u, need_q)
        assert scorer.chunks[0].joined == (layout == "joined")
        scorer.row_layout()
    finally:
        scorer.close()
    scorer = small_scorer(eng, case, need_u, need_q, fetch)
    try:
        chunk = scorer.chunks[0]
        scorer.step()
        check_results(scorer.results(), case, ref, f"exact, {layout}")
        assert (scorer.cap_u, scorer.cap_q) == (need_u, need_q) and scorer.chunks[0] is chunk
        check_results(scorer.results(grow=True), case, ref, f"exact, grow allowed, {layout}")
        assert (scorer.cap_u, scorer.cap_q) == (need_u, need_q) and scorer.chunks[0] is chunk
    finally:
        scorer.close()


def test_engine_window_stats_retries_from_a_hint_of_one(eng):
    import torch

    case = sc.window_case(sc.SMALL_MISSING)
    ref = sc.reference(case)
    _, counts, pos = device_block(eng, case.blk)
    sets = make_sets(case)
    tgt_freq, planes, _ = eng.site_flags(counts, list(sc.PLOIDY), sets)
    lo, hi = torch.as_tensor(case.lo).to(eng.device), torch.as_tensor(case.hi).to(eng.device)
    check_results(eng.window_stats(tgt_freq, planes, sets, lo, hi, pos=pos, cap_hint=1), case, ref, "cap_hint = 1")
