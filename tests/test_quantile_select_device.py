"""The Q quantile of sai_window_stats on hand-placed doubles (tests/quantile_select_cases.py; test_quantile_select_cases_cpu.py
proves that every case is on the route, at the depth and on the value source it claims): pairs of doubles that share
0 .. 13 leading base-256 digits, more than kWaveCap copies of one number, first-digit bins at kWaveCap and one past
it, ranks at the first, the last and an inner member of a bin, every arm of numpy's lerp between 1-ulp neighbours,
inverted sites handed over as plain v -- each read in the wave form, through the slot list, with the frequencies
in global memory and with the rows in global memory.

tgt_freq and the flag planes are built here as device tensors, no genotypes involved.  Every call goes twice: into
buffers of the test's own (capacities of exactly the need, canaries around everything) and through Engine.window_stats.  The
reference is numpy on the float64 effective values; Q is compared bit for bit, counts and lists exactly."""

import numpy as np
import pytest

import quantile_select_cases as qc
from conftest import same_f64

pytestmark = pytest.mark.gpu

GUARD = 64  # int32 words in front of the U list and behind the Q list
CANARY = -0x21524111  # never a position
TAIL = -77  # filler behind the offsets and the totals
REC_TAIL = 0xA5  # filler behind the records


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


def make_sets(call):
    from sai_amd import _ffi

    # w and y_list belong to the site pass; the windows stage reads x, quantile and whether ancestral alleles exist
    return [_ffi.make_params(0.5, s["x"], s["quantile"], [(">=", 0.0)], s["anc"]) for s in call.sets]


def check_records(rec, want, call, where):
    n_s, n_w = call.n_sets, int(call.lo.size)
    assert rec.shape == (n_s, n_w), where
    for name, exp in (("n_sites", want.n_sites), ("n_cond", want.n_cond), ("u_count", want.u_count), ("n_cdd_q", want.n_cdd_q)):
        got = rec[name].astype(np.int64)
        assert np.array_equal(got, exp), (*where, name, got.tolist(), exp.tolist())
    for s in range(n_s):
        for w in range(n_w):
            got, exp = rec["q"][s, w], want.q[s, w]
            assert same_f64(got, exp), (*where, "q", s, w, call.query[s], float(got).hex(), float(exp).hex())


def run_call(eng, call, where):
    import torch

    from sai_amd.engine import RECORD_DTYPE

    dev = eng.device
    want = qc.statement(call)
    n_s, n_w = call.n_sets, int(call.lo.size)
    n = n_s * n_w
    tgt, planes = torch.as_tensor(call.tgt_freq).to(dev), torch.as_tensor(call.planes).to(dev)
    lo, hi, pos = (torch.as_tensor(a).to(dev) for a in (call.lo, call.hi, call.pos))
    sets = make_sets(call)
    u_flat = np.concatenate([want.u_lists[s][w] for s in range(n_s) for w in range(n_w)]).astype(np.int32)
    q_flat = np.concatenate([want.q_lists[s][w] for s in range(n_s) for w in range(n_w)]).astype(np.int32)
    need_u, need_q = int(u_flat.size), int(q_flat.size)
    cap_u, cap_q = max(need_u, 1), max(need_q, 1)  # a list without entries still gets a word, which must stay as it is
    rec_bytes = n * RECORD_DTYPE.itemsize
    records = torch.full((rec_bytes + 48,), REC_TAIL, dtype=torch.uint8, device=dev)
    offsets = torch.full((2 * n + 8,), TAIL, dtype=torch.int64, device=dev)
    words = int(eng.lib.sai_window_total_words(n_s, n_w))
    totals = torch.full((words + 16,), TAIL, dtype=torch.int64, device=dev)
    lists = torch.full((2 * GUARD + cap_u + cap_q,), CANARY, dtype=torch.int32, device=dev)
    u, q = lists[GUARD : GUARD + cap_u], lists[GUARD + cap_u : GUARD + cap_u + cap_q]
    eng.window_stats_async(tgt, planes, sets, lo, hi, pos, (records[:rec_bytes], offsets[: 2 * n], u, q, totals))
    torch.cuda.synchronize()

    raw = records.cpu().numpy()
    check_records(raw[:rec_bytes].view(RECORD_DTYPE).reshape(n_s, n_w), want, call, (*where, "own buffers"))
    assert (raw[rec_bytes:] == REC_TAIL).all(), (*where, "bytes behind the records")
    off = offsets.cpu().numpy()
    for col, counts in ((0, want.u_count), (1, want.n_cdd_q)):
        c = counts.reshape(-1)
        assert np.array_equal(off[: 2 * n].reshape(n, 2)[:, col], np.cumsum(c) - c), (*where, "offsets", col)
    assert (off[2 * n :] == TAIL).all(), (*where, "words behind the offsets")
    tot = totals.cpu().numpy()
    assert tot[:2].tolist() == [need_u, need_q], (*where, "totals")
    assert (tot[words:] == TAIL).all(), (*where, "words behind the scan scratch")
    got = lists.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[GUARD + cap_u + cap_q :] == CANARY).all(), (*where, "guards around the lists")
    assert np.array_equal(got[GUARD : GUARD + need_u], u_flat) and (got[GUARD + need_u : GUARD + cap_u] == CANARY).all(), (*where, "U lists")
    assert np.array_equal(got[GUARD + cap_u : GUARD + cap_u + need_q], q_flat), (*where, "Q lists")
    assert (got[GUARD + cap_u + need_q : GUARD + cap_u + cap_q] == CANARY).all(), (*where, "Q lists")
    # the inputs are only read
    assert np.array_equal(tgt.cpu().numpy().view(np.uint64), call.tgt_freq.view(np.uint64)) and np.array_equal(planes.cpu().numpy(), call.planes)

    res = eng.window_stats(tgt, planes, sets, lo, hi, pos=pos, cap_hint=max(cap_u, cap_q, 2) // 2)  # one retry on the way
    check_records(res.records, want, call, (*where, "Engine.window_stats"))
    for s in range(n_s):
        for w in range(n_w):
            assert res.u_list(s, w).tolist() == want.u_lists[s][w].tolist(), (*where, "U list", s, w)
            assert res.q_list(s, w).tolist() == want.q_lists[s][w].tolist(), (*where, "Q list", s, w)


CASE_IDS = qc.case_ids()


@pytest.mark.parametrize("name,way", CASE_IDS, ids=[f"{a}-{b}" for a, b in CASE_IDS])
def test_quantile_select(eng, name, way):
    case = qc.case(name, way)
    for i, call in enumerate(case.calls):
        run_call(eng, call, (case.name, f"call {i}"))
