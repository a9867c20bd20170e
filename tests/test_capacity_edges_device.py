"""The windows stage and the streaming kernels on inputs built for their internal capacities (tests/capacity_cases.py;
test_capacity_cases_cpu.py shows that every input sits where it says): each limit of windows.hip at its value and
one past it, with windows that start at a tile boundary and mid-tile, in the wave form and the workgroup form; the
packed 16- and 8-bit accumulators of the stream kernels with worst-case rows at the population sizes around the
switch to the form that widens them several times.  Every comparison is exact."""

import numpy as np
import pytest

import capacity_cases as cc
from conftest import same_f64
from test_hip_kernels import _window_pass

pytestmark = pytest.mark.gpu

CASES = cc.window_cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


# ---- window cases -----------------------------------------------------------------------------------

_EXPECTED: dict = {}


def expected(case):
    """[set][window] -> (U, Q) of the oracle on the window's slice; computed once per case, shared by every test."""
    if case.name not in _EXPECTED:
        from oracle import sai_oracle as O

        ref, tgt, *srcs = [m.astype(np.int64) for m in case.mats]
        table = []
        for s in case.specs:
            row = []
            for lo, hi in case.ranges:
                kw = dict(ref_gts=ref[lo:hi], tgt_gts=tgt[lo:hi], src_gts_list=[g[lo:hi] for g in srcs], ref_ploidy=case.ploidy[0],
                          tgt_ploidy=case.ploidy[1], src_ploidy_list=case.ploidy[2:], pos=case.pos[lo:hi], w=s["w"],
                          y_list=s["y_list"], anc_allele_available=s["anc"])  # fmt: skip
                row.append((O.u_stat(x=s["x"], **kw), O.q_stat(quantile=s["quantile"], **kw)))
            table.append(row)
        _EXPECTED[case.name] = table
    return _EXPECTED[case.name]


def make_sets(case, n_sets):
    from sai_amd import _ffi

    return [_ffi.make_params(s["w"], s["x"], s["quantile"], s["y_list"], s["anc"]) for s in case.specs[:n_sets]]


def check_against_oracle(case, res, n_sets, tag):
    want = expected(case)
    assert res.records.shape == (n_sets, len(case.ranges))
    for si in range(n_sets):
        for wi, (lo, hi) in enumerate(case.ranges):
            eu, eq = want[si][wi]
            rec = res.records[si, wi]
            where = (case.name, tag, si, wi)
            assert rec["n_sites"] == hi - lo, where
            assert rec["n_cond"] == case.claims[wi]["n_cond"][si], where
            assert rec["u_count"] == eu["value"], where
            assert rec["n_cdd_q"] == len(eq["cdd_pos"]), where
            assert same_f64(rec["q"], eq["value"]), (*where, rec["q"], eq["value"])
            assert res.u_list(si, wi).tolist() == eu["cdd_pos"].tolist(), where
            assert res.q_list(si, wi).tolist() == np.asarray(eq["cdd_pos"]).astype(np.int64).tolist(), where


def two_kernel_route(eng, case, n_sets):
    starts = np.array([w[0] for w in case.windows], dtype=np.int64)
    ends = np.array([w[1] for w in case.windows], dtype=np.int64)
    res, lo, hi = _window_pass(eng, case.mats, case.ploidy, make_sets(case, n_sets), case.pos, starts, ends)
    assert list(zip(lo.tolist(), hi.tolist())) == [tuple(r) for r in case.ranges]
    return res


def set_counts(case):
    """The numbers of leading sets a case is run with: below kWinWaves one wave per window, from kWinWaves on one
    workgroup per window; all of them last (the call the case's claims about rows and stored frequencies are for)."""
    waves = cc.constants()["kWinWaves"]
    n = len(case.specs)
    if case.name.startswith(("freqcap", "tiles")):
        return [n]  # limits of the workgroup form only
    return sorted({1, waves - 1, waves, n})


FORM_RUNS = [(c.name, n) for c in CASES for n in set_counts(c)]


@pytest.mark.parametrize("name,n_sets", FORM_RUNS, ids=[f"{a}-{b}sets" for a, b in FORM_RUNS])
def test_window_limits_two_kernel_route(eng, name, n_sets):
    """site_counts + site_flags + window_bounds + window_stats: a dense pass (every frequency stored, 64 per tile)."""
    case = BY_NAME[name]
    check_against_oracle(case, two_kernel_route(eng, case, n_sets), n_sets, "two kernels")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_window_limits_resident_scorer(eng, case):
    """The fused pass in candidates mode (stored frequencies = the union of the sets' condition sites, which is what
    makes the count over a window's tiles land on kFreqCap) and the windows stage behind it; word 0 of the planes has
    the popcount the case claims over every window's tiles."""
    import torch

    from sai_amd.resident import ResidentBlock, ResidentScorer

    n_sets = len(case.specs)
    block = ResidentBlock([eng.tile(m) for m in case.mats], case.ploidy, torch.as_tensor(case.pos.astype(np.int32)).to(eng.device))
    scorer = ResidentScorer(eng, block, case.windows, make_sets(case, n_sets), cap_u=1 << 12, cap_q=1 << 12)
    try:
        assert scorer.fused
        scorer.step()
        res = scorer.results(grow=True)
        word0 = np.ascontiguousarray(scorer.flags.cpu().numpy().view(np.uint64)[:, 0])
        per_tile = np.unpackbits(word0.view(np.uint8)).reshape(len(word0), 64).sum(axis=1)
        for (lo, hi), claim in zip(case.ranges, case.claims):
            assert int(per_tile[lo // 64 : -(-hi // 64)].sum()) == claim["stored"], (case.name, lo, hi)
        check_against_oracle(case, res, n_sets, "resident")
    finally:
        scorer.close()


SWITCH = [c for c in CASES if not c.name.startswith(("freqcap", "tiles"))]


@pytest.mark.parametrize("case", SWITCH, ids=[c.name for c in SWITCH])
def test_form_switch_gives_identical_records_and_lists(eng, case):
    """The same data and the same first kWinWaves - 1 sets as a call of their own (one wave per window) and as the
    first sets of a call of kWinWaves (one workgroup per window): identical records and lists."""
    waves = cc.constants()["kWinWaves"]
    few, many = two_kernel_route(eng, case, waves - 1), two_kernel_route(eng, case, waves)
    assert few.records.tobytes() == many.records[: waves - 1].tobytes()
    for si in range(waves - 1):
        for wi in range(len(case.ranges)):
            assert few.u_list(si, wi).tolist() == many.u_list(si, wi).tolist(), (case.name, si, wi)
            assert few.q_list(si, wi).tolist() == many.q_list(si, wi).tolist(), (case.name, si, wi)


# ---- stream cases -----------------------------------------------------------------------------------

SIZES = cc.stream_sizes()
M = 16 * cc.constants()["kChunkIters"]  # the widest population of the form that widens its fields once
# ref, tgt, sources: a call that takes the form for wide populations because of ONE population just past the limit, a
# call whose populations are all at or below it, and a wide population next to one- and two-individual sources
MIXES = {"multi": (M, M + 1, 1), "single": (M, M - 1, 2), "wide and narrow": (2 * M + 1, 16, 1, 2)}
PLOIDY = 127  # a row of 127s is a frequency of exactly 1: the per-site decision has something to decide


def mix_matrices(sizes):
    return [cc.stream_rows(n) if n > 2 else cc.stream_sources(n) for n in sizes]


def reference_counts(mats):
    out = np.empty((len(mats), cc.STREAM_SITES, 2), dtype=np.int64)
    for p, m in enumerate(mats):
        out[p, :, 0], out[p, :, 1] = cc.counts_reference(m)
    return out


def stream_sets(n_sets, n_src):
    from sai_amd import _ffi

    ops = [">=", "=", "<=", ">", "<"]
    return [_ffi.make_params((1.0, 0.6, 0.3)[s % 3], 0.2, 0.9, [(ops[(s + k) % 5], (0.0, 1.0, 0.5)[(s + k) % 3]) for k in range(n_src)],
                             s % 2 == 0) for s in range(n_sets)]  # fmt: skip


@pytest.mark.parametrize("mix", list(MIXES), ids=list(MIXES))
def test_stream_counts_at_the_multi_switch(eng, mix):
    """site_counts, the fused site_pass (below and above the number of sets that takes the predicate table) and
    site_pass_dd (fused and counts only) give the int64 reference's {dosage sum, called} on worst-case rows."""
    import torch

    mats = mix_matrices(MIXES[mix])
    want = reference_counts(mats)
    pops = [eng.tile(m) for m in mats]
    pl = [PLOIDY] * len(pops)
    n_src = len(pops) - 2
    assert np.array_equal(eng.site_counts(pops).cpu().numpy().astype(np.int64), want)
    exact = torch.as_tensor(want.astype(np.int32)).to(eng.device)
    table_from = cc.constants()["kTableFromSets"]
    for n_sets in (1, table_from + 1):
        sets = stream_sets(n_sets, n_src)
        tf, planes, _ = eng.site_flags(exact, pl, sets)
        assert int((planes[:, 1:] != 0).sum()) > 0
        counts = torch.zeros_like(exact)
        tf2, planes2 = eng.site_pass(pops, pl, sets, counts=counts)
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), want), (mix, n_sets)
        assert torch.equal(planes, planes2) and tf.cpu().numpy().tobytes() == tf2.cpu().numpy().tobytes()
        counts.zero_()
        (tf3, planes3), ad = eng.site_pass_dd(pops, pl, sets, 2, n_src, counts=counts)
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), want), (mix, n_sets)
        assert torch.equal(planes, planes3) and tf.cpu().numpy().tobytes() == tf3.cpu().numpy().tobytes()
        check_dd_terms(ad, mats, n_src)
    counts = torch.zeros_like(exact)
    _, ad = eng.site_pass_dd(pops, None, [], 2, n_src, counts=counts)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), want)
    check_dd_terms(ad, mats, n_src)


def check_dd_terms(ad, mats, n_src_pops):
    src = np.concatenate(mats[2 : 2 + n_src_pops], axis=1)
    got = ad.cpu().numpy().astype(np.int64)
    for which in (0, 1):
        assert np.array_equal(got[which], cc.absdiff_reference(mats[which], src)), which


@pytest.mark.parametrize("n_ind", SIZES)
def test_absdiff_fields_at_their_limit(eng, n_ind):
    """site_absdiff (two source individuals per launch, then one) and the terms that ride along site_pass_dd, for 1, 2
    and 3 source individuals: rows whose every |a - b| is 255, at every size around the chunk of rows a 16-bit field
    absorbs.  A chunk is kChunkIters full rows per lane plus at most ONE more (the partial row joins the chunk in
    which the full rows end), so a field holds at most 255 * (kChunkIters + 1); the largest chunk that still fits is
    256 rows (255 * 257 = 2^16 - 1), the next one the loop's step of kUnroll allows, 260, overflows -- and fails this
    test at both sizes of two chunks."""
    import torch

    g = cc.stream_rows(n_ind)
    other = cc.stream_rows(SIZES[(SIZES.index(n_ind) + 3) % len(SIZES)])
    pop, pop2 = eng.tile(g), eng.tile(other)
    for n_src in (1, 2, 3):
        s = cc.stream_sources(n_src)
        src = eng.tile(s)
        want = cc.absdiff_reference(g, s)
        assert want.max() == 255 * n_ind
        assert np.array_equal(eng.site_absdiff(pop, src).cpu().numpy().astype(np.int64), want), n_src
        counts = torch.zeros((3, cc.STREAM_SITES, 2), dtype=torch.int32, device=eng.device)
        _, ad = eng.site_pass_dd([pop, pop2, src], None, [], 2, 1, counts=counts)
        got = ad.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], cc.absdiff_reference(other, s)), n_src
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), reference_counts([g, other, s])), n_src
    sets = stream_sets(2, 1)
    fused, ad = eng.site_pass_dd([pop, pop2, src], [PLOIDY] * 3, sets, 2, 1)
    plain = eng.site_pass([pop, pop2, src], [PLOIDY] * 3, sets)
    assert np.array_equal(ad.cpu().numpy().astype(np.int64)[0], want)
    assert torch.equal(fused[1], plain[1]) and fused[0].cpu().numpy().tobytes() == plain[0].cpu().numpy().tobytes()


@pytest.mark.parametrize("n_ind", SIZES)
def test_packed2_pass_at_the_same_sizes(eng, n_ind):
    """The 2-bit layout's pass on rows of all 2, all missing and 2 / missing alternating: the int64 reference's counts
    and the int8 pass's frequencies and planes."""
    import torch

    mats = [cc.packed_rows(n_ind), cc.packed_rows(SIZES[(SIZES.index(n_ind) + 3) % len(SIZES)]), cc.packed_rows(2)]
    want = reference_counts(mats)
    tiled = [eng.tile(m) for m in mats]
    packed = [eng.pack2(t) for t in tiled]
    pl = [2, 2, 2]
    sets = stream_sets(3, 1)
    c8 = torch.zeros((3, cc.STREAM_SITES, 2), dtype=torch.int32, device=eng.device)
    tf8, planes8 = eng.site_pass(tiled, pl, sets, counts=c8)
    c2 = torch.zeros_like(c8)
    tf2, planes2 = eng.site_pass_packed2(packed, pl, sets, counts=c2)
    assert np.array_equal(c8.cpu().numpy().astype(np.int64), want) and np.array_equal(c2.cpu().numpy().astype(np.int64), want)
    assert torch.equal(planes8, planes2) and tf8.cpu().numpy().tobytes() == tf2.cpu().numpy().tobytes()
    assert int((planes2[:, 1:] != 0).sum()) > 0
    c3 = torch.zeros_like(c8)
    eng.site_pass_packed2(packed, pl, [], counts=c3)
    assert torch.equal(c2, c3)
