"""The fused site pass that reads a wide ref only until no site of the tile can still pass (site_pass.hip, the probing
form of ``site_counts_kernel``): sources, a vote; the first ``sai_ref_probe_rows()`` ref rows, a vote; the other ref
rows, the skipping form's vote; the target.

The yardstick is the stand-alone route, ``eng.site_counts`` followed by ``eng.site_flags``: it reads everything and
shares no code with the new loop.  Every comparison is byte for byte and covers the whole of both outputs, in pre-filled
buffers, as in test_site_pass_skip_device.py.  Each case runs the pass four ways -- as launched by default, with
``SAI_REF_PROBE=0``, with ``SAI_TGT_SKIP=0`` and in the ``candidates_read_all`` mode -- and all four must give the
yardstick's bytes.

What a tile's wave does is not visible in the outputs, so ``stages`` works it out on the host from the same data -- 0: no
source-matching site (ref and target unread), 1: no such site's partial alt sum is still below w (exit after the
probe), 2: no site passes once ref is whole (target unread), 3: read whole -- and the cases assert that the tiles they
are about are of the stage they mean.

Shapes: 41 tiles and a partial one, a target of ``sai_skip_min_tgt_ind() + 5``, one or three sources of 2, ref widths
(P the probe rows, M the minimum) M - 1 (the old route), M, M + 5, M + 16 * 4 + 39, P and P + 1 (a rest of no row and of
one: the old route too while M > P + 1)."""

import dataclasses
import math

import numpy as np
import pytest

import test_grid_stride_cpu as G
import test_site_pass_skip_device as S

pytestmark = pytest.mark.gpu

N_SITES = 41 * 64 + 17
SITE_TILES_PER_CU = 16  # `constexpr int kStreamWavesPerCu = 16;` (common.hpp): the grid of populations as narrow as the capped-grid case's
# (the probing form's 24 waves per CU replace the 8 of wide populations and long passes only; the loop over the tiles is the same)
SENTINEL = S.SENTINEL
W = 0.1
ROUTES = ("default", "SAI_REF_PROBE=0", "SAI_TGT_SKIP=0", "candidates_read_all")
CMP = {"=": np.equal, "<": np.less, ">": np.greater, "<=": np.less_equal, ">=": np.greater_equal}


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from sai_amd.engine import Engine

    return Engine.get(0)


@pytest.fixture(scope="module")
def consts(eng):
    """(P, M, target width)"""
    p, m = int(eng.lib.sai_ref_probe_rows()), int(eng.lib.sai_ref_probe_min_ind())
    assert p >= 64 and p % 64 == 0 and m >= p and m % 16 == 0
    return p, m, int(eng.lib.sai_skip_min_tgt_ind()) + 5


def widths(consts):
    p, m, _ = consts
    return [m - 1, m, m + 5, m + 16 * 4 + 39, p, p + 1]


def params(specs):
    from sai_amd import _ffi

    return [_ffi.make_params(w, 0.3, 0.9, ops, True) for w, ops in specs]


def one_spec(n_src, w=W):
    return [(w, [("=", 1.0)] * n_src)]


def stages(mats, ploidy, specs, probe_rows, n_sites=None):
    """Per tile: 0 no source-matching site, 1 none whose partial alt sum is still below w, 2 none that passes once ref is
    whole, 3 some site passes the ref and source conditions -- in float64, with the quotients the pass takes."""
    n_sites = len(mats[0]) if n_sites is None else n_sites
    counts = G.counts_numpy(mats)
    with np.errstate(invalid="ignore"):
        f = [G.freq_numpy(counts[p], ploidy[p]) for p in range(len(mats))]
        valid_src = np.all([(f[p] >= 0.0) & (f[p] <= 1.0) for p in range(2, len(mats))], axis=0)
        valid_src[n_sites:] = False  # the last tile's spare lanes
        ref = mats[0][:, :probe_rows]
        bound = np.where(ref >= 0, ref, 0).sum(axis=1, dtype=np.int64).astype(np.float64) / float(mats[0].shape[1] * ploidy[0])
        hits = [valid_src & np.all([CMP[op](f[2 + k], y) for k, (op, y) in enumerate(ops)], axis=0) for _, ops in specs]
        any_hit = np.any(hits, axis=0)
        may_probe = np.any([h & (bound < w) for h, (w, _) in zip(hits, specs)], axis=0)
        may_whole = (f[0] >= 0.0) & (f[0] <= 1.0) & np.any([h & (f[0] < w) for h, (w, _) in zip(hits, specs)], axis=0)
    assert not (may_whole & ~may_probe).any() and not (may_probe & ~any_hit).any()  # the votes only ever narrow
    per_tile = lambda b: np.add.reduceat(b, np.arange(0, len(b), 64)) > 0  # noqa: E731
    return per_tile(any_hit).astype(int) + per_tile(may_probe) + per_tile(may_whole)


def check(eng, monkeypatch, pops, ploidy, sets, where):
    """The four routes of the candidates pass against site_counts + site_flags.  -> the per-site OR of the conditions."""
    import torch

    n_sites, n = pops[0].n_sites, len(sets)
    counts = eng.site_counts(pops)
    tf, fl, _ = eng.site_flags(counts, ploidy, sets)
    fl_np, tf_np = fl.cpu().numpy().view(np.uint64), tf.cpu().numpy()
    assert (fl_np[:, 0] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (fl_np[:, 1 + n :] == 0).all()
    want_planes = np.full_like(fl_np, np.uint64(0xFFFFFFFFFFFFFFFF))  # what neither route writes stays as it was
    want_planes[:, 1 : 1 + n] = fl_np[:, 1 : 1 + n]
    want_planes[:, 0] = np.bitwise_or.reduce(fl_np[:, 1 : 1 + n], axis=1)
    cond_any = ((want_planes[:, 0][:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)
    assert not cond_any[n_sites:].any()
    cond_any = cond_any[:n_sites]
    want_freq = S.packed_slots(cond_any, tf_np, n_sites)
    want_per_site = np.where(cond_any, tf_np, np.nan)
    for route in ROUTES:
        monkeypatch.delenv("SAI_TGT_SKIP", raising=False)
        monkeypatch.delenv("SAI_REF_PROBE", raising=False)
        if "=" in route:
            monkeypatch.setenv(*route.split("="))
        mode = "candidates_read_all" if route == "candidates_read_all" else "candidates"
        out = (torch.full((n_sites,), SENTINEL, dtype=torch.float64, device=eng.device), torch.full_like(fl, -1))
        eng.site_pass(pops, ploidy, sets, out=out, freq_mode=mode)
        assert np.array_equal(out[1].cpu().numpy().view(np.uint64), want_planes), (where, route)
        assert out[0].cpu().numpy().tobytes() == want_freq.tobytes(), (where, route)
        tf2, fl2 = eng.site_pass(pops, ploidy, sets, freq_mode=mode)  # fresh buffers: zeroed planes, NaN frequencies
        assert np.array_equal(fl2.cpu().numpy().view(np.uint64)[:, : 1 + n], want_planes[:, : 1 + n]), (where, route)
        assert G.same_f64_all(eng.site_tgt_freq(fl2, tf2, n_sites).cpu().numpy(), want_per_site), (where, route)
    monkeypatch.delenv("SAI_TGT_SKIP", raising=False)
    monkeypatch.delenv("SAI_REF_PROBE", raising=False)
    return cond_any


def spread(total, rows):
    """``total`` alt calls over ``rows`` rows, as evenly as they go."""
    v = np.full(rows, total // rows, dtype=np.int64) + (np.arange(rows) < total % rows)
    assert rows > 0 and v.max() <= 127
    return v.astype(np.int8)


def make_mats(n_sites, n_ref, n_tgt, n_src, kind, probe_rows, seed, w=W, ploidy_ref=2):
    """ref / tgt / n_src sources of 2.  ``kind`` per site: 0 -- source dosages 0 or 1 (no match with "= 1"), ref dosages
    0 or 1; 1, 2, 3 -- every source call 2 (a match) and ref: 1 a full dosage in every probe row (the bound reaches w
    there), 2 nothing in the probe rows and just enough behind them to reach w, 3 nothing at all (the site passes).  The
    target has calls at every site, so a passing site is a candidate."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 2, size=(n_sites, n_ref)).astype(np.int8)
    ref[kind > 0] = 0
    ref[kind == 1, :probe_rows] = ploidy_ref
    assert probe_rows / n_ref >= w
    if (kind == 2).any():
        ref[kind == 2, probe_rows:] = spread(math.ceil(w * ploidy_ref * n_ref), n_ref - probe_rows)
    tgt = np.where(rng.random((n_sites, n_tgt)) < 0.02, -1, rng.integers(0, 3, size=(n_sites, n_tgt))).astype(np.int8)
    srcs = []
    for _ in range(n_src):
        s = rng.integers(0, 2, size=(n_sites, 2)).astype(np.int8)
        s[kind > 0] = 2
        srcs.append(s)
    return [ref, tgt, *srcs]


def pattern(name, n_sites):
    """Which sites match the sources."""
    n_tiles = -(-n_sites // 64)
    p = np.zeros(n_sites, dtype=bool)
    if name == "one per tile":
        p[np.minimum(np.arange(n_tiles) * 64 + (np.arange(n_tiles) * 37) % 64, n_sites - 1)] = True
    elif name == "even tiles":
        p[(np.arange(0, n_tiles, 2) * 64 + 5)] = True
    elif name == "site 0":
        p[[3 * 64, 17 * 64]] = True
    elif name == "site 63":
        p[[3 * 64 + 63, 40 * 64 + 63]] = True
    elif name == "last tile":
        p[n_sites - 1] = True
    else:
        assert name == "none"
    return p


@pytest.mark.parametrize("n_src", [1, 3])
@pytest.mark.parametrize("which", range(6))
def test_tiles_with_and_without_a_source_match(eng, monkeypatch, consts, which, n_src):
    """No source match anywhere (every row zero, stage 0 everywhere); a match in every tile, in even tiles only, at site
    0, at site 63, in the partial last tile only -- each as a passing site (stage 3) and as one the probe excludes
    (stage 1: the tile's row is zero again)."""
    probe_rows, _, n_tgt = consts
    n_ref = widths(consts)[which]
    for name in ("none", "one per tile", "even tiles", "site 0", "site 63", "last tile"):
        matched = pattern(name, N_SITES)
        tiles = np.unique(np.flatnonzero(matched) // 64)
        for k in (3, 1) if name != "none" else (3,):
            mats = make_mats(N_SITES, n_ref, n_tgt, n_src, matched * k, probe_rows, seed=which + 10 * n_src + 100 * k)
            st = stages(mats, [2] * (2 + n_src), one_spec(n_src), probe_rows)
            assert np.array_equal(np.flatnonzero(st), tiles) and (st[tiles] == k).all(), (name, k)
            got = check(eng, monkeypatch, eng.tile_many(mats), [2] * (2 + n_src), params(one_spec(n_src)), (name, n_ref, n_src, k))
            assert np.array_equal(got, matched & (k == 3)), (name, k)


def test_spare_lanes_of_the_last_tile_vote_no(eng, monkeypatch, consts):
    """Passing data only BEYOND n_sites, in the last tile's spare lanes: the blocks are tiled from 42 whole tiles and
    handed over with 41 tiles and 17 sites."""
    probe_rows, m, n_tgt = consts
    n_full = 42 * 64
    kind = np.zeros(n_full, dtype=int)
    kind[N_SITES:] = 3
    mats = make_mats(n_full, m + 5, n_tgt, 1, kind, probe_rows, seed=3)
    assert not stages(mats, [2, 2, 2], one_spec(1), probe_rows, n_sites=N_SITES).any()
    pops = [dataclasses.replace(p, n_sites=N_SITES) for p in eng.tile_many(mats)]
    assert not check(eng, monkeypatch, pops, [2, 2, 2], params(one_spec(1)), "spare lanes").any()


@pytest.mark.parametrize("ploidy_ref", [2, 1])
@pytest.mark.parametrize("extra", [5, 16 * 4 + 39])
def test_alt_calls_behind_the_probe_rows_and_inside_them(eng, monkeypatch, consts, extra, ploidy_ref):
    """A source match whose ref alt calls lie only in rows >= P, enough of them to reach w: the probe sees zeros, the
    tile goes on (stage 2) and the bit is down.  The mirror: the calls lie in rows < P and the tile exits (stage 1).
    Between them tiles with a passing site (stage 3) and with none (stage 0); diploid and haploid ref."""
    probe_rows, m, n_tgt = consts
    n_ref = max(m, probe_rows) + (extra if ploidy_ref == 2 else 16 * 4 + 39)  # a haploid ref needs the rows for its calls
    kind = np.zeros(N_SITES, dtype=int)
    tiles = np.arange(-(-N_SITES // 64))
    want = tiles % 4
    for t in tiles[want > 0]:
        kind[min(t * 64 + (t * 11) % 64, N_SITES - 1)] = want[t]
    mats = make_mats(N_SITES, n_ref, n_tgt, 1, kind, probe_rows, seed=extra, ploidy_ref=ploidy_ref)
    ploidy = [ploidy_ref, 2, 2]
    assert np.array_equal(stages(mats, ploidy, one_spec(1), probe_rows), want)
    got = check(eng, monkeypatch, eng.tile_many(mats), ploidy, params(one_spec(1)), ("behind / inside", n_ref, ploidy_ref))
    assert np.array_equal(got, kind == 3)


def test_the_boundary(eng, monkeypatch, consts):
    """w = 1/8 and a diploid ref of n: a partial alt sum of n / 4 makes the bound EQUAL to w -- not below it, the tile
    may exit (stage 1); one alt call less and it must go on, and the site passes.  Beside such a site one where 8 missing
    calls in rows >= P shrink the divisor and lift the quotient to w or above: its bit is down; alone in a tile it is
    a tile that goes on and leaves the target unread (stage 2)."""
    probe_rows, m, n_tgt = consts
    n_ref = max(m, probe_rows) + 64
    eq = n_ref // 4
    assert n_ref % 4 == 0 and eq <= 2 * probe_rows - 2 and 4 * (eq - 1) >= n_ref - 8
    w = 0.125
    sites = {"equal": 64 + 5, "one less": 3 * 64 + 6, "one less, beside": 5 * 64 + 7, "lifted, beside": 5 * 64 + 8, "lifted": 7 * 64 + 9}
    kind = np.zeros(N_SITES, dtype=int)
    kind[list(sites.values())] = 3
    mats = make_mats(N_SITES, n_ref, n_tgt, 3, kind, probe_rows, seed=12, w=w)
    ref = mats[0]
    for name, site in sites.items():
        alts = eq if name == "equal" else eq - 1
        ref[site, : alts // 2] = 2
        ref[site, alts // 2] = alts % 2
        if name.startswith("lifted"):
            ref[site, n_ref - 8 :] = -1
    spec = [(w, [("=", 1.0)] * 3)]
    st = stages(mats, [2] * 5, spec, probe_rows)
    assert {int(t): int(s) for t, s in enumerate(st) if s} == {1: 1, 3: 3, 5: 3, 7: 2}
    got = check(eng, monkeypatch, eng.tile_many(mats), [2] * 5, params(spec), "boundary")
    assert sorted(np.flatnonzero(got)) == sorted(sites[k] for k in ("one less", "one less, beside"))


def test_calls_in_the_probe_rows(eng, monkeypatch, consts):
    """Missing calls in the probe rows at passing and other sites, a ref whose probe rows are all missing (with and
    without calls behind them), a ref with no call at all, dosages of 64 and more in the probe rows (the call-by-call
    path) at a source-matching site and at another."""
    probe_rows, m, n_tgt = consts
    n_ref = max(m, probe_rows) + 5
    sites = {"passing, half of the probe missing": 2 * 64 + 1, "excluded, half of the probe missing": 4 * 64 + 2,
             "probe missing, zeros behind": 6 * 64 + 3, "probe missing, calls behind": 8 * 64 + 4, "no call": 10 * 64 + 5,
             "dosage 100": 12 * 64 + 6, "passing, beside a dosage of 64": 14 * 64 + 7, "source missing": 16 * 64 + 8}  # fmt: skip
    kind = np.zeros(N_SITES, dtype=int)
    kind[list(sites.values())] = 3
    kind[sites["excluded, half of the probe missing"]] = 1
    mats = make_mats(N_SITES, n_ref, n_tgt, 3, kind, probe_rows, seed=8)
    ref, srcs = mats[0], mats[2:]
    ref[sites["passing, half of the probe missing"], :probe_rows:2] = -1
    ref[sites["excluded, half of the probe missing"], :probe_rows:2] = -1
    ref[sites["probe missing, zeros behind"], :probe_rows] = -1
    ref[sites["probe missing, calls behind"], :probe_rows] = -1
    ref[sites["probe missing, calls behind"], probe_rows:] = 2
    ref[sites["no call"]] = -1
    ref[sites["dosage 100"], 17] = 100
    ref[sites["passing, beside a dosage of 64"] + 1, 33] = 64  # at a site without a source match, same tile
    srcs[1][sites["source missing"]] = -1
    rng = np.random.default_rng(9)
    other = rng.choice(np.flatnonzero(kind == 0), size=200, replace=False)  # missing calls at sites without a match
    ref[other[:100], 3] = -1
    ref[other[100:], probe_rows + 1] = -2
    srcs[0][other[100:], 1] = -2
    st = stages(mats, [2] * 5, one_spec(3), probe_rows)
    assert {int(t): int(s) for t, s in enumerate(st) if s} == {2: 3, 4: 1, 6: 3, 8: 2, 10: 2, 12: 1, 14: 3}
    got = check(eng, monkeypatch, eng.tile_many(mats), [2] * 5, params(one_spec(3)), "probe rows")
    up = ("passing, half of the probe missing", "probe missing, zeros behind", "passing, beside a dosage of 64")
    assert sorted(np.flatnonzero(got)) == sorted(sites[k] for k in up)


def test_a_tile_exits_only_when_every_hit_set_is_excluded(eng, monkeypatch, consts):
    """Two sets: set 0 (w = 0.01) hits where source 0 has frequency 1, set 1 (w = 0.3) where it has 0.  Site x: only set 0
    hits, bound 0.1 -- excluded, although 0.1 is below the OTHER set's w.  Site y: only set 1 hits.  x alone, and x with a
    y of bound 0.4: the tile exits after the probe.  x with a y of bound 0.1: it goes on and y is set 1's candidate."""
    probe_rows, m, n_tgt = consts
    n_ref = max(m, probe_rows) + 16 * 4 + 39
    spec = [(0.01, [("=", 1.0), (">=", 0.0)]), (0.3, [("=", 0.0), (">=", 0.0)])]
    rng = np.random.default_rng(31)
    ref = rng.integers(0, 2, size=(N_SITES, n_ref)).astype(np.int8)
    tgt = rng.integers(0, 3, size=(N_SITES, n_tgt)).astype(np.int8)
    src0 = np.tile(np.array([[0, 1]], dtype=np.int8), (N_SITES, 1))  # frequency 0.25: neither set
    src1 = rng.integers(0, 3, size=(N_SITES, 2)).astype(np.int8)

    def put(site, src_dosage, bound):
        src0[site] = src_dosage
        ref[site] = 0
        ref[site, :probe_rows] = spread(math.ceil(bound * 2 * n_ref), probe_rows)

    x = [2 * 64 + 3, 4 * 64 + 3, 6 * 64 + 3]
    for site in x:
        put(site, 2, 0.1)
    put(4 * 64 + 40, 0, 0.4)
    put(6 * 64 + 40, 0, 0.1)
    mats = [ref, tgt, src0, src1]
    st = stages(mats, [2] * 4, spec, probe_rows)
    assert {int(t): int(s) for t, s in enumerate(st) if s} == {2: 1, 4: 1, 6: 3}
    got = check(eng, monkeypatch, eng.tile_many(mats), [2] * 4, params(spec), "two sets")
    assert list(np.flatnonzero(got)) == [6 * 64 + 40]


@pytest.mark.parametrize("n_sets", [2, 3])
def test_several_sets(eng, monkeypatch, consts, n_sets):
    """=, >=, < with y in {0, 0.5, 1} over two and three sets of different w and three sources, on dosages with missing
    calls in every population and ref frequencies from 0 to a half: tiles of every stage exist."""
    probe_rows, m, n_tgt = consts
    n_ref = max(m, probe_rows) + 16 * 4 + 39
    rng = np.random.default_rng(40 + n_sets)
    freq = rng.choice([0.0, 0.004, 0.05, 0.5], size=(N_SITES, 1), p=[0.3, 0.2, 0.3, 0.2])
    ref = (rng.random((N_SITES, n_ref)) < freq).astype(np.int8) * rng.integers(1, 3, size=(N_SITES, n_ref)).astype(np.int8)
    ref = np.where(rng.random(ref.shape) < 0.01, -1, ref).astype(np.int8)
    tgt = np.where(rng.random((N_SITES, n_tgt)) < 0.02, -1, rng.integers(0, 3, size=(N_SITES, n_tgt))).astype(np.int8)
    # sources that match rarely: most sites hold a 1 somewhere
    srcs = [np.where(rng.random((N_SITES, 2)) < 0.05, -1, rng.choice([0, 1, 2], size=(N_SITES, 2), p=[0.15, 0.7, 0.15])).astype(np.int8) for _ in range(3)]
    mats, ploidy = [ref, tgt, *srcs], [2, 2, 2, 1, 2]
    pops = eng.tile_many(mats)
    seen = np.zeros(4, dtype=int)
    for trial, ops in enumerate([[("=", 1.0), (">=", 0.5), ("<", 0.5)], [("<", 1.0), ("=", 0.0), (">=", 1.0)], [("=", 0.0), ("=", 0.5), ("=", 1.0)],
                                 [("=", 1.0), ("=", 1.0), ("=", 1.0)], [("<", 0.0), (">=", 0.5), ("=", 0.5)]]):  # fmt: skip
        spec = [(w, ops[s:] + ops[:s]) for s, w in zip(range(n_sets), (0.2, 0.01, 0.06))]
        seen += np.bincount(stages(mats, ploidy, spec, probe_rows), minlength=4)
        check(eng, monkeypatch, pops, ploidy, params(spec), (n_sets, trial))
    assert (seen > 0).all(), seen


def test_every_wave_meets_every_stage_in_turn(eng, monkeypatch, consts):
    """More than four times as many tiles as the largest grid (16 one-wave blocks per CU): wave v takes tiles v, v + cap,
    v + 2 cap, ...; tile v + j cap is of stage (v + j) % 4, so every wave meets a tile that exits at the source vote,
    one that exits after the probe, one that reads ref and leaves the target unread and one read whole, one after the
    other, whichever it starts with."""
    import torch

    probe_rows, m, n_tgt = consts
    n_ref = max(m, probe_rows) + 5
    cap = SITE_TILES_PER_CU * int(torch.cuda.get_device_properties(0).multi_processor_count)
    n_sites = G.site_count(2 * cap)
    tiles = np.arange(-(-n_sites // 64))
    assert len(tiles) > 4 * cap
    want = (tiles % cap + tiles // cap) % 4
    kind = np.zeros(n_sites, dtype=int)
    kind[np.minimum(tiles * 64 + (tiles * 11) % 64, n_sites - 1)[want > 0]] = want[want > 0]
    small = make_mats(64 * 64, n_ref, n_tgt, 1, np.zeros(64 * 64, dtype=int), probe_rows, seed=77)
    mats = [np.tile(x, (-(-n_sites // len(x)), 1))[:n_sites] for x in small]  # sites without a match: one block, repeated
    mats[0][kind > 0] = 0
    mats[0][kind == 1, :probe_rows] = 2
    mats[0][kind == 2, probe_rows:] = spread(math.ceil(W * 2 * n_ref), n_ref - probe_rows)
    mats[2][kind > 0] = 2
    assert np.array_equal(stages([mats[0], mats[1][:, :1], mats[2]], [2, 2, 2], one_spec(1), probe_rows), want)
    got = check(eng, monkeypatch, eng.tile_many(mats), [2, 2, 2], params(one_spec(1)), "capped grid")
    assert np.array_equal(got, kind == 3)


def test_a_call_of_many_sets_taken_set_by_set(eng, monkeypatch, consts):
    """Four sets evaluated set by set (``SAI_NO_PRED_TABLE``): as many as the grid rule calls many, so the call keeps the
    skipping form and its grid -- the same yardstick on data with tiles of every stage."""
    probe_rows, m, n_tgt = consts
    n_ref = max(m, probe_rows) + 5
    tiles = np.arange(-(-N_SITES // 64))
    kind = np.zeros(N_SITES, dtype=int)
    kind[np.minimum(tiles * 64 + (tiles * 11) % 64, N_SITES - 1)[tiles % 4 > 0]] = (tiles % 4)[tiles % 4 > 0]
    mats = make_mats(N_SITES, n_ref, n_tgt, 1, kind, probe_rows, seed=55)
    spec = [(W, [("=", 1.0)]), (0.01, [(">=", 0.5)]), (0.3, [("<", 0.5)]), (W, [("=", 0.0)])]
    monkeypatch.setenv("SAI_NO_PRED_TABLE", "1")
    check(eng, monkeypatch, eng.tile_many(mats), [2, 2, 2], params(spec), "four sets, set by set")
