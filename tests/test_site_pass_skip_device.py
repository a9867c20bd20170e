"""The fused site pass that leaves a wide target's rows unread in tiles where no site passes the ref and source
conditions (site_pass.hip, the SKIP form of ``site_counts_kernel``).

The yardstick is the stand-alone route, ``eng.site_counts`` followed by ``eng.site_flags``: it reads everything and
shares no code with the new loop.  Every comparison is byte for byte and covers the whole of both outputs: the plane
rows (in a buffer filled with ones beforehand: a skipped tile's row must be written), the packed ``tgt_freq`` slots in
a sentinel-filled buffer (nothing beyond a tile's first popcount(any) slots), and ``eng.site_tgt_freq`` of a fresh
buffer (NaN elsewhere).  Each case runs the pass three ways -- as launched by default, with ``SAI_TGT_SKIP=0`` and in the
``candidates_read_all`` mode -- and all three must give the yardstick's bytes.

Shapes: ref 33 individuals, one or three sources of 2, targets of ``kSkipMinTgtInd`` - 1 (the old form), + 0, + 5 (a
partial last 16-row group: a tail of one load) and + 103 (beyond 16 * 4 rows more: a tail batch of full groups and a
partial one); 41 tiles and a partial one.  One more case has more than twice as many tiles as the largest grid of the
family, so that every wave meets skipped and read tiles in turn."""

import dataclasses

import numpy as np
import pytest

import test_grid_stride_cpu as G

pytestmark = pytest.mark.gpu

N_SITES = 41 * 64 + 17
SITE_TILES_PER_CU = 16  # `constexpr int kStreamWavesPerCu = 16;` (common.hpp): the largest grid of the family per CU
SENTINEL = -7.25
W = 0.5  # ref_freq < W passes


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
def min_ind(eng):
    n = int(eng.lib.sai_skip_min_tgt_ind())
    assert n > 200 and n % 16 == 0  # C2's 200-individual target must go on being read everywhere
    return n


def widths(min_ind):
    return [min_ind - 1, min_ind, min_ind + 5, min_ind + 16 * 4 + 39]


def make_mats(n_sites, n_tgt, n_src, passing, seed, missing_tgt=0.02):
    """ref 33 / tgt / n_src sources of 2, diploid.  A site of ``passing`` (bool per site) has ref all 0 and every source
    call 2 (frequency 1); every other site has source dosages 0 or 1 (frequency at most 0.5) and ref dosages 0 or 1."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 2, size=(n_sites, 33)).astype(np.int8)
    ref[passing] = 0
    tgt = np.where(rng.random((n_sites, n_tgt)) < missing_tgt, -1, rng.integers(0, 3, size=(n_sites, n_tgt))).astype(np.int8)
    srcs = []
    for _ in range(n_src):
        s = rng.integers(0, 2, size=(n_sites, 2)).astype(np.int8)
        s[passing] = 2
        srcs.append(s)
    return [ref, tgt, *srcs]


def one_set(n_src, w=W, ops=None):
    from sai_amd import _ffi

    return _ffi.make_params(w, 0.3, 0.9, ops or [("=", 1.0)] * n_src, True)


def packed_slots(cond_any, tf, n_sites):
    """The tgt_freq buffer a candidates pass leaves in a sentinel-filled one: a tile's stored sites packed at its start."""
    n_tiles = -(-n_sites // 64)
    padded = np.zeros(n_tiles * 64, dtype=bool)
    padded[:n_sites] = cond_any
    per_tile = padded.reshape(n_tiles, 64)
    slot = (np.cumsum(per_tile, axis=1) - 1 + np.arange(n_tiles)[:, None] * 64)[per_tile]
    want = np.full(n_sites, SENTINEL)
    want[slot] = tf[cond_any]
    return want


def check(eng, monkeypatch, pops, ploidy, sets, where, want_any_tiles=None):
    """The three routes of the candidates pass against site_counts + site_flags.  -> the per-site OR of the conditions."""
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
    if want_any_tiles is not None:
        assert np.array_equal(np.flatnonzero(want_planes[:, 0]), np.asarray(want_any_tiles)), where
    want_freq = packed_slots(cond_any, tf_np, n_sites)
    want_per_site = np.where(cond_any, tf_np, np.nan)
    for route in ("default", "SAI_TGT_SKIP=0", "candidates_read_all"):
        monkeypatch.delenv("SAI_TGT_SKIP", raising=False)
        if route == "SAI_TGT_SKIP=0":
            monkeypatch.setenv("SAI_TGT_SKIP", "0")
        mode = "candidates_read_all" if route == "candidates_read_all" else "candidates"
        out = (torch.full((n_sites,), SENTINEL, dtype=torch.float64, device=eng.device), torch.full_like(fl, -1))
        eng.site_pass(pops, ploidy, sets, out=out, freq_mode=mode)
        assert np.array_equal(out[1].cpu().numpy().view(np.uint64), want_planes), (where, route)
        assert out[0].cpu().numpy().tobytes() == want_freq.tobytes(), (where, route)
        tf2, fl2 = eng.site_pass(pops, ploidy, sets, freq_mode=mode)  # fresh buffers: zeroed planes, NaN frequencies
        assert np.array_equal(fl2.cpu().numpy().view(np.uint64)[:, : 1 + n], want_planes[:, : 1 + n]), (where, route)
        assert G.same_f64_all(eng.site_tgt_freq(fl2, tf2, n_sites).cpu().numpy(), want_per_site), (where, route)
    monkeypatch.delenv("SAI_TGT_SKIP", raising=False)
    return cond_any


def pattern(name, n_sites):
    """Which sites pass the ref and source conditions -> (bool per site, tiles with a passing site)."""
    n_tiles = -(-n_sites // 64)
    p = np.zeros(n_sites, dtype=bool)
    if name == "none":
        pass
    elif name == "one per tile":
        p[np.minimum(np.arange(n_tiles) * 64 + (np.arange(n_tiles) * 37) % 64, n_sites - 1)] = True
    elif name == "even tiles":
        p[(np.arange(0, n_tiles, 2) * 64 + 5)] = True
    elif name == "site 0":
        p[[3 * 64, 17 * 64]] = True
    elif name == "site 63":
        p[[3 * 64 + 63, 40 * 64 + 63]] = True
    elif name == "last tile":
        p[n_sites - 1] = True
    return p, np.unique(np.flatnonzero(p) // 64)


@pytest.mark.parametrize("n_src", [1, 3])
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_tiles_with_and_without_a_passing_site(eng, monkeypatch, min_ind, which, n_src):
    """(a) no site passes anywhere, (b) one in every tile, (c) only in even tiles, (d) only at site 0 of a tile, only at
    site 63, only in the partial last tile.  The target has no site without a call, so every passing site is a candidate."""
    n_tgt = widths(min_ind)[which]
    pops_of = {}
    for name in ("none", "one per tile", "even tiles", "site 0", "site 63", "last tile"):
        passing, tiles = pattern(name, N_SITES)
        mats = make_mats(N_SITES, n_tgt, n_src, passing, seed=which + 10 * n_src)
        pops_of[name] = eng.tile_many(mats)
        got = check(eng, monkeypatch, pops_of[name], [2] * (2 + n_src), [one_set(n_src)], (name, n_tgt, n_src), want_any_tiles=tiles)
        assert np.array_equal(got, passing), name


def test_spare_lanes_of_the_last_tile_vote_no(eng, monkeypatch, min_ind):
    """(d) passing data only BEYOND n_sites, in the last tile's spare lanes: the blocks are tiled from 42 whole tiles and
    handed over with 41 tiles and 17 sites."""
    n_full = 42 * 64
    passing = np.zeros(n_full, dtype=bool)
    passing[N_SITES:] = True
    pops = [dataclasses.replace(p, n_sites=N_SITES) for p in eng.tile_many(make_mats(n_full, min_ind + 5, 1, passing, seed=3))]
    got = check(eng, monkeypatch, pops, [2, 2, 2], [one_set(1)], "spare lanes", want_any_tiles=[])
    assert not got.any()


def test_missing_calls(eng, monkeypatch, min_ind):
    """(e) a passing site whose target calls are all missing leaves its bit down, the next one, with calls, stores its
    frequency in slot 0 of its tile; (f) missing calls in ref and the sources at passing and other sites -- a source
    without a call has no frequency and the site no bit; a ref with some calls missing still passes."""
    n_tgt = min_ind + 5
    passing = np.zeros(N_SITES, dtype=bool)
    sites = {"tgt all missing": 5 * 64 + 9, "tgt valid": 6 * 64 + 30, "ref some missing": 9 * 64 + 1, "ref all missing": 11 * 64 + 2,
             "src missing": 13 * 64 + 3, "src half missing": 15 * 64 + 4}  # fmt: skip
    passing[list(sites.values())] = True
    mats = make_mats(N_SITES, n_tgt, 3, passing, seed=8)
    ref, tgt, srcs = mats[0], mats[1], mats[2:]
    tgt[sites["tgt all missing"]] = -1
    ref[sites["ref some missing"], ::2] = -1
    ref[sites["ref all missing"]] = -1
    srcs[1][sites["src missing"]] = -1
    srcs[2][sites["src half missing"], 0] = -1
    rng = np.random.default_rng(9)
    other = rng.choice(np.flatnonzero(~passing), size=200, replace=False)  # missing calls at sites that do not pass
    ref[other[:100], 3] = -1
    srcs[0][other[100:], 1] = -2
    got = check(eng, monkeypatch, eng.tile_many(mats), [2] * 5, [one_set(3)], "missing",
                want_any_tiles=sorted(sites[k] // 64 for k in ("tgt valid", "ref some missing", "src half missing")))  # fmt: skip
    assert sorted(np.flatnonzero(got)) == sorted(sites[k] for k in ("tgt valid", "ref some missing", "src half missing"))


@pytest.mark.parametrize("n_sets", [1, 2, 3])
def test_operators_and_thresholds(eng, monkeypatch, min_ind, n_sets):
    """(g) =, >=, < with y in {0, 0.5, 1} over one to three sets and three sources, on dosages with missing calls in every
    population; ref frequencies on both sides of w.  Sparse enough that tiles with and without a candidate both exist."""
    from sai_amd import _ffi

    rng = np.random.default_rng(40 + n_sets)
    ref = rng.integers(0, 2, size=(N_SITES, 33)).astype(np.int8) * (rng.random((N_SITES, 1)) < 0.5)
    ref = np.where(rng.random(ref.shape) < 0.01, -1, ref).astype(np.int8)
    tgt = np.where(rng.random((N_SITES, min_ind)) < 0.02, -1, rng.integers(0, 3, size=(N_SITES, min_ind))).astype(np.int8)
    srcs = [np.where(rng.random((N_SITES, 2)) < 0.05, -1, rng.integers(0, 3, size=(N_SITES, 2))).astype(np.int8) for _ in range(3)]
    pops = eng.tile_many([ref, tgt, *srcs])
    seen_empty = seen_full = 0
    for trial, ops in enumerate([[("=", 1.0), (">=", 0.5), ("<", 0.5)], [("<", 1.0), ("=", 0.0), (">=", 1.0)], [(">=", 0.0), ("=", 0.5), ("=", 1.0)],
                                 [("=", 1.0), ("=", 1.0), ("=", 1.0)], [("<", 0.0), (">=", 0.5), ("=", 0.5)]]):  # fmt: skip
        sets = [_ffi.make_params(w, 0.2, 0.9, ops[s:] + ops[:s], True) for s, w in zip(range(n_sets), (0.2, 0.01, 1.0))]
        got = check(eng, monkeypatch, pops, [2, 2, 2, 1, 2], sets, (n_sets, trial))
        per_tile = np.add.reduceat(got, np.arange(0, N_SITES, 64))
        seen_empty += int((per_tile == 0).sum())
        seen_full += int((per_tile > 0).sum())
    assert seen_empty > 0 and seen_full > 0


def test_calls_that_take_the_old_route(eng, monkeypatch, min_ind):
    """A set without ancestral alleles, a dense call and a call with ``counts=`` read everything as before: the same
    yardstick, and the target's counts right in every tile -- also where no site passes."""
    import torch

    from sai_amd import _ffi

    passing, _ = pattern("even tiles", N_SITES)
    mats = make_mats(N_SITES, min_ind + 5, 1, passing, seed=21)
    pops, ploidy = eng.tile_many(mats), [2, 2, 2]
    want_counts = G.counts_numpy(mats)
    counts = eng.site_counts(pops)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    for sets in ([one_set(1)], [one_set(1), _ffi.make_params(W, 0.3, 0.9, [("=", 1.0)], False)]):
        tf, fl, _ = eng.site_flags(counts, ploidy, sets)
        tf2, fl2 = eng.site_pass(pops, ploidy, sets)  # dense
        assert torch.equal(fl, fl2) and tf.cpu().numpy().tobytes() == tf2.cpu().numpy().tobytes()
        c3 = torch.zeros_like(counts)
        out = (torch.full((N_SITES,), SENTINEL, dtype=torch.float64, device=eng.device), eng.alloc_planes(N_SITES, len(sets)))
        eng.site_pass(pops, ploidy, sets, out=out, counts=c3, freq_mode="candidates")
        assert np.array_equal(c3.cpu().numpy(), want_counts)
        n = len(sets)
        any_word = fl[:, 1]
        for s in range(1, n):
            any_word = any_word | fl[:, 1 + s]
        assert torch.equal(out[1][:, 1:], fl[:, 1:]) and torch.equal(out[1][:, 0], any_word)
        cond_any = ((any_word.cpu().numpy().view(np.uint64)[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)[:N_SITES]
        assert out[0].cpu().numpy().tobytes() == packed_slots(cond_any, tf.cpu().numpy(), N_SITES).tobytes()
        if n == 2:  # the set without ancestral alleles: candidates without counts, inverted words and all
            out = (torch.full((N_SITES,), SENTINEL, dtype=torch.float64, device=eng.device), eng.alloc_planes(N_SITES, n))
            eng.site_pass(pops, ploidy, sets, out=out, freq_mode="candidates")
            assert torch.equal(out[1][:, 1:], fl[:, 1:]) and torch.equal(out[1][:, 0], any_word)
            assert out[0].cpu().numpy().tobytes() == packed_slots(cond_any, tf.cpu().numpy(), N_SITES).tobytes()


def test_every_wave_meets_skipped_and_read_tiles_in_turn(eng, monkeypatch, min_ind):
    """More than twice as many tiles as the grid (16 one-wave blocks per CU for populations this narrow): wave w takes
    tiles w, w + cap, w + 2 cap; a passing site lies in tile w + j cap when w + j is even, so every wave reads a tile
    after one it skipped and skips one after one it read."""
    import torch

    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    cap = SITE_TILES_PER_CU * n_cu
    n_sites = G.site_count(cap)
    n_tiles = -(-n_sites // 64)
    assert n_tiles > 2 * cap
    passing = np.zeros(n_sites, dtype=bool)
    all_tiles = np.arange(n_tiles)
    tiles = all_tiles[(all_tiles % cap + all_tiles // cap) % 2 == 0]
    passing[np.minimum(tiles * 64 + (tiles * 11) % 64, n_sites - 1)] = True
    mats = make_mats(n_sites, min_ind + 5, 1, passing, seed=77)
    got = check(eng, monkeypatch, eng.tile_many(mats), [2, 2, 2], [one_set(1)], "capped grid", want_any_tiles=np.unique(np.flatnonzero(passing) // 64))
    assert np.array_equal(got, passing)
