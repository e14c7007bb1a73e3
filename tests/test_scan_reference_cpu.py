"""CPU, no kernel: the references, cases and bounds of scan_fixture.py that test_scan_reference_gpu.py holds K5 (GAE) and K6 (the
running filter) to. The long-double sweep is the oracle's estimate_advantages; the cases reach the tile arithmetic they are named
after; and each bound tells a kernel that gets that arithmetic wrong from a right one by a factor of at least 1 000, on the very
inputs the GPU file runs."""
import numpy as np
import pytest

import scan_fixture as F
from oracle import gae as G

L = np.longdouble


def test_long_double_is_wider_than_float64():
    """The references are only references where long double carries more than float64's 53 bits."""
    assert np.finfo(L).eps <= 2.0 ** -63


# ------------------------------------------------------------------------------------------------ K5: the reference
@pytest.mark.parametrize("gt", list(F.GAMMA_TAU))
@pytest.mark.parametrize("n,mask", [(5, "open1"), (300, "episodes"), (2049, "end@2047"), (4096, "open0")])
def test_sweep_is_estimate_advantages(n, mask, gt):
    gamma, tau = F.GAMMA_TAU[gt]
    r, m, v = F.gae_inputs(n, mask)
    a_ref, r_ref, raw_ref = G.estimate_advantages(r, m, v, gamma, tau)
    ref = F.gae_reference(n, mask, gt, "f64")
    # (the oracle sweeps in float64: it is held to the bound the kernel is held to, and sits far inside)
    assert F.worst(raw_ref.ravel(), ref["adv"], F.gae_bound(ref["adv"], "f64")) <= 1.0 / 16
    assert F.worst(r_ref.ravel(), ref["ret"], F.gae_bound(ref["ret"], "f64")) <= 1.0 / 16
    assert F.worst(a_ref.ravel(), ref["std"], F.standardized_bound(ref, "f64")) <= 1.0 / 16
    a = raw_ref.ravel()
    np.testing.assert_allclose(ref["stats"].astype(float), [n, a.mean(), ((a - a.mean()) ** 2).sum()], rtol=1e-12)


def test_float32_reference_is_the_sweep_on_rounded_inputs():
    n, mask, gt = 2049, "episodes", "0.99x0.95"
    r, m, v = F.gae_inputs(n, mask)
    ref = F.gae_reference(n, mask, gt, "f32")
    adv, ret = F.gae_sweep(r.astype(np.float32), m, v.astype(np.float32), *F.GAMMA_TAU[gt])
    assert np.array_equal(adv, ref["adv"]) and np.array_equal(ret, ref["ret"])
    assert np.array_equal(ref["stored"], ref["adv"].astype(np.float32).astype(L))
    np.testing.assert_array_equal(ref["stats"], F.moments(ref["stored"]))
    # and it is another reference than the float64 one, by far more than the float64 bound
    ref64 = F.gae_reference(n, mask, gt, "f64")
    assert F.worst(ref["adv"], ref64["adv"], F.gae_bound(ref64["adv"], "f64")) > 1000.0


@pytest.mark.parametrize("gt", list(F.GAMMA_TAU))
def test_float64_sweep_sits_far_inside_the_bound(gt):
    """The float64 bound is the project's 1e-11, not a fitted one: a plain float64 sweep -- whose error a kernel that composes
    2 048-sample maps has no reason to exceed -- stays below 1/16 of it at the largest case of each kind."""
    gamma, tau = F.GAMMA_TAU[gt]
    for n, mask in [(F.N_THIRD_ROUND, "open1"), (F.N_THIRD_ROUND, "episodes"), (F.N_INTO_SECOND, "end@%d" % (F.ROUND * F.TILE))]:
        ref = F.gae_reference(n, mask, gt, "f64")
        adv, ret = F.gae_sweep(*F.gae_inputs(n, mask), gamma, tau, dtype=np.float64)
        w = max(F.worst(adv, ref["adv"], F.gae_bound(ref["adv"], "f64")), F.worst(ret, ref["ret"], F.gae_bound(ref["ret"], "f64")))
        print("%s n=%d %s: float64 sweep at %.3g of the bound" % (gt, n, mask, w))
        assert w <= 1.0 / 16


# ------------------------------------------------------------------------------------------------ K5: the cases
def _tile_maps(n, mask, gt):
    """P of every tile: the product of its gamma tau m_i, float64."""
    gamma, tau = F.GAMMA_TAU[gt]
    r, m, v = F.gae_inputs(n, mask)
    nt = (n + F.TILE - 1) // F.TILE
    c = np.ones(nt * F.TILE)
    c[:n] = gamma * tau * m
    return np.prod(c.reshape(nt, F.TILE), axis=1)


def _tiles_looked_at(P, t):
    """How many maps tile t composes before the product of the P's is below 2^-200 or the batch ends."""
    acc, k = 1.0, 0
    for j in range(t + 1, len(P)):
        acc, k = acc * P[j], k + 1
        if abs(acc) < F.P_STOP:
            break
    return k


def test_cases_reach_the_look_to_the_right():
    """What each gamma * tau makes of the open batch of 131 tiles: how far tile 0 looks."""
    n = F.N_THIRD_ROUND
    looked = {gt: _tiles_looked_at(_tile_maps(n, "open1", gt), 0) for gt in F.GAMMA_TAU}
    assert looked == {"1x1": 130, "0.9999x1": 130, "0.99x0.95": 2, "0.95x0.95": 1}
    # the 2^-200 stop as opposed to an exact 0: 0.9405^2048 is 2^-181, a second tile is needed and its product is not 0
    P = _tile_maps(n, "open1", "0.99x0.95")
    assert F.P_STOP < P[1] < 1.0 and 0.0 < P[1] * P[2] < F.P_STOP
    # the sizes: exactly one round for tile 0 (64 tiles: 63 to its right ... the 65th tile starts the second), one sample into it, well into it, a third
    assert [(s + F.TILE - 1) // F.TILE for s in F.BIG_SIZES] == [64, 65, 67, 131]
    assert all(_tiles_looked_at(_tile_maps(s, "open1", "1x1"), 0) == nt - 1 for s, nt in zip(F.BIG_SIZES, (64, 65, 67, 131)))
    # a single end stops the look exactly there: tile 0 of the batch with its end at tile 64's first sample looks at 64 tiles, one whole round
    assert _tiles_looked_at(_tile_maps(F.N_INTO_SECOND, "end@%d" % (F.ROUND * F.TILE), "1x1"), 0) == 64
    assert _tiles_looked_at(_tile_maps(F.N_INTO_SECOND, "end@%d" % F.TILE, "1x1"), 0) == 1
    assert _tiles_looked_at(_tile_maps(F.N_INTO_SECOND, "end@%d" % (F.TILE - 1), "1x1"), 0) == 66       # (an end in tile 0 itself stops nothing)
    # the rollout's episodes end every look after one tile, whatever gamma * tau: the old tests' blind spot
    assert np.all(_tile_maps(F.N_THIRD_ROUND, "episodes", "1x1") == 0.0)


def test_every_listed_case_exists_once():
    assert len(set(F.BIG_CASES)) == len(F.BIG_CASES) == 12 and len(set(F.SMALL_CASES)) == len(F.SMALL_CASES)
    for n, mask in F.BIG_CASES + F.SMALL_CASES:
        assert mask in F.gae_masks(n)
    assert {n for n, _ in F.SMALL_CASES} == set(F.SMALL_SIZES) and {n for n, _ in F.BIG_CASES} == set(F.BIG_SIZES)
    # every kind of mask, and every position of a single end, somewhere behind a tile that hands a carry in
    assert {mk for n, mk in F.BIG_CASES + F.SMALL_CASES if n > F.TILE} == set(F.gae_masks(F.N_THIRD_ROUND))


# ------------------------------------------------------------------------------------------------ K5: the bounds
_MUTANT_CASES = [(F.N_THIRD_ROUND, "open1"), (F.N_THIRD_ROUND, "open0"), (F.N_INTO_SECOND, "end@%d" % (F.ROUND * F.TILE))]
# gamma * tau at which a mutant must show (on the open batch). Stopping after one tile is invisible up to 0.9405, where two tiles
# reach 2^-362; stopping after one round needs gamma * tau = 1 or 0.9999 (0.9999^131072 = 2e-6 of advantages of 5e3)
_MUST_SHOW = {"no_carry": list(F.GAMMA_TAU), "one_tile": ["1x1", "0.9999x1"], "one_round": ["1x1", "0.9999x1"],
              "swapped": list(F.GAMMA_TAU), "v_edge": list(F.GAMMA_TAU), "stale": list(F.GAMMA_TAU)}


def _excess(adv, ret, ref):
    return max(F.worst(adv, ref["adv"], F.gae_bound(ref["adv"], "f64")), F.worst(ret, ref["ret"], F.gae_bound(ref["ret"], "f64")))


@pytest.mark.parametrize("gt", list(F.GAMMA_TAU))
def test_bounds_tell_wrong_kernels_apart(gt):
    """The kernel's arithmetic on tiles, in float64 numpy, passes the GPU file's bound on the GPU file's inputs; each way of getting
    the cross-tile carry wrong misses it by a factor of at least 1 000 wherever it can show at all.

    What cannot be shown this way is the 2^-200 stop itself: what it drops is below 2^-200 of an advantage, far under any bound, so
    a kernel that stops at another small threshold passes too. The stop is shown harmless, not bit-exact."""
    gamma, tau = F.GAMMA_TAU[gt]
    margins = {mu: 0.0 for mu in F.GAE_MUTANTS}
    for n, mask in _MUTANT_CASES:
        r, m, v = F.gae_inputs(n, mask)
        ref = F.gae_reference(n, mask, gt, "f64")
        assert _excess(*F.gae_tiled(r, m, v, gamma, tau), ref) <= 1.0, (n, mask)
        for mu in F.GAE_MUTANTS:
            stale = F.gae_inputs(n, mask, salt=1) if mu == "stale" else None       # (the GPU file's second call of equal n)
            margins[mu] = max(margins[mu], _excess(*F.gae_tiled(r, m, v, gamma, tau, mutant=mu, stale=stale), ref))
    print(gt, {k: "%.3g" % x for k, x in margins.items()})
    for mu, where in _MUST_SHOW.items():
        if gt in where:
            assert margins[mu] >= 1000.0, "%s at gamma tau %s: only %.3g x the bound" % (mu, gt, margins[mu])
    if gt in ("0.99x0.95", "0.95x0.95"):        # (and here a one-tile look is right, or wrong by less than the bound sees: the old tests' gamma * tau)
        assert margins["one_tile"] <= 1.0 and margins["one_round"] <= 1.0


def test_float32_bound_tells_wrong_kernels_apart():
    """The float32 entry point's bound is 2^-24 wide, not 1e-11: the mutants still miss it by 1 000 x at gamma tau = 1 (on the batch
    that ends with m = 0: with every P exactly 1 two maps commute, and the wrong order shows only where the last tile's P = 0)."""
    gt, (n, mask) = "1x1", _MUTANT_CASES[1]
    gamma, tau = F.GAMMA_TAU[gt]
    r, m, v = F.as_dtype(F.gae_inputs(n, mask), "f32")
    ref = F.gae_reference(n, mask, gt, "f32")
    f32 = lambda x: x.astype(np.float32)
    adv, ret = F.gae_tiled(r, m, v, gamma, tau)
    assert max(F.worst(f32(adv), ref["adv"], F.gae_bound(ref["adv"], "f32")), F.worst(f32(ret), ref["ret"], F.gae_bound(ref["ret"], "f32"))) <= 1.0
    for mu in F.GAE_MUTANTS:
        stale = F.as_dtype(F.gae_inputs(n, mask, salt=1), "f32") if mu == "stale" else None
        adv, ret = F.gae_tiled(r, m, v, gamma, tau, mutant=mu, stale=stale)
        w = max(F.worst(f32(adv), ref["adv"], F.gae_bound(ref["adv"], "f32")), F.worst(f32(ret), ref["ret"], F.gae_bound(ref["ret"], "f32")))
        assert w >= 1000.0, "%s: only %.3g x the float32 bound" % (mu, w)


# ------------------------------------------------------------------------------------------------ K6
def test_filter_cases_take_every_merge_route():
    tiles = lambda n: (n + 63) // 64
    assert [tiles(n) for n in F.ZF_ROWS] == [1, 1, 16, 17, 65] and tiles(F.ZF_TWO_LEVEL[0]) == 257
    assert len(F.ZF_CASES) == 7 * 5 + 2
    X0, X, act = F.zf_inputs(1025, 129)
    assert 0.75 < act.mean() < 0.85
    # the clip has work to do, and the columns differ in scale and offset
    s0, s1, y = F.zf_reference(1025, 129, clip=0.0)
    assert (np.abs(y) > F.ZF_CLIP).sum() > 10
    assert X.std(axis=0)[-1] > 3 * X.std(axis=0)[0] and X.mean(axis=0)[-1] - X.mean(axis=0)[0] > 3


@pytest.mark.parametrize("n,dim", [(1, 129), (64, 300), (1024, 129), (1025, 300), (4100, 129), (4100, 63), (16385, 129)])
def test_filter_bounds_tell_wrong_kernels_apart(n, dim):
    """K6's tile structure in float64 numpy meets the GPU file's tolerances; a column block that takes its group counts from the
    wrong group, and a merge that drops a last partial tile, miss them by 1 000 x wherever they can show (more than 128
    columns; a row count that is no multiple of 64)."""
    X0, X, act = F.zf_inputs(n, dim)
    s0, s1, y = F.zf_reference(n, dim)
    assert F.zf_excess(*F.zf_tiled(X, act, s0), s1, y) <= 1.0
    shows = {"wrong_group_count": dim > 128, "skip_last_partial_tile": n % 64 != 0}
    for mu in F.ZF_MUTANTS:
        w = F.zf_excess(*F.zf_tiled(X, act, s0, mutant=mu), s1, y)
        if shows[mu]:
            # (the count may stay right -- the wrong group's count moves only the weights: then mean, S and y must show it)
            assert w >= 1000.0, "%s at n=%d dim=%d: only %.3g x the tolerances" % (mu, n, dim, w)
        else:
            assert w <= 1.0, (mu, w)


def test_filter_wrong_group_count_shows_without_the_count():
    """The state's count is column 0's, which the wrong-group mutant leaves alone: mean, S and y carry the whole margin."""
    X0, X, act = F.zf_inputs(1025, 129)
    s0, s1, y = F.zf_reference(1025, 129)
    st, ym = F.zf_tiled(X, act, s0, mutant="wrong_group_count")
    assert st[0] == s1[0]
    assert np.array_equal(st[1:129], F.zf_tiled(X, act, s0)[0][1:129])                # column block 0 untouched
    assert abs(st[129] - s1[129]) > 1000 * F.ZF_TOL["mean"] * (1 + abs(s1[129]))      # column 128: the first of block 1
