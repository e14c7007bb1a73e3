"""egopose_amd/failsafe.py: the `valuefs` fail-safe for takes run side by side is the sequential evaluator's, exactly. A toy
deterministic `run_pass` stands in for the simulation: a take's value at step t depends on its own earlier re-seats."""
import copy

import numpy as np

from egopose_amd.failsafe import FACTOR, SpeculativeValueFailSafe, below, decisions
from egopose_amd.zfilter import RunningStat

LENS = [7, 40, 13, 22, 31]
SEED = 6           # first-pass guesses wrong for some takes, right for others (asserted below)


def _toy_take(base, stat):
    """One take from (and into) `stat`, as the evaluator's loop runs it: a re-seat lifts the following values, which then decay."""
    values, taken, boost = [], [], 0.0
    for t in range(len(base)):
        v = base[t] + boost
        stat.push(np.array([v]))
        values.append(v)
        hit = t != len(base) - 1 and v < 0.6 * stat.mean[0]
        taken.append(hit)
        boost = boost + 0.7 if hit else boost * 0.8
    return np.array(values), np.array(taken, bool)


def _bases(seed=SEED, lens=LENS):
    rng = np.random.RandomState(seed)
    return [rng.uniform(0.2, 2.0, size=n) for n in lens]


def _run_pass_of(bases, log=None):
    def run_pass(ids, prefixes):
        if log is not None:
            log.append(list(ids))
        return [_toy_take(bases[i], p) for i, p in zip(ids, prefixes)]
    return run_pass


def _sequential(bases, stat):
    return [_toy_take(b, stat) for b in bases]


def test_scheduler_equals_the_sequential_loop():
    bases = _bases()
    log = []
    fs = SpeculativeValueFailSafe()
    res = fs.run(range(5), _run_pass_of(bases, log))
    stat = RunningStat(1)
    want = _sequential(bases, stat)
    assert list(res) == [0, 1, 2, 3, 4]
    for i in range(5):
        np.testing.assert_array_equal(res[i][0], want[i][0])
        np.testing.assert_array_equal(res[i][1], want[i][1])
    assert sum(int(w[1].sum()) for w in want) > 0 and any(not w[1][:-1].all() for w in want)
    assert fs.stat.n == stat.n == sum(LENS) and fs.stat.mean[0] == stat.mean[0] and fs.stat._S[0] == stat._S[0]
    assert 2 <= fs.passes < 5, "the seed must make the first pass's guesses wrong for one take and right for another"
    assert fs.pass_takes == [len(ids) for ids in log] and log[0] == [0, 1, 2, 3, 4]
    assert all(log[p + 1] == log[p][len(log[p]) - len(log[p + 1]):] and len(log[p + 1]) < len(log[p]) for p in range(len(log) - 1))


def _adversarial_take(i, stat):
    """3 steps; the first value sits between 0.6 x the mean that the wrong run of take i - 1 leaves and the one its right run
    leaves, and the values that follow differ by orders of magnitude with the first decision."""
    values, taken, hit = [], [], False
    for t in range(3):
        v = 10.0 ** i if t == 0 else (10.0 ** (i + 2) if (hit or i == 0) else 0.01)
        stat.push(np.array([v]))
        values.append(v)
        d = t != 2 and below(v, stat)
        hit = d if t == 0 else hit
        taken.append(d)
    return np.array(values), np.array(taken, bool)


def test_pass_bound_when_every_first_decision_flips_with_the_prefix():
    n = 6
    fs = SpeculativeValueFailSafe()
    res = fs.run(range(n), lambda ids, pre: [_adversarial_take(i, p) for i, p in zip(ids, pre)])
    assert n - 1 <= fs.passes <= n and fs.pass_takes[0] == n and fs.pass_takes == sorted(fs.pass_takes, reverse=True)
    stat = RunningStat(1)
    for i in range(n):
        v, d = _adversarial_take(i, stat)
        np.testing.assert_array_equal(res[i][0], v)
        np.testing.assert_array_equal(res[i][1], d)


def test_statistic_carries_over_to_the_next_run():
    bases = _bases()
    fs = SpeculativeValueFailSafe()
    r1 = fs.run([0, 1], _run_pass_of(bases))
    n1 = fs.stat.n
    r2 = fs.run([2, 3, 4], _run_pass_of(bases))
    stat = RunningStat(1)
    want = _sequential(bases, stat)
    assert n1 == LENS[0] + LENS[1] and fs.stat.n == sum(LENS) and fs.stat.mean[0] == stat.mean[0]
    for i, r in list(r1.items()) + list(r2.items()):
        np.testing.assert_array_equal(r[0], want[i][0])
        np.testing.assert_array_equal(r[1], want[i][1])
    given = RunningStat(1)
    given.push(np.array([3.0]))
    assert SpeculativeValueFailSafe(given).stat is given


def test_the_end_step_makes_no_decision():
    stat = RunningStat(1)
    for v in (10.0, 10.0, 10.0):
        stat.push(np.array([v]))
    before = copy.deepcopy(stat)
    values = np.array([9.0, 0.1, 9.0, 0.1])
    d, after = decisions(values, 3, stat)
    assert d.tolist() == [False, True, False, False]                 # 0.1 at the end step: pushed, not acted on
    assert decisions(values, None, stat)[0].tolist() == [False, True, False, True]
    assert stat.n == before.n == 3 and stat.mean[0] == before.mean[0]        # the prefix is not modified
    ref = copy.deepcopy(before)
    for v in values:
        ref.push(np.array([v]))
    assert after.n == 7 and after.mean[0] == ref.mean[0] and after._S[0] == ref._S[0]
    assert FACTOR == 0.6 and below(5.9, before) and not below(6.0, before)


def test_degenerate_inputs():
    fs = SpeculativeValueFailSafe()
    assert fs.run([], lambda ids, pre: 1 / 0) == {} and fs.passes == 0 and fs.pass_takes == [] and fs.stat.n == 0
    res = fs.run(["a"], lambda ids, pre: [(np.array([0.5]), np.array([False]))])
    assert fs.passes == 1 and fs.pass_takes == [1] and fs.stat.n == 1 and fs.stat.mean[0] == 0.5
    assert res["a"][0].tolist() == [0.5] and res["a"][1].tolist() == [False]
    d, after = decisions([], -1, fs.stat)
    assert d.shape == (0,) and after.n == 1
