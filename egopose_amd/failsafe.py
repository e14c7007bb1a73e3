"""The `valuefs` fail-safe of ego_mimic_eval.py for takes that are evaluated side by side, exactly. NumPy only.

The sequential evaluator keeps ONE running statistic of every value estimate it has seen -- across takes, in take order
(`value_stat`, ego_mimic_eval.py:68,152) -- and re-seats the humanoid after a step whose value lies below 0.6 x the running
mean (:167). Take i's decisions therefore depend on all values of the takes before it. But the statistic reaches a take's
trajectory only through the booleans "re-seat after step t": a take run under a GUESSED prefix statistic whose decisions, checked
afterwards against the TRUE prefix, all come out the same IS the run the sequential evaluator would have made, and is final.
`SpeculativeValueFailSafe.run` runs all takes under a guess, accepts the longest consistent prefix of takes, re-runs the rest
with better guesses, and repeats; the first unaccepted take always runs under its true prefix next, so there are at most as
many passes as takes.
"""
from __future__ import annotations

import copy

import numpy as np

from .zfilter import RunningStat

FACTOR = 0.6           # ego_mimic_eval.py:167: value < 0.6 * value_stat.mean


def below(value, stat):
    """The fail-safe's test of one value that has just been pushed into `stat`."""
    return bool(value < FACTOR * stat.mean[0])


def decisions(values, end_step, stat):
    """Replay of the evaluator's loop over one take's `values` from the prefix statistic `stat` (not modified) ->
    (reseat[len(values)] booleans, the statistic afterwards). Every value is pushed (RunningStat.push: the sequential
    evaluator's arithmetic); the step `end_step` -- the one that reports `end`, ego_mimic_eval.py:164-165 -- makes no decision."""
    stat = copy.deepcopy(stat)
    values = np.asarray(values, dtype=float).reshape(-1)
    out = np.zeros(values.shape[0], dtype=bool)
    for t, v in enumerate(values):
        stat.push(np.array([v]))
        if t != end_step:
            out[t] = below(v, stat)
    return out, stat


class SpeculativeValueFailSafe:
    """`stat`: the true running statistic; it persists across `run()` calls as the evaluator's does.
    After a run: `passes`, `pass_takes` (takes per pass)."""

    def __init__(self, stat=None, decide_on_end=False):
        """`decide_on_end`: the step that ends a take takes a decision too (the evaluation of feature-only takes, which has no
        `end` break: ego_mimic_eval_wild.py:113-138)."""
        self.stat = RunningStat(1) if stat is None else stat
        self.decide_on_end = bool(decide_on_end)
        self.passes, self.pass_takes = 0, []

    def run(self, take_ids, run_pass):
        """`run_pass(take_ids, prefixes) -> [(values, taken_decisions)]` runs the given takes, each from a copy of its prefix
        statistic (a RunningStat), to their end: the step that reports `end` is the last value. Deterministic in (take, taken
        decisions). -> {take_id: (values, decisions)} of the accepted runs, in take order."""
        take_ids = list(take_ids)
        n = len(take_ids)
        self.passes, self.pass_takes = 0, []
        latest = [None] * n
        guess = [copy.deepcopy(self.stat) for _ in range(n)]
        done = 0                                   # takes [0, done) are final; self.stat is the true statistic in front of take `done`
        while done < n:
            assert self.passes < n, "a pass must finalise at least one take"
            todo = list(range(done, n))
            res = run_pass([take_ids[i] for i in todo], [copy.deepcopy(guess[i]) for i in todo])
            self.passes += 1
            self.pass_takes.append(len(todo))
            for i, (values, taken) in zip(todo, res):
                latest[i] = (np.asarray(values, dtype=float).reshape(-1), np.asarray(taken, dtype=bool).reshape(-1))
            first = done
            while done < n:
                values, taken = latest[done]
                want, after = decisions(values, -1 if self.decide_on_end else len(values) - 1, self.stat)
                if not np.array_equal(want, taken):
                    break
                self.stat = after
                done += 1
            assert done > first, "the first unaccepted take ran under its true prefix and must be accepted"
            # the first mismatch's true prefix is known now; behind it, the prefix as the latest values would leave it
            g = copy.deepcopy(self.stat)
            for i in range(done, n):
                guess[i] = copy.deepcopy(g)
                for v in latest[i][0]:
                    g.push(np.array([v]))
        return {take_ids[i]: latest[i] for i in range(n)}
