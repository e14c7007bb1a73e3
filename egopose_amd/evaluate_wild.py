"""ego_mimic on feature-only takes: videos that have CNN features but no MoCap, hence no expert (ego_pose/ego_mimic_eval_wild.py:85-155).

The takes are the keys of `<data_dir>/features/cnn_feat_<test_feat>.p`, in that order. Per take the video contexts and the state
regressor's predictions are computed once, at batch 1 (`evaluate.regressor_states`); the humanoid is reset to the model's rest
pose one metre up (`HumanoidEnv.reset()` without experts) and seated on `state_pred[0]` aligned to that pose; every tick takes the
mean action, and the `valuefs` rule -- value below 0.6 x the running mean over all values of all takes, in take order -- is the only
fail-safe. There is no `info['end']` break: the loop runs `test_len = len - 2 * fr_margin` ticks and the decision is also taken on
the last one. The reference then indexes `state_pred[t + 1]` with t = test_len - 1, one past the end (an IndexError whenever the rule
fires there); here that one re-seat is clamped away -- no re-seat after the last tick. It cannot change `traj_pred`: the last row was
recorded before the tick. Results: ({'traj_pred', 'vel_pred'}, {'algo': 'ego_mimic'}), saved as iter_%04d_<test_feat>.p.

`WildEvaluator` goes take by take through the single-env facade (and keeps `show_noise`): it IS `Evaluator`'s loop
(`Evaluator._eval_take`, which carries that clamp) with another reset and `HAS_EXPERT = False` -- no expert row, no reward, no `end`.
`BatchedWildEvaluator` puts the takes on
`num_envs` lockstep slots: it IS `BatchedEvaluator`'s pass (fused actor + critic step with the frozen filter, pinned value copy,
exact speculative `valuefs` scheduling) over another kind of take. A take's result does not depend on the slot count.
"""
from __future__ import annotations

import pickle

from .evaluate import BatchedEvaluator, Evaluator


def load_features(cfg, test_feat):
    """{take: [len][cnn_fdim]} of `<data_dir>/features/cnn_feat_<test_feat>.p` (what gen_cnn_feature --out-id writes)."""
    with open("%s/features/cnn_feat_%s.p" % (cfg.data_dir, test_feat), "rb") as f:
        cnn_feat_dict, _ = pickle.load(f)
    return cnn_feat_dict


def cli_takes(cfg, env, data, test_feat):
    """What the evaluation CLIs run on -> (cnn_feat_dict or None, the features' width): the feature-only takes of `--test-feat`
    (ego_mimic_eval_wild.py:36-39, ego_forecast_eval_wild.py:40-43: no experts), or else the experts of `--data`, loaded into `env`."""
    if test_feat is not None:
        cnn_feat_dict = load_features(cfg, test_feat)
        return cnn_feat_dict, next(iter(cnn_feat_dict.values())).shape[-1]
    env.load_experts(cfg.takes[data], cfg.expert_feat_file, cfg.cnn_feat_file)
    return None, env.cnn_feat[0].shape[-1]


def _check_no_experts(env):
    if env.expert_list is not None:
        raise ValueError("the wild evaluators need an env without experts (its reset is the rest pose)")


class WildEvaluator(Evaluator):
    """`Evaluator` over `cnn_feat_dict` = {take: features}; the env has no experts. `trace[take]`: actions, values, resets, state_pred."""

    HAS_EXPERT = False

    def __init__(self, cfg, env, cnn_feat_dict, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                 running_state=None, show_noise=False, logger=None, keep_trace=False):
        _check_no_experts(env)
        super().__init__(cfg, env, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                         running_state=running_state, fail_safe="valuefs", show_noise=show_noise, logger=logger, keep_trace=keep_trace)
        self.cnn_feat_dict = cnn_feat_dict

    def _reset_to_take(self, take):
        test_len = self.cnn_feat_dict[take].shape[0] - 2 * self.cfg.fr_margin
        if test_len < 1:
            raise ValueError("take %s: no frames between the margins" % take)
        self.env.reset()
        return take, self.cnn_feat_dict[take], test_len

    # ------------------------------------------------------------------ ego_mimic_eval_wild.py:94-140 (Evaluator._eval_take)
    def eval_take(self, take):
        traj_pred, _, vel_pred, num_reset = self._eval_take(take)
        return traj_pred, vel_pred, num_reset

    # ------------------------------------------------------------------ ego_mimic_eval_wild.py:147-156
    def run(self, takes=None):
        traj_pred, vel_pred = {}, {}
        self.num_reset = 0
        for take in self.cnn_feat_dict.keys():
            if takes is not None and take not in takes:
                continue
            traj_pred[take], vel_pred[take], n = self.eval_take(take)
            self.num_reset += n
        return {"traj_pred": traj_pred, "vel_pred": vel_pred}, {"algo": "ego_mimic"}


class BatchedWildEvaluator(BatchedEvaluator):
    """`BatchedEvaluator` over `cnn_feat_dict` = {take: features}; the env has no experts. `run()` -> the wild (results, meta);
    `self.num_reset`: the decisions the rule took in the last run (the last tick's included)."""

    DECIDE_ON_END = True

    def __init__(self, cfg, env, cnn_feat_dict, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                 running_state=None, logger=None, keep_trace=False, num_envs=8, device_index=0, n_threads=None):
        _check_no_experts(env)
        super().__init__(cfg, env, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                         running_state=running_state, fail_safe="valuefs", logger=logger, keep_trace=keep_trace, num_envs=num_envs,
                         device_index=device_index, n_threads=n_threads)
        self.takes = list(cnn_feat_dict.keys())
        self.cnn_feat = [cnn_feat_dict[take] for take in self.takes]

    def _take_names(self):
        return self.takes

    def _take_tables(self, i):
        if self.cnn_feat[i].shape[0] - 2 * self.cfg.fr_margin < 1:
            raise ValueError("take %s: no frames between the margins" % self.takes[i])
        return self._feature_tables(self.cnn_feat[i])

    def _seat_ref(self, i):
        qpos = self.env.rest_qpos()            # HumanoidEnv.reset() without experts
        qpos[2] += 1.0
        return qpos

    def _results(self, sel, tables):
        results, meta = super()._results(sel, tables)
        self.num_reset = meta["num_reset"]
        return {"traj_pred": results["traj_pred"], "vel_pred": results["vel_pred"]}, {"algo": "ego_mimic"}
