"""Evaluation driver of the ego_mimic policy: one env, deterministic policy, state-regressor resets.

Mirrors /root/reference/ego_pose/ego_mimic_eval.py:93-197 (reset_env_state, eval_expert and the per-take loop that
writes `(results, meta)`), on top of the single-env facade of `HumanoidEnv` (batch of one through the same engine and
kernels as training) and the host-side metrics of `egopose_amd.metrics` (ego_pose/eval_pose.py:31-69).

Per take: roll the policy over the whole clip (`fix_len = len - 2*fr_margin`) with the mean action; whenever the
fail-safe fires -- 'valuefs': the value estimate drops below 0.6 x its running mean, 'naivefs': the env reports a
fall -- re-seat the humanoid on the state regressor's prediction for the next frame, aligned to where the
character stands (utils/tools.py:71-75). Rendering (`env_vis`, `--render`) is out of scope.

`BatchedEvaluator` is the same evaluation with the takes side by side: every take is a slot of `env.batched(N)`, all slots advance
in lockstep, in passes of N takes in take order, and a tick is

    record qpos / qvel -> [observation -> frozen filter -> policy MLP -> mean action | value MLP -> value] -> env-step
    -> host: fail-safe decision per slot -> re-seat the flagged slots on their take's state_pred[t + 1]

with the bracket one launch (`FusedActorCritic.with_filter`, egp_policy_step_f32 (vlayers)) and the values' copy to pinned memory
queued behind it. The pass itself -- the batched env, the frozen filter's device state, seating and re-seating slots, the records and
their copy-out, a tick's event / env-step / timed wait -- is `lockstep_eval.LockstepPass`, shared with the forecast evaluation; the
launch, the value copy and the host decision are here. The video contexts and the state regressor's predictions of a take are
computed once per take, at batch 1 as above (a take's result does not depend on the slot count). 'valuefs' compares against a running mean over ALL values in take
order; `egopose_amd.failsafe` makes that exact for takes that run side by side (speculative runs, checked against the true
statistic afterwards, re-run where a decision differs). The reward (which nothing reads) is not evaluated; `show_noise` stays
with `Evaluator`, and so does `causal` as the reference wrote it (a full sweep over the prefix at every tick).

`BatchedOnlineEvaluator` is the online (`--causal`) evaluation on the same slots: `BatchedEvaluator` with another policy-context table.
The reference re-initialises the POLICY's video net at every tick on the frames seen so far (ego_mimic_eval.py:143-145), so row t of
the table is row t + m of that net over frames [0, t + 2m] -- `VideoStateNet.online_contexts`, T + m forward steps and one launch of T
windows of m + 1 steps per take instead of a sweep per tick. The value net and the state regressor keep their whole-take tables, as
in the reference. `Evaluator(causal=True)`, prefix by prefix, is the yardstick it is tested against.

Takes that have video features only (no MoCap, no expert): `egopose_amd.evaluate_wild` (`--test-feat NAME`), on the same pass and,
take by take, on the same loop (`Evaluator._eval_take`). `regressor_states` is the state regressor's prediction of a take for both.
"""
from __future__ import annotations

import copy
import pickle

import numpy as np
import torch

from . import metrics
from .lockstep_eval import LockstepPass, Timing, check_frozen_filter
from .reward import reward_func
from .zfilter import RunningStat


def regressor_states(state_net, mean, std, cnn_feat, fr_margin):
    """The state regressor's de-normalised prediction for the frames of a take between the margins, at batch 1
    (ego_mimic_eval.py:121-122) -> float64 [len - 2 * fr_margin][state]."""
    m, sp = fr_margin, next(state_net.parameters())
    state_pred = state_net(cnn_feat.to(device=sp.device, dtype=sp.dtype).unsqueeze(1))[m:-m].double().cpu().numpy()
    return state_pred * std[None, :] + mean[None, :]


class _MimicEvaluator:
    """What `Evaluator` and `BatchedEvaluator` share: the nets in test mode, the fail-safe's name, the trace, the pickle."""

    def __init__(self, cfg, env, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                 running_state, fail_safe, causal, show_noise, sync, logger, keep_trace):
        if fail_safe not in ("valuefs", "naivefs", "none"):
            raise ValueError("fail_safe must be 'valuefs', 'naivefs' or 'none'")
        self.cfg, self.env = cfg, env
        self.policy_net, self.policy_vs_net = policy_net, policy_vs_net
        self.value_net, self.value_vs_net = value_net, value_vs_net
        self.state_net = state_net
        self.state_net_mean, self.state_net_std = np.asarray(state_net_mean, float), np.asarray(state_net_std, float)
        self.running_state = running_state
        self.fail_safe, self.causal, self.show_noise, self.sync = fail_safe, causal, show_noise, sync
        self.logger = logger
        self.trace = {} if keep_trace else None      # per take: actions, values, reset frames, regressor states
        for net in (policy_net, policy_vs_net, value_net, value_vs_net, state_net):
            net.eval()
        for net in (policy_vs_net, value_vs_net):
            net.set_mode("test")

    def save(self, results, meta, it, data="test"):
        fs_tag = "" if self.fail_safe == "valuefs" else "_" + self.fail_safe
        c_tag = "_causal" if self.causal else ""
        return metrics.save_results("%s/iter_%04d_%s%s%s.p" % (self.cfg.result_dir, it, data, fs_tag, c_tag), results, meta)


class Evaluator(_MimicEvaluator):

    def __init__(self, cfg, env, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                 running_state=None, fail_safe="valuefs", causal=False, show_noise=False, sync=False, logger=None,
                 keep_trace=False):
        super().__init__(cfg, env, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                         running_state, fail_safe, causal, show_noise, sync, logger, keep_trace)
        self.value_stat = RunningStat(1)
        p = next(policy_net.parameters())
        self.device, self.dtype = p.device, p.dtype

    # ------------------------------------------------------------------ ego_mimic_eval.py:93-100
    def reset_env_state(self, state, ref_qpos):
        env = self.env
        qpos = np.array(ref_qpos, float, copy=True)
        qpos[2:] = state[:qpos.size - 2]
        qvel = np.array(state[qpos.size - 2:], float, copy=True)
        metrics.align_human_state(qpos, qvel, ref_qpos)
        env.set_state(qpos, qvel)
        return env.get_obs()

    def _filter(self, state):
        return self.running_state(state, update=False) if self.running_state is not None else state

    # What a subclass over feature-only takes changes (evaluate_wild.WildEvaluator): how the env is reset to a take, and whether the
    # take has an expert -- its row per tick, the reward, and the `info['end']` that ends the take before a decision.
    HAS_EXPERT = True

    def _reset_to_take(self, expert_ind):
        """Reset the env to the take -> (its name, its features, its frames between the margins)."""
        env, m = self.env, self.cfg.fr_margin
        test_len = env.cnn_feat[expert_ind].shape[0] - 2 * m
        env.set_fix_sampling(expert_ind, m, test_len)
        env.reset()
        return env.expert_list[expert_ind], env.get_episode_cnn_feat(), test_len

    # ------------------------------------------------------------------ ego_mimic_eval.py:103-175, ego_mimic_eval_wild.py:94-140
    @torch.no_grad()
    def _eval_take(self, key):
        """-> (traj_pred, traj_orig or None, vel_pred, num_reset) of one take."""
        env, cfg = self.env, self.cfg
        m = cfg.fr_margin
        take, cnn_feat, test_len = self._reset_to_take(key)
        traj_pred, traj_orig, vel_pred = [], [], []
        num_reset, reward_episode = 0, 0.0

        cnn_feat = torch.as_tensor(cnn_feat, dtype=self.dtype, device=self.device)
        self.policy_vs_net.initialize(cnn_feat)
        self.value_vs_net.initialize(cnn_feat)
        state_pred = regressor_states(self.state_net, self.state_net_mean, self.state_net_std, cnn_feat, m)

        state = self._filter(self.reset_env_state(state_pred[0], env.data.qpos))
        tr = None
        if self.trace is not None:
            tr = self.trace[take] = dict(actions=[], values=[], resets=[], state_pred=state_pred)
        for t in range(test_len):
            data = env.data
            traj_pred.append(data.qpos.copy())
            vel_pred.append(data.qvel.copy())
            if self.HAS_EXPERT:
                traj_orig.append(env.get_expert_attr("qpos", env.get_expert_index(t)).copy())
            if self.causal:
                self.policy_vs_net.initialize(cnn_feat[:t + 2 * m + 1])
                self.policy_vs_net.t = t
            state_var = torch.as_tensor(state, dtype=self.dtype, device=self.device).unsqueeze(0)
            policy_in = self.policy_vs_net(state_var)
            value = float(self.value_net(self.value_vs_net(state_var)).item())
            self.value_stat.push(np.array([value]))
            action = self.policy_net.select_action(policy_in, mean_action=not self.show_noise)[0].double().cpu().numpy()
            if tr is not None:
                tr["actions"].append(action.copy())
                tr["values"].append(value)
            next_state, _, done, info = env.step(action)
            next_state = self._filter(next_state)
            if self.HAS_EXPERT:
                reward, _ = reward_func[cfg.reward_id](env, state, action, info)
                reward_episode += reward
                if info["end"]:
                    break
            if (self.fail_safe == "valuefs" and value < 0.6 * self.value_stat.mean[0]) or (self.fail_safe == "naivefs" and info["fail"]):
                if self.logger is not None:
                    self.logger.info("reset state!")
                num_reset += 1
                if tr is not None:
                    tr["resets"].append(t)
                # A decision on the last tick has no next frame to re-seat on. With an expert `end` has ended the take before it; without
                # one the reference reads state_pred[test_len] there, an IndexError. It cannot change traj_pred: the last row is recorded.
                if t + 1 < test_len:
                    state = self._filter(self.reset_env_state(state_pred[t + 1], env.data.qpos))
            else:
                state = next_state
        if self.HAS_EXPERT:
            self.last_reward = reward_episode
        return np.vstack(traj_pred), np.vstack(traj_orig) if traj_orig else None, np.vstack(vel_pred), num_reset

    def eval_expert(self, expert_ind):
        return self._eval_take(expert_ind)

    # ------------------------------------------------------------------ ego_mimic_eval.py:183-197
    def run(self, takes=None):
        """Evaluate every take of the env's expert list -> (results, meta) in the reference's pickle layout."""
        traj_pred, traj_orig, vel_pred, num_reset = {}, {}, {}, 0
        for i, take in enumerate(self.env.expert_list):
            if takes is not None and take not in takes:
                continue
            traj_pred[take], traj_orig[take], vel_pred[take], n = self.eval_expert(i)
            num_reset += n
        results = {"traj_pred": traj_pred, "traj_orig": traj_orig, "vel_pred": vel_pred}
        meta = {"algo": "ego_mimic", "num_reset": num_reset}
        return results, meta


class BatchedEvaluator(_MimicEvaluator):
    """`Evaluator` with the takes on `num_envs` lockstep slots (module docstring). `run()` -> the same (results, meta), `save()`
    the same pickle. `keep_trace`: `self.trace[take]` = dict(actions [T][nu], values [T], resets, state_pred, states [T][obs]) of
    the accepted run. `self.timing`: wall seconds of the last run, split into the wait for the host physics and the rest, and the
    fail-safe scheduler's passes."""

    def __init__(self, cfg, env, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                 running_state=None, fail_safe="valuefs", causal=False, show_noise=False, sync=False, logger=None,
                 keep_trace=False, num_envs=8, device_index=0, n_threads=None):
        from . import policy_step
        from .failsafe import SpeculativeValueFailSafe
        if causal or show_noise:
            raise NotImplementedError("causal / show_noise evaluation runs take by take: use Evaluator")
        check_frozen_filter(running_state, ": use Evaluator")
        if not (policy_step.supported(policy_net) and policy_step.supported_value(value_net)):
            raise NotImplementedError("the batched evaluation needs the HIP actor + critic step (float32 PolicyGaussian and Value "
                                      "over plain MLPs): use Evaluator")
        super().__init__(cfg, env, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                         running_state, fail_safe, False, False, sync, logger, keep_trace)
        self.num_envs, self.device_index, self.n_threads = int(num_envs), int(device_index), n_threads
        self._fs = SpeculativeValueFailSafe(decide_on_end=self.DECIDE_ON_END)
        self.timing = {}

    value_stat = property(lambda self: self._fs.stat)      # the running statistic of every accepted value, across run() calls

    # What a subclass over another kind of take changes (evaluate_wild.BatchedWildEvaluator): whether the tick that ends a take still
    # takes the fail-safe decision (it never re-seats), the takes' names, a take's tables, the pose its first seat is aligned to, and
    # how the records become results.
    DECIDE_ON_END = False

    def _take_names(self):
        return self.env.expert_list

    def _seat_ref(self, i):
        return self.env.expert_arr[i]["qpos"][self.cfg.fr_margin]

    # ------------------------------------------------------------------ per take, once: contexts and regressor states (batch 1)
    @torch.no_grad()
    def _feature_tables(self, cnn_feat_np):
        """Contexts of both video nets and the de-normalised regressor states of one take's features (batch 1)."""
        m = self.cfg.fr_margin
        p = next(self.policy_net.parameters())
        cnn_feat = torch.as_tensor(cnn_feat_np, dtype=p.dtype, device=p.device)
        pol = self._policy_contexts(cnn_feat)
        self.value_vs_net.initialize(cnn_feat)
        state_pred = regressor_states(self.state_net, self.state_net_mean, self.state_net_std, cnn_feat, m)
        return dict(len=cnn_feat.shape[0] - 2 * m, pol=pol.float().contiguous(),
                    val=self.value_vs_net.v_out.float().contiguous(), state_pred=state_pred)

    def _policy_contexts(self, cnn_feat):
        """[len - 2m][v_hdim]: the policy's context per tick of a take (BatchedOnlineEvaluator: the online ones)."""
        self.policy_vs_net.initialize(cnn_feat)
        return self.policy_vs_net.v_out

    def _take_tables(self, i):
        env, m = self.env, self.cfg.fr_margin
        test_len = env.cnn_feat[i].shape[0] - 2 * m
        ex = env.expert_arr[i]
        if test_len < 1 or ex["qpos"].shape[0] < m + test_len:
            raise ValueError("take %s: no frames between the margins, or fewer expert frames than features" % env.expert_list[i])
        return dict(self._feature_tables(env.cnn_feat[i]), orig=np.array(ex["qpos"][m:m + test_len], float))

    # ------------------------------------------------------------------ ego_mimic_eval.py:93-100 for a set of slots
    @staticmethod
    def _seat_rows(states, ref_qpos):
        nq = ref_qpos.shape[1]
        qpos = np.array(ref_qpos, float, copy=True)
        qpos[:, 2:] = states[:, :nq - 2]
        qvel = np.array(states[:, nq - 2:], float, copy=True)
        for k in range(qpos.shape[0]):
            metrics.align_human_state(qpos[k], qvel[k], ref_qpos[k])
        return qpos, qvel

    def _reseat_below(self, i):
        """naivefs: the head height below which take i counts as fallen (env.py: HumanoidEnv.step)."""
        env = self.env
        return env.fix_head_lb if env.fix_head_lb is not None else float(env.expert_arr[i]["head_height_lb"]) - 0.1

    # ------------------------------------------------------------------ ego_mimic_eval.py:103-175 for N takes at a time
    @torch.no_grad()
    def _run_pass(self, take_inds, prefixes):
        """Run the takes `take_inds` (indices into the expert list), each from a copy of its prefix statistic, in passes of N
        slots -> [(values, taken re-seat decisions)]; the full records go to self._latest."""
        from .failsafe import below
        R = self._run
        lp, fused, v_dev, v_host, N = R["lp"], R["fused"], R["v_dev"], R["v_host"], self.num_envs
        eng = lp.eng

        def launch(t, k):
            fused.with_filter(lp.ctx, R["pol_slab"][:k], R["t_all"][t, :k], eng.qpos[:k], eng.qvel[:k], lp.zf_in, None, lp.clip, lp.states[t, :k],
                              None, None, lp.actions[t, :k], R["val_slab"][:k], v_dev[t, :k], phase_t=lp.phase_t(t))

        def value_copy(t):                         # to pinned memory, behind the event the env-step waits on -> its own event
            v_host[t].copy_(v_dev[t], non_blocking=True)
            ev_v = torch.cuda.Event()
            ev_v.record()
            return ev_v

        out = []
        for c0 in range(0, len(take_inds), N):
            chunk = take_inds[c0:c0 + N]
            k = len(chunk)
            tabs = [R["tables"][i] for i in chunk]
            lens = np.array([tb["len"] for tb in tabs])
            stats = [copy.deepcopy(st) for st in prefixes[c0:c0 + N]]
            for j, tb in enumerate(tabs):
                R["pol_slab"][j, :tb["len"]] = tb["pol"]
                R["val_slab"][j, :tb["len"]] = tb["val"]
            ref0 = np.stack([self._seat_ref(i) for i in chunk])
            active = lp.seat(*self._seat_rows(np.stack([tb["state_pred"][0] for tb in tabs]), ref0))
            resets = [[] for _ in range(k)]
            below_lb = np.array([self._reseat_below(i) for i in chunk]) if self.fail_safe == "naivefs" else None
            T = int(lens.max())
            for t in range(T):
                lp.tick(t, launch, value_copy).synchronize()
                flagged = []
                for j in range(k):
                    if not active[j]:
                        continue
                    value = float(v_host[t, j])
                    if stats[j] is not None:
                        stats[j].push(np.array([value]))
                    last = t + 1 >= lens[j]
                    if last and not self.DECIDE_ON_END:        # info['end']: no decision, the take is over
                        active[j] = 0
                        continue
                    if self.fail_safe == "valuefs":
                        hit = below(value, stats[j])
                    elif self.fail_safe == "naivefs":
                        hit = bool(eng.head_z[j] < below_lb[j])
                    else:
                        hit = False
                    if hit:
                        if not last:                           # (a decision on the take's last tick has no next frame to re-seat on)
                            flagged.append(j)
                        resets[j].append(t)
                    if last:
                        active[j] = 0
                if flagged:
                    fl = np.array(flagged)
                    lp.reseat(fl, *self._seat_rows(np.stack([tabs[j]["state_pred"][t + 1] for j in flagged]), np.array(eng.qpos_host[fl], float)))
            h_traj, h_qv, h_act, h_st = lp.copy_out(T, "traj", "qvel", "actions", "states")
            h_val = v_host[:T, :k].t().double().numpy().copy()
            for j, i in enumerate(chunk):
                L = int(lens[j])
                taken = np.zeros(L, bool)
                taken[resets[j]] = True
                self._latest[i] = dict(traj_pred=h_traj[j, :L].copy(), vel_pred=h_qv[j, :L].copy(), actions=h_act[j, :L].copy(),
                                       states=h_st[j, :L].copy(), values=h_val[j, :L].copy(), resets=list(resets[j]))
                out.append((h_val[j, :L], taken))
        return out

    def run(self, takes=None):
        """Evaluate every take of the env's expert list (or of `takes`) -> (results, meta) in the reference's pickle layout."""
        from . import policy_step
        N = self.num_envs
        sel = [i for i, take in enumerate(self._take_names()) if takes is None or take in takes]
        self.timing = tm = Timing(takes=len(sel), fs_passes=0, fs_pass_takes=[])
        self._latest = {}
        tables = {}
        if sel:
            with torch.no_grad(), torch.cuda.device(self.device_index):
                tables = {i: self._take_tables(i) for i in sel}
                Tm = max(tb["len"] for tb in tables.values())
                lp = LockstepPass(self.env, N, self.device_index, self.n_threads, self.running_state, Tm, tm)
                dev, f32 = lp.dev, torch.float32
                self._run = dict(lp=lp, tables=tables, fused=policy_step.FusedActorCritic(self.policy_net, self.value_net, dev),
                                 pol_slab=torch.zeros(N, Tm, self.policy_vs_net.v_hdim, dtype=f32, device=dev),
                                 val_slab=torch.zeros(N, Tm, self.value_vs_net.v_hdim, dtype=f32, device=dev),
                                 v_dev=torch.zeros(Tm, N, dtype=f32, device=dev), v_host=torch.zeros(Tm, N, dtype=f32).pin_memory(),
                                 t_all=torch.arange(Tm, dtype=torch.int64, device=dev).unsqueeze(1).expand(Tm, N).contiguous())
                if self.fail_safe == "valuefs":
                    self._fs.run(sel, self._run_pass)
                    tm["fs_passes"], tm["fs_pass_takes"] = self._fs.passes, list(self._fs.pass_takes)
                else:
                    self._run_pass(sel, [None] * len(sel))
                    tm["fs_passes"], tm["fs_pass_takes"] = 1, [len(sel)]
            self._run = None
        out = self._results(sel, tables)
        self._latest = None
        tm.close()
        return out

    def _results(self, sel, tables):
        traj_pred, traj_orig, vel_pred, num_reset = {}, {}, {}, 0
        names = self._take_names()
        for i in sel:
            take, rec = names[i], self._latest[i]
            traj_pred[take], vel_pred[take] = rec["traj_pred"], rec["vel_pred"]
            if "orig" in tables[i]:
                traj_orig[take] = tables[i]["orig"]
            num_reset += len(rec["resets"])
            if self.logger is not None:
                for _ in rec["resets"]:
                    self.logger.info("reset state!")
            if self.trace is not None:
                self.trace[take] = dict(actions=rec["actions"], values=rec["values"], resets=rec["resets"], state_pred=tables[i]["state_pred"],
                                        states=rec["states"])
        return {"traj_pred": traj_pred, "traj_orig": traj_orig, "vel_pred": vel_pred}, {"algo": "ego_mimic", "num_reset": num_reset}


class BatchedOnlineEvaluator(BatchedEvaluator):
    """The online evaluation (ego_mimic_eval.py --causal) on lockstep slots: the policy's context at tick t is its video net over the
    frames up to t + 2 * fr_margin only (module docstring). Everything else -- the pass, the fused launch, the fail-safe scheduler,
    the records -- is BatchedEvaluator's; `save()` writes iter_%04d_<data>[_<fail_safe>]_causal.p."""

    def __init__(self, cfg, env, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                 running_state=None, fail_safe="valuefs", sync=False, logger=None, keep_trace=False, num_envs=8, device_index=0,
                 n_threads=None):
        super().__init__(cfg, env, policy_net, policy_vs_net, value_net, value_vs_net, state_net, state_net_mean, state_net_std,
                         running_state=running_state, fail_safe=fail_safe, sync=sync, logger=logger, keep_trace=keep_trace,
                         num_envs=num_envs, device_index=device_index, n_threads=n_threads)
        self.causal = True

    def _policy_contexts(self, cnn_feat):
        return self.policy_vs_net.online_contexts(cnn_feat)


def select_evaluator(policy_net, value_net, num_envs=1, sequential=False, causal=False, show_noise=False, batched_online=False):
    """Which evaluator `main()` uses -> (class, reason or None): BatchedEvaluator for num_envs > 1 -- BatchedOnlineEvaluator for a
    `causal` run when the caller can take it (`batched_online`) -- unless something needs the take-by-take path (then Evaluator,
    with the reason to print)."""
    from . import policy_step
    if sequential or int(num_envs) <= 1:
        return Evaluator, None
    if show_noise or (causal and not batched_online):
        return Evaluator, "--causal / --show-noise run take by take"
    if not (policy_step.supported(policy_net) and policy_step.supported_value(value_net)):
        return Evaluator, "the nets are outside the fused actor + critic step (float32 PolicyGaussian and Value over plain MLPs)"
    return (BatchedOnlineEvaluator if causal else BatchedEvaluator), None


def compute_metrics(results, dt=1.0 / 30.0, algo="ego_mimic", verbose=False):
    return metrics.compute_metrics(results, dt, algo, verbose)


def main(argv=None):
    """`python -m egopose_amd.evaluate --cfg subject_03 --iter 3000 --data test [--fail-safe naivefs] [--causal] [--num-envs N] [--sequential]`:
    the non-rendering part of ego_pose/ego_mimic_eval.py (checkpoint + state-net loading: :60-80) followed by the
    statistics of ego_pose/eval_pose.py (--mode stats). `--mode stats [--statereg-cfg S --statereg-iter M] [--joint-pos] [--keep-hands]
    [--host]` is that script's stats mode on the saved results; `--joint-pos` adds the joint-position metrics (`egopose_amd.pose3d`);
    `--physical [--contacts FILE] [--contact-height H] [--ground-z Z]` adds foot skate, ground penetration and floating
    (`egopose_amd.plausibility`) in the modes eval, stats and wild-stats."""
    import argparse
    from .config import Config
    from .env import HumanoidEnv
    from .evaluate_wild import BatchedWildEvaluator, WildEvaluator, cli_takes
    from .nets import MLP, PolicyGaussian, Value, VideoRegNet, VideoStateNet
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="subject_03")
    ap.add_argument("--iter", type=int, default=0)
    ap.add_argument("--data", default="test")
    ap.add_argument("--fail-safe", default="valuefs")
    ap.add_argument("--causal", action="store_true")
    ap.add_argument("--show-noise", action="store_true")
    ap.add_argument("--gpu-index", type=int, default=0)
    ap.add_argument("--num-envs", type=int, default=1,
                    help="> 1: takes side by side on that many env slots (BatchedEvaluator; with --causal BatchedOnlineEvaluator)")
    ap.add_argument("--sequential", action="store_true", help="take by take (Evaluator) whatever --num-envs says")
    ap.add_argument("--test-feat", default=None, help="evaluate the feature-only takes of datasets/features/cnn_feat_<NAME>.p (no MoCap)")
    ap.add_argument("--mode", default="eval", choices=["eval", "wild-stats", "stats"],
                    help="wild-stats: 2D keypoint statistics of saved --test-feat results; stats: the statistics of saved --data results")
    ap.add_argument("--statereg-cfg", default=None, help="wild-stats, stats: also score the state regressor's results of this config")
    ap.add_argument("--statereg-iter", type=int, default=100)
    ap.add_argument("--host", action="store_true", help="wild-stats, stats, --joint-pos, --physical: the per-frame numpy loop instead of the GPU kernel")
    ap.add_argument("--joint-pos", action="store_true", help="eval, stats: also the joint-position metrics (MPJPE, PA-MPJPE; egopose_amd.pose3d)")
    ap.add_argument("--keep-hands", action="store_true", help="--joint-pos: count the hands too (left out by default: noisy in some captures)")
    from . import plausibility
    plausibility.add_arguments(ap)             # --physical [--contacts FILE] [--contact-height H] [--ground-z Z]: eval, stats, wild-stats
    args = ap.parse_args(argv)
    cfg = Config(args.cfg, create_dirs=False)
    if args.mode == "wild-stats":
        return _wild_stats(cfg, args)
    if args.mode == "stats":
        return _stats(cfg, args)
    if args.joint_pos and args.test_feat is not None:
        raise SystemExit("--joint-pos needs MoCap: not with --test-feat")
    dev, dtype = torch.device("cuda", args.gpu_index), torch.float32
    env = HumanoidEnv(cfg)
    env.seed(cfg.seed)
    cnn_feat_dict, cnn_dim = cli_takes(cfg, env, args.data, args.test_feat)
    sd, ad = env.observation_space.shape[0], env.action_space.shape[0]
    mk = lambda hdim, kind, param: VideoStateNet(cnn_dim, hdim, cfg.fr_margin, kind, param, cfg.causal)
    policy_vs, value_vs = mk(cfg.policy_v_hdim, cfg.policy_v_net, cfg.policy_v_net_param), mk(cfg.value_v_hdim, cfg.value_v_net, cfg.value_v_net_param)
    policy = PolicyGaussian(MLP(sd + cfg.policy_v_hdim, cfg.policy_hsize, cfg.policy_htype), ad, log_std=cfg.log_std, fix_std=cfg.fix_std)
    value = Value(MLP(sd + cfg.value_v_hdim, cfg.value_hsize, cfg.value_htype))
    from .zfilter import load_reference_pickle
    with open("%s/iter_%04d.p" % (cfg.model_dir, args.iter), "rb") as f:      # checkpoints written by the reference name utils.zfilter.ZFilter
        cp = load_reference_pickle(f)
    policy.load_state_dict(cp["policy_dict"]); policy_vs.load_state_dict(cp["policy_vs_dict"])
    value.load_state_dict(cp["value_dict"]); value_vs.load_state_dict(cp["value_vs_dict"])
    sn_cp, meta = pickle.load(open(cfg.state_net_model, "rb"))
    sn_cfg = meta["cfg"]
    state_net = VideoRegNet(meta["mean"].size, sn_cfg.v_hdim, cnn_dim, no_cnn=True, cnn_type=sn_cfg.cnn_type, mlp_dim=sn_cfg.mlp_dim,
                            v_net_type=sn_cfg.v_net, v_net_param=sn_cfg.v_net_param, causal=sn_cfg.causal)
    state_net.load_state_dict(sn_cp["state_net_dict"])
    for net in (policy, policy_vs, value, value_vs, state_net):
        net.to(dev, dtype)
    # (the feature-only takes have no online mode: the reference has none)
    cls, why = select_evaluator(policy, value, args.num_envs, args.sequential, args.causal, args.show_noise, batched_online=cnn_feat_dict is None)
    if why is not None:
        print("falling back to the sequential Evaluator: %s" % why)
    if cnn_feat_dict is not None:
        nets = (policy, policy_vs, value, value_vs, state_net, meta["mean"], meta["std"])
        if cls is BatchedEvaluator:
            ev = BatchedWildEvaluator(cfg, env, cnn_feat_dict, *nets, running_state=cp["running_state"], num_envs=args.num_envs,
                                      device_index=args.gpu_index)
        else:
            ev = WildEvaluator(cfg, env, cnn_feat_dict, *nets, running_state=cp["running_state"], show_noise=args.show_noise)
        results, rmeta = ev.run()
        path = ev.save(results, rmeta, args.iter, args.test_feat)
        print("num reset: %d, saved results to %s" % (ev.num_reset, path))
        if args.physical:
            plausibility.from_args(results, cfg, args, "ego_mimic")
        env.close()
        return
    if cls is not Evaluator:                           # BatchedEvaluator, or BatchedOnlineEvaluator for --causal
        if args.fail_safe == "naivefs":
            env.set_fix_head_lb(0.3)                   # ego_mimic_eval.py:51-52 (the sequential path keeps the take's own bound)
        ev = cls(cfg, env, policy, policy_vs, value, value_vs, state_net, meta["mean"], meta["std"], running_state=cp["running_state"],
                 fail_safe=args.fail_safe, num_envs=args.num_envs, device_index=args.gpu_index)
    else:
        ev = Evaluator(cfg, env, policy, policy_vs, value, value_vs, state_net, meta["mean"], meta["std"], running_state=cp["running_state"],
                       fail_safe=args.fail_safe, causal=args.causal, show_noise=args.show_noise)
    results, rmeta = ev.run()
    path = ev.save(results, rmeta, args.iter, args.data)
    print("num reset: %d, saved results to %s" % (rmeta["num_reset"], path))
    compute_metrics(results, verbose=True)
    if args.joint_pos:
        _joint_pos(results, cfg, args, "ego_mimic", table=False)
    if args.physical:
        plausibility.from_args(results, cfg, args, "ego_mimic", which=("traj_pred", "traj_orig"))
    env.close()


def _joint_pos(results, cfg, args, algo, table=True, ctx=None):
    """The `--joint-pos` figures of `results`: the 3D line in millimetres (and the per-body table), hands out of the mask unless --keep-hands."""
    from . import pose3d
    from .skeleton import load_skeleton
    skel = load_skeleton()
    mask = pose3d.body_mask(skel, () if args.keep_hands else pose3d.HANDS)
    out = pose3d.compute_joint_metrics(results, skel, mask=mask, backend="host" if args.host else "hip", ctx=ctx, cfg=cfg, algo=algo,
                                       verbose=table, device_index=args.gpu_index)
    if not table:
        print(pose3d.format_line([out[k] for k in pose3d.FIGURES]))
    return out


def _stats(cfg, args):
    """eval_pose.py --mode stats (:72-87): the three numbers of the SAVED ego_mimic result and, with --statereg-cfg, of the state
    regressor's beside it, after remove_noisy_hands on copies; with --joint-pos also the joint-position figures of both."""
    from .statereg import StateRegConfig
    fs_tag = "" if args.fail_safe == "valuefs" else "_" + args.fail_safe
    jobs = [("ego mimic", "%s/iter_%04d_%s%s%s.p" % (cfg.result_dir, args.iter, args.data, fs_tag, "_causal" if args.causal else ""))]
    if args.statereg_cfg is not None:
        sr_cfg = StateRegConfig(args.statereg_cfg, create_dirs=False)
        jobs.append(("state reg", "%s/iter_%04d_%s.p" % (sr_cfg.result_dir, args.statereg_iter, args.data)))
    ctx = None
    if (args.joint_pos or args.physical) and not args.host:
        from .pose2d import context_of
        ctx = context_of(cfg, device_index=args.gpu_index)
    out = {}
    try:
        for i, (algo, path) in enumerate(jobs):
            with open(path, "rb") as f:
                saved, _ = pickle.load(f)
            res = {k: {take: np.array(tr, float, copy=True) for take, tr in saved[k].items()} for k in ("traj_pred", "traj_orig")}
            metrics.remove_noisy_hands(res)
            out[algo] = metrics.compute_metrics(res, algo=algo, verbose=True)
            if args.joint_pos:
                out[algo]["joint_pos"] = _joint_pos(res, cfg, args, algo, ctx=ctx)
            if args.physical:                  # one row per algorithm, and after the last one what MoCap itself reaches
                from . import plausibility
                which = ("traj_pred", "traj_orig") if i == len(jobs) - 1 else ("traj_pred",)
                out[algo]["physical"] = plausibility.from_args(res, cfg, args, algo, which=which, ctx=ctx, what=algo)
    finally:
        if ctx is not None:
            ctx.close()
    return out


def _wild_stats(cfg, args):
    """eval_pose_wild.py --mode stats: the 2D keypoint distance and the smoothness of the saved wild results."""
    from . import pose2d
    from .statereg import StateRegConfig
    meta, pose_ctx, loader = pose2d.wild_stats_front(cfg, args.test_feat)
    jobs = [("ego mimic", "%s/iter_%04d_%s.p" % (cfg.result_dir, args.iter, args.test_feat))]
    if args.statereg_cfg is not None:
        sr_cfg = StateRegConfig(args.statereg_cfg, create_dirs=False)
        jobs.append(("state reg", "%s/iter_%04d_%s.p" % (sr_cfg.result_dir, args.statereg_iter, args.test_feat)))
    out = {}
    for algo, path in jobs:
        with open(path, "rb") as f:
            res, _ = pickle.load(f)
        out[algo] = pose2d.eval_pose_wild_stats(res, meta, loader, cfg, backend="host" if args.host else "hip", pose_ctx=pose_ctx,
                                                algo=algo, verbose=True, device_index=args.gpu_index)
        if args.physical:                      # the only 3D figures of takes without MoCap
            from . import plausibility
            out[algo]["physical"] = plausibility.from_args(res, cfg, args, algo, what=algo)
    return out


if __name__ == "__main__":
    main()
