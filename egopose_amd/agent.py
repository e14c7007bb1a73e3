"""PPO agents on the batched rollout (drop-in for the reference's agent classes on the ego_mimic path).

  Agent      agents/agent.py:9-122       sample() -> (TrajBatch, LoggerRL); hooks; set_noise_rate
  AgentPG    agents/agent_pg.py:7-57     update_value / update_policy (A2C) / update_params
  AgentPPO   agents/agent_ppo.py:6-65    clipped-surrogate update, grad-norm clip
  AgentEgo   ego_pose/core/agent_ego.py:8-57   video-context nets, v_metas, TrajBatchEgo
  AgentVGAIL ego_pose/core/agent_vgail.py:7-88 AgentEgo + a video-conditioned GAIL discriminator trained after every PPO update

Constructor keywords are the reference's. ``sample`` does not fork Python workers: it drives
``LockstepRollout`` over ``num_envs`` env slots of this rank's GPU (``num_threads`` becomes the number of
host physics threads). ``update_params`` keeps everything in HBM: values -> K5 GAE (+ global
standardisation) -> ``opt_num_epochs`` full-batch epochs; with ``torch.distributed`` initialised the flat
policy+value gradient is all-reduced once per epoch (RCCL over xGMI) so that every rank applies the
gradient of the global batch mean, exactly what the reference's single-process full batch computes.

Precision. The reference driver builds everything in float64 (ego_pose/ego_mimic.py:31-32,83-90) and hands
``dtype=torch.float64`` nets to ``AgentEgo``. The HIP LSTM / fused policy kernels and the MFMA GEMMs are float32, so
on a GPU a float64 agent keeps the caller's float64 modules as MASTER weights (state_dict, checkpoints, the caller's
optimizers step them) and computes with float32 SHADOW copies (``ShadowNets``): shadow gradients are copied up into
the masters' ``.grad`` before the all-reduce / clip / optimizer steps, the stepped masters are copied down again.
``EGP_NET_DTYPE=float64`` keeps a float64 agent on the float64 torch paths (parity runs at 1e-9).

The update step. Every optimizer step of every agent is one protocol on a stepper -- ``optim.FlatUpdater`` (fused clip + Adam
over flat buffers) when the set-up is the one its kernels implement, else ``optim.TorchUpdater`` (the caller's optimizers step
themselves): ``zero_grad()``, the caller's forward and backward, then ``collect_grads`` (shadow gradients -> masters),
``all_reduce``, ``step`` (value step, clip, policy step; compute copies refreshed). ``AgentPG`` builds one stepper for
(optimizer_value, optimizer_policy) on first use, ``AgentVGAIL`` another for (optimizer_discrim,) -- and a ``TorchUpdater`` of
its own for the plain form of the discriminator update, the reference's loop in torch ops that the fused form is tested against.
"""
from __future__ import annotations

import copy
import math
import os
import sys
import time
import types

import numpy as np
import torch

from . import dist as D
from . import optim as O
from .rl_core import LoggerRL, TrajBatch, TrajBatchEgo
from .torch_utils import to_test, to_train


def _column(batch, name, dtype, device):
    col = batch.device_column(name) if hasattr(batch, "device_column") else None
    if col is not None and col.device == device:
        return col.to(dtype)
    return torch.from_numpy(np.asarray(getattr(batch, name))).to(dtype).to(device)


def compute_dtype(dtype, device):
    """Arithmetic type of the nets for an agent declared with `dtype` on `device` (see the module docstring)."""
    if dtype == torch.float64 and torch.device(device).type == "cuda":
        want = os.environ.get("EGP_NET_DTYPE", "float32")
        if want not in ("float32", "float64"):
            raise ValueError("EGP_NET_DTYPE must be float32 or float64, got %r" % want)
        return getattr(torch, want)
    return dtype


class ShadowNets:
    """Low-precision compute copies of the caller's (master) modules, matched parameter by parameter."""

    def __init__(self, masters, dtype):
        self.masters = dict(masters)
        self.nets = {k: copy.deepcopy(m).to(dtype) for k, m in self.masters.items()}
        self.pairs = []
        for k, m in self.masters.items():
            mp, sp = dict(m.named_parameters()), dict(self.nets[k].named_parameters())
            if list(mp) != list(sp):
                raise RuntimeError("shadow copy of %s lost parameters" % k)
            self.pairs += [(mp[n], sp[n]) for n in mp]
        self._train = [(m, s) for m, s in self.pairs if m.requires_grad]

    @torch.no_grad()
    def pull(self):
        """masters -> shadows (after an optimizer step, a checkpoint load or the driver's `action_log_std.fill_`)."""
        dst, src = [s for _, s in self.pairs], [m for m, _ in self.pairs]
        if all(m.device == s.device for m, s in self.pairs):
            torch._foreach_copy_(dst, src)
        else:                                   # masters parked on the CPU (the driver's `with to_cpu(...)`)
            for d, m in zip(dst, src):
                d.copy_(m)

    def zero_grad(self):
        for _, s in self._train:
            s.grad = None

    @torch.no_grad()
    def push_grads(self):
        """shadow gradients -> the masters' .grad (master dtype), where the exchange / clip / optimizer steps find them."""
        dst, src = [], []
        for m, s in self._train:
            if s.grad is None:
                m.grad = None
                continue
            if m.grad is None or m.grad.shape != s.grad.shape:
                m.grad = torch.empty_like(m)
            dst.append(m.grad)
            src.append(s.grad)
        if dst:
            torch._foreach_copy_(dst, src)


class Agent:

    def __init__(self, env, policy_net, value_net, dtype, device, custom_reward=None, mean_action=False,
                 render=False, running_state=None, num_threads=1, num_envs=None, num_groups=None, net_dtype=None):
        self.env, self.policy_net, self.value_net = env, policy_net, value_net
        self.dtype, self.device = dtype, device
        self.cdtype = net_dtype if net_dtype is not None else compute_dtype(dtype, device)         # what the nets compute in (float32 shadows of float64 masters)
        self.shadow = None
        self.cn = types.SimpleNamespace(policy_net=policy_net, value_net=value_net)     # the nets the kernels run
        self.custom_reward = custom_reward
        self.mean_action, self.render = mean_action, render
        self.running_state = running_state
        self.num_threads = num_threads
        self.num_envs = int(num_envs if num_envs is not None else os.environ.get("EGP_NUM_ENVS", 1024))
        self.num_groups = int(num_groups if num_groups is not None else os.environ.get("EGP_NUM_GROUPS", 2))
        self.noise_rate = 1.0
        self.traj_cls = TrajBatch
        self.logger_cls = LoggerRL
        self._rollout = None
        self._steppers = []         # every update stepper built so far (see the module docstring)
        self._bind_compute_nets()
        if self.cdtype != self.dtype and os.environ.get("EGP_QUIET", "0") != "1":
            #  a float64 driver gets float32 arithmetic on the GPU: say so once, where the agent is built
            print("egopose_amd: agent declared %s computes in %s on %s (float64 master weights for checkpoints / optimizers; "
                  "EGP_NET_DTYPE=float64 keeps float64 arithmetic)" % (str(self.dtype).replace("torch.", ""),
                                                                     str(self.cdtype).replace("torch.", ""), self.device), file=sys.stderr)

    def _master_nets(self):
        return dict(policy_net=self.policy_net, value_net=self.value_net)

    def _bind_compute_nets(self):
        """self.cn = the modules every kernel runs: the caller's own, or float32 shadows of float64 masters."""
        masters = self._master_nets()
        if any(m is None for m in masters.values()):
            masters = {k: m for k, m in masters.items() if m is not None}        # (AgentEgo binds again with its video nets)
            self.shadow, self.cn = None, types.SimpleNamespace(**masters)
        elif self.cdtype != self.dtype:
            self.shadow = ShadowNets(masters, self.cdtype)
            self.cn = types.SimpleNamespace(**self.shadow.nets)
        else:
            self.shadow = None
            self.cn = types.SimpleNamespace(**masters)
        self.sample_modules = [self.cn.policy_net]
        self.update_modules = [self.cn.policy_net, self.cn.value_net]

    def _params_stepped(self):
        for up in self._steppers:
            up.rebind()          # (a caller may have moved its modules: `with to_cpu(...)` around a checkpoint)
        if self.shadow is not None:
            self.shadow.pull()

    # hooks kept for subclasses / API compatibility
    def pre_episode(self):
        return

    def pre_sample(self):
        return

    def push_memory(self, memory, state, action, mask, next_state, reward, exp):
        memory.push(state, action, mask, next_state, reward, exp)

    def trans_policy(self, states):
        return states

    def trans_value(self, states):
        return states

    def set_noise_rate(self, noise_rate):
        self.noise_rate = noise_rate

    def _video_net(self):
        raise NotImplementedError("the batched sampler is built for AgentEgo (video-context policy)")

    def _get_rollout(self):
        if self._rollout is None:
            from .rollout import LockstepRollout
            dev = torch.device(self.device)
            if dev.type != "cuda":
                raise RuntimeError("egopose_amd samples on an MI355X only: device=%s has no HIP path (no CPU fallback)" % (dev,))
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            reward_id = getattr(self.env.cfg, "reward_id", "quat_v3")
            # custom_reward=None (agents/agent.py:53-58): the batch trains on the ENV's reward (HumanoidEnv.step returns 1.0 per
            # step, humanoid_v1.py:188) and the logger sees c_reward = 0, c_info = [0] -- kind 'env', never a silent quat_v3
            # a callable without a kernel (anything but the registry's three): the reference's plug point as it is -- evaluated on the
            # host per stepped slot through env.SlotView, kind 'callable' (slow by construction; the registry's rewards never go there)
            kind = "env" if self.custom_reward is None else getattr(self.custom_reward, "egp_kernel", "callable")
            if kind not in ("env", "quat_v3", "constant", "pose_dist", "callable") or (kind == "callable" and not callable(self.custom_reward)):
                raise NotImplementedError("custom_reward %r: unknown kernel tag %r (reward_id=%s)" % (self.custom_reward, kind, reward_id))
            n_threads = None if self.num_threads in (None, 0) else int(self.num_threads)
            sim = self.env.batched(self.num_envs, idx, n_threads=n_threads, n_groups=self.num_groups)
            seed = int(getattr(self.env.cfg, "seed", 0)) * 1000 + D.rank()
            self._rollout = LockstepRollout(sim, self.cn.policy_net, self._video_net(), self.running_state, seed=seed)
            self._rollout.reward_kind = kind
            self._rollout.custom_reward = self.custom_reward if kind == "callable" else None
        return self._rollout

    def sample(self, min_batch_size):
        t0 = time.time()
        self._params_stepped()              # shadows follow whatever the caller did to the masters since the last call
        self.pre_sample()
        ro = self._get_rollout()
        ro.noise_rate, ro.mean_action = self.noise_rate, self.mean_action
        ro.sim.ctx.set_reward_weights(self.env.cfg.reward_weights)
        with to_test(*self.sample_modules):
            per_rank = int(math.ceil(min_batch_size / D.world_size()))
            self._last_min_batch = per_rank
            batch, log = ro.sample(per_rank, end_reward=float(self.env.end_reward))
        if D.world_size() > 1:      # logger totals + filter deltas: one all-gather, merged on the device (scalars beside the update's collectives)
            log = D.merge_sampling_pass(log, self.running_state, ro.zf_delta_base if self.running_state is not None else None, self.device)
        log.sample_time = time.time() - t0
        return batch, log


class AgentPG(Agent):

    def __init__(self, gamma=0.99, tau=0.95, optimizer_policy=None, optimizer_value=None, opt_num_epochs=1,
                 value_opt_niter=1, **kwargs):
        super().__init__(**kwargs)
        self.gamma, self.tau = gamma, tau
        self.optimizer_policy, self.optimizer_value = optimizer_policy, optimizer_value
        self.opt_num_epochs, self.value_opt_niter = opt_num_epochs, value_opt_niter
        self._stepper = None            # the stepper of (optimizer_value, optimizer_policy), built on first use
        # A/B handles of the update's fused forms (the tests run both sides; all on by default, no environment switches):
        self.use_fused_optim = True     # clip + both Adam steps over flat buffers (optim.FlatUpdater) instead of the torch optimizers
        self.use_fused_loss = True      # both losses and their output gradients in one launch (optim.ppo_losses)
        self.share_train_context = True    # the value net adopts the policy net's segmented batch (VideoStateNet.adopt_train_context)
        self.reuse_first_pass = True    # the no-grad value / fixed-log-prob pass doubles as epoch 0's forward
        self.update_stats = {}

    # -- pieces shared by the A2C and PPO updates -------------------------------------------------
    def _advantages(self, rewards, masks, values):
        """K5 on device + standardisation with the GLOBAL mean / unbiased std (core/common.py:5-25). This rank's sample
        counts left in `self._pending_counts` (rows, exploration rows) ride in the same all-reduce as the advantage moments and
        come back as `self._global_counts`: one scalar exchange per update."""
        ctx = self._kernel_ctx()
        adv, ret, stats = ctx.gae(rewards.contiguous(), masks.contiguous(), values.reshape(-1).contiguous(), self.gamma, self.tau)
        stats, self._global_counts = D.merge_moments_and_counts(stats, getattr(self, "_pending_counts", None))
        ctx.gae_standardize(adv, stats)
        return adv.unsqueeze(1), ret.unsqueeze(1)

    def _advantages_with_counts(self, rewards, masks, values, counts):
        """-> (advantages, returns, global counts or None). None: `_advantages` was replaced (tests put the oracle's GAE
        there) and did not exchange the counts; update_policy then does it itself."""
        self._pending_counts, self._global_counts = counts, None
        try:
            adv, ret = self._advantages(rewards, masks, values)
        finally:
            self._pending_counts = None
        return adv, ret, self._global_counts

    def _kernel_ctx(self):
        return self._get_rollout().sim.ctx

    def _policy_params(self):
        return [p for g in self.optimizer_policy.param_groups for p in g["params"]]

    def _clip_list(self):
        return []

    def _build_stepper(self, optimizers, clip, pre_step, flat=True):
        """The stepper of `optimizers`: optim.FlatUpdater (`clip` = its clip groups) when `flat`, on the GPU with use_fused_optim
        and a set-up its kernels implement, else optim.TorchUpdater (`pre_step` = its clip callables)."""
        up = None
        if flat and torch.device(self.device).type == "cuda" and self.use_fused_optim and all(o is not None for o in optimizers):
            compute_of = {m: c for m, c in self.shadow.pairs} if self.shadow is not None else None
            up = O.FlatUpdater.build(optimizers, clip, compute_of)
        if up is None:
            up = O.TorchUpdater(optimizers, self.shadow, pre_step)
        self._steppers.append(up)
        return up

    def _get_stepper(self):
        if self._stepper is None:
            self._stepper = self._build_stepper([self.optimizer_value, self.optimizer_policy], self._clip_list(),
                                                {1: lambda: self.clip_policy_grad()})
        return self._stepper

    def _get_updater(self):
        """optim.FlatUpdater for this agent's two optimizers, or None (CPU device, non-Adam optimizers, use_fused_optim = False, ...)."""
        up = self._get_stepper()
        return up if isinstance(up, O.FlatUpdater) else None

    def _zero_grads(self):
        self._get_stepper().zero_grad()

    def _optim_step(self, which=(0, 1)):
        """After backward: gradient exchange, clip, optimizer steps (0 = value, 1 = policy; the reference steps the critic
        first, agents/agent_ppo.py:24-30), compute copies refreshed."""
        up = self._get_stepper()
        up.collect_grads(which)
        up.all_reduce(which)
        up.step(which)

    def clip_policy_grad(self):
        return

    def _value_backward(self, states, returns, n_global):
        """MSE critic loss of the global batch (this rank's share) -> gradients, no optimizer step."""
        if self.value_opt_niter != 1:
            raise NotImplementedError("value_opt_niter != 1 is not on the ego_mimic path")
        pred = self.cn.value_net(self.trans_value(states))
        loss = (pred - returns).pow(2).sum() / n_global
        loss.backward()
        return loss

    def update_value(self, states, returns):
        """update critic (agents/agent_pg.py:19-26)"""
        self._zero_grads()
        loss = self._value_backward(states, returns, D.global_count(states.shape[0], states.device))
        self._optim_step(which=(0,))
        return loss

    def update_policy(self, states, actions, returns, advantages, exps):
        ind = exps.nonzero().squeeze(1)
        n_val = D.global_count(states.shape[0], states.device)
        n_exp = D.global_count(ind.shape[0], states.device)
        for _ in range(self.opt_num_epochs):
            self._zero_grads()
            self._value_backward(states, returns, n_val)
            logp = self.cn.policy_net.get_log_prob(self.trans_policy(states)[ind], actions[ind])
            loss = -(logp * advantages[ind]).sum() / n_exp
            loss.backward()
            self._optim_step()

    def _load_batch(self, batch):
        dev = torch.device(self.device)
        cols = {k: _column(batch, k, self.cdtype, dev) for k in ("states", "actions", "rewards", "masks", "exps")}
        return cols

    def update_params(self, batch):
        t0 = time.time()
        to_train(*self.update_modules)
        self._params_stepped()
        c = self._load_batch(batch)
        with to_test(*self.update_modules):
            with torch.no_grad():
                values = self.cn.value_net(self.trans_value(c["states"]))
        advantages, returns = self._advantages(c["rewards"], c["masks"], values)
        self.update_policy(c["states"], c["actions"], returns, advantages, c["exps"])
        return time.time() - t0


class AgentPPO(AgentPG):

    def __init__(self, clip_epsilon=0.2, opt_batch_size=64, use_mini_batch=False, policy_grad_clip=None, target_kl=None,
                 update_diagnostics=False, stop_on_nonfinite=False, **kwargs):
        """The last three keywords switch the update monitor on (all off = the reference's update, nothing added):
          update_diagnostics  every full-batch epoch also evaluates the monitor's record (optim.ppo_stats: one more launch per
                              epoch on the fused path; optim.ppo_stats_torch on the plain one). `update_stats` gains one list per
                              figure of optim.stats_summary with one entry per epoch that took its step, `epochs_run`,
                              `stop_reason` (None) and `stop_figures` (None). The records are read with the losses, after the
                              last epoch is queued: no host synchronisation is added.
          target_kl           stop the epochs once approx_kl (the k3 estimate of KL(sampling policy || current policy), mean over
                              the exploration rows) exceeds it: `stop_reason` "kl". A NaN estimate (no exploration rows) never stops.
          stop_on_nonfinite   stop before any step of an epoch whose inputs hold a non-finite value (a NaN advantage, an inf
                              value): `stop_reason` "nonfinite".
        Either of the last two makes the host read the epoch's record -- ONE small device-to-host copy per epoch, after the
        epoch's loss and monitor launches and BEFORE its backward pass -- and, with more than one rank, one all-gather of the
        records per epoch, so that every rank decides from the same global figures (ranks deciding differently would deadlock
        in the gradient all-reduce). A stopped epoch takes no backward pass, no gradient exchange and no optimizer step:
        parameters, Adam moments and step counts are those after the previous epoch; its figures are `stop_figures`."""
        super().__init__(**kwargs)
        self.clip_epsilon, self.opt_batch_size = clip_epsilon, opt_batch_size
        self.use_mini_batch, self.policy_grad_clip = use_mini_batch, policy_grad_clip
        self.target_kl = None if target_kl is None else float(target_kl)
        self.update_diagnostics, self.stop_on_nonfinite = bool(update_diagnostics), bool(stop_on_nonfinite)
        if self.target_kl is not None and not self.target_kl >= 0:
            raise ValueError("target_kl must be a number >= 0 (or None), got %r" % (target_kl,))
        if use_mini_batch and self._monitor_on():
            raise ValueError("the update monitor (target_kl / update_diagnostics / stop_on_nonfinite) covers the full-batch update: with "
                             "use_mini_batch=True an epoch is thousands of windows, each with its own step")

    # -- the update monitor ----------------------------------------------------------------------------
    def _monitor_on(self):
        return self.update_diagnostics or self._monitor_gated()

    def _monitor_gated(self):
        """True when the host decides after every epoch's record whether the epoch takes its step."""
        return self.target_kl is not None or self.stop_on_nonfinite

    def _gather_records(self, recs):
        """`recs` (k, fields) float64, this rank's records of k epochs -> host lists [rank][epoch][field]: one device-to-host
        copy, after one all-gather when there are several ranks."""
        if D.world_size() == 1:
            return [recs.tolist()]
        mine = recs.to(D._comm_device(recs.device)).contiguous()
        rows = torch.empty((D.world_size(),) + tuple(mine.shape), dtype=mine.dtype, device=mine.device)
        if torch.distributed.get_backend() != "gloo":
            torch.distributed.all_gather_into_tensor(rows, mine)
        else:
            torch.distributed.all_gather(list(rows.unbind(0)), mine)
        D._note()
        return rows.tolist()

    def _monitor_decide(self, fig):
        """The stop rule on the GLOBAL figures of one epoch -> "nonfinite", "kl" or None."""
        if self.stop_on_nonfinite and fig["nonfinite_rows"] > 0:
            return "nonfinite"
        if self.target_kl is not None and fig["approx_kl"] > self.target_kl:        # (NaN compares False: no exploration rows, no stop)
            return "kl"
        return None

    def _monitor_gate(self, rec):
        """After an epoch's launches: read its record `rec` (fields,), combine the ranks' -> (figures, stop reason or None)."""
        fig = O.stats_summary([r[0] for r in self._gather_records(rec.unsqueeze(0))])
        return fig, self._monitor_decide(fig)

    def _monitor_publish(self, stats, figs, epochs_run, reason):
        """`figs`: the figures of every epoch evaluated, in order (the stopped one last)."""
        for k in O.STATS_KEYS:
            stats[k] = [f[k] for f in figs[:epochs_run]]
        stats["epochs_run"], stats["stop_reason"] = epochs_run, reason
        stats["stop_figures"] = figs[epochs_run] if reason is not None else None
        return stats

    def _group_contexts(self, states=None):
        """Hook: prepare the critic's and the actor's state transforms together (AgentEgo). False = nothing prepared."""
        return False

    def _dropout_active(self):
        """True when a module of the update draws dropout masks in train mode (a TCN video net with dropout > 0): a train-mode
        forward pass then is not the eval-mode pass the reference takes its GAE values and fixed log-probs from."""
        for net in self.update_modules:
            for m in net.modules():
                p = m.p if isinstance(m, torch.nn.modules.dropout._DropoutNd) else getattr(m, "dropout", 0.0)
                if isinstance(p, (int, float)) and p > 0:
                    return True
        return False

    def _clip_list(self):
        return [(list(params), max_norm) for params, max_norm in (self.policy_grad_clip or [])]

    def clip_policy_grad(self):
        if self.policy_grad_clip is not None:
            for params, max_norm in self.policy_grad_clip:
                torch.nn.utils.clip_grad_norm_(params, max_norm)

    def _fused_losses(self):
        """Both losses and their gradients w.r.t. the nets' outputs from ONE HIP launch (optim.ppo_losses) instead of ~35
        element-wise library kernels per epoch: float32 compute nets on the GPU with a Gaussian policy head."""
        pol = self.cn.policy_net
        ls = getattr(pol, "action_log_std", None)
        return (torch.device(self.device).type == "cuda" and self.cdtype == torch.float32 and self.value_opt_niter == 1
                and hasattr(pol, "mean_std") and ls is not None and ls.dim() == 2 and ls.shape[0] == 1 and ls.shape[1] <= 256
                and ls.dtype == torch.float32 and self.use_fused_loss)

    def ppo_loss(self, states, actions, advantages, fixed_log_probs, ind, n_exp=None):
        """`ind` = rows with exps == 1 (agents/agent_ppo.py:45-51), or None when that is every row (no gather copies)."""
        logp = self._policy_head(states, actions, ind, False)
        if ind is not None:
            advantages, fixed_log_probs = advantages[ind], fixed_log_probs[ind]
        return self._surrogate(logp, advantages, fixed_log_probs, logp.shape[0] if n_exp is None else n_exp)

    def _exploration_rows(self, exps, n):
        """Rows with exps == 1 (agents/agent_ppo.py:45-46), or None when that is every row (no gather copies)."""
        ind = exps.nonzero().squeeze(1)
        return (None if ind.shape[0] == n else ind), ind.shape[0]

    def _surrogate(self, logp, adv, fixed, n_exp):
        ratio = torch.exp(logp - fixed)
        clipped = torch.clamp(ratio, 1.0 - self.clip_epsilon, 1.0 + self.clip_epsilon) * adv
        return -torch.min(ratio * adv, clipped).sum() / n_exp

    def _policy_head(self, states, actions, ind, fused):
        """The policy's half of `_epoch_forward`: the action mean (`fused`) or the log-probabilities of the rows `ind`."""
        x = self.trans_policy(states)
        if ind is not None:
            x = x[ind]
        if fused:
            return self._policy_mean(x)
        return self.cn.policy_net.get_log_prob(x, actions if ind is None else actions[ind])

    def _epoch_forward(self, states, actions, ind, fused):
        """One epoch's forward pass -> (pred, head): both video contexts (grouped where the nets allow it), the critic's
        values of every row, and of the rows `ind` the policy's action mean when the loss kernel runs (`fused`: it forms
        the log-probabilities itself), else their log-probabilities."""
        self._group_contexts(states)
        pred = self.cn.value_net(self.trans_value(states))
        return pred, self._policy_head(states, actions, ind, fused)

    def update_policy(self, states, actions, returns, advantages, exps, first_pass=None, counts=None):
        """`first_pass` = (pred, head, ind) of a forward pass ALREADY made with the current weights and autograd on
        (AgentEgo.update_params): it served as the no-grad value / fixed-log-prob pass and now is epoch 0's forward --
        the weights have not moved in between, so the numbers are the reference's, with two forward passes fewer.
        `head` is the policy's action mean when the fused loss kernel runs (`_fused_losses`), else its log-probabilities.
        `counts` = (global rows, global exploration rows) when the caller has exchanged them already."""
        if self.use_mini_batch:
            return self._update_policy_minibatch(states, actions, returns, advantages, exps)
        fused = self._fused_losses()
        if first_pass is None:
            ind, n_ind = self._exploration_rows(exps, states.shape[0])
        else:
            ind = first_pass[2]
            n_ind = states.shape[0] if ind is None else ind.shape[0]
        if counts is None:
            n_val = D.global_count(states.shape[0], states.device)
            n_exp = D.global_count(n_ind, states.device)
        else:
            n_val, n_exp = counts
        if fused:
            return self._update_policy_fused(states, actions, returns, advantages, ind, n_ind, n_val, n_exp, first_pass)
        if self.value_opt_niter != 1:
            raise NotImplementedError("value_opt_niter != 1 is not on the ego_mimic path")
        if first_pass is None:
            with to_test(*self.update_modules):
                with torch.no_grad():
                    fixed = self._policy_head(states, actions, None, False)
            fixed = fixed if ind is None else fixed[ind]
        else:
            fixed = first_pass[1].detach()
        adv = advantages if ind is None else advantages[ind]
        losses = []
        mon, gated = self._monitor_on(), self._monitor_gated()
        recs, figs, reason = [], [], None
        for epoch in range(self.opt_num_epochs):
            # critic and actor have disjoint parameters: one backward over the sum of the two losses yields exactly the two
            # separate gradients, before the single gradient exchange; the value step precedes the policy step as in the
            # reference. (Running two backward passes on two HIP streams was faster and hung the GPU intermittently --
            # concurrent library GEMMs, docs/DESIGN_TRAIL.md section 2.)
            pred, logp = first_pass[:2] if first_pass is not None and epoch == 0 else self._epoch_forward(states, actions, ind, False)
            v_loss = (pred - returns).pow(2).sum() / n_val
            s_loss = self._surrogate(logp, adv, fixed, n_exp)
            if mon:
                recs.append(O.ppo_stats_torch(pred.detach(), returns, None, None, getattr(self.cn.policy_net, "action_log_std", None), advantages,
                                              fixed, self.clip_epsilon, rows=ind, logp=logp.detach()))
                if gated:
                    fig, reason = self._monitor_gate(recs[-1])
                    figs.append(fig)
                    if reason is not None:
                        break
            self._zero_grads()
            (v_loss + s_loss).backward()
            self._optim_step()
            losses.append((v_loss.detach(), s_loss.detach()))
        self.update_stats = {"value_loss": [float(v) for v, _ in losses], "surr_loss": [float(s) for _, s in losses]}
        if mon:
            if not gated and recs:
                by_rank = self._gather_records(torch.stack(recs))
                figs = [O.stats_summary([r[e] for r in by_rank]) for e in range(len(recs))]
            self._monitor_publish(self.update_stats, figs, len(losses), reason)

    # -- shuffled mini-batch epochs (agents/agent_ppo.py:24-44) ----------------------------------------
    def _update_policy_minibatch(self, states, actions, returns, advantages, exps):
        """Every epoch shuffles the batch (NumPy's global generator, as the reference: a run seeded like the reference's shuffles
        identically) and takes one value step and one policy step per window of `opt_batch_size` rows; the last window may be
        short. Two forms: the fused one (`_fused_losses`: float32 on the GPU, Gaussian head) keeps the whole update on the
        device; the plain one is the reference's formulation in torch ops, on any device and dtype."""
        if D.world_size() > 1:
            raise RuntimeError("AgentPPO(use_mini_batch=True) runs on one rank: with %d ranks the number of rows, and so the number of "
                               "optimizer steps per epoch, differs between ranks and the gradient exchange would not line up "
                               "(use the full-batch update for multi-GPU runs)" % D.world_size())
        with to_test(*self.update_modules):
            with torch.no_grad():
                fixed_log_probs = self.cn.policy_net.get_log_prob(self.trans_policy(states), actions)
        n, batch = states.shape[0], int(self.opt_batch_size)
        n_iter = int(math.ceil(n / batch))
        if self._fused_losses() and 1 <= batch <= O.L.PPO_LOSS_MB_MAX_ROWS and n > 0:
            return self._update_policy_minibatch_fused(states, actions, returns, advantages, fixed_log_probs, exps, batch, n_iter)
        cols = (states, actions, returns, advantages, fixed_log_probs, exps)
        v_losses, s_losses = [], []
        for _ in range(self.opt_num_epochs):
            perm = np.arange(n)
            np.random.shuffle(perm)
            perm = torch.from_numpy(perm).to(states.device)
            cols = tuple(c[perm] for c in cols)              # (the reference permutes the already permuted columns)
            for i in range(n_iter):
                states_b, actions_b, returns_b, advantages_b, fixed_b, exps_b = (c[i * batch:min((i + 1) * batch, n)] for c in cols)
                ind = exps_b.nonzero().squeeze(1)
                for _ in range(self.value_opt_niter):
                    self._zero_grads()
                    pred = self.cn.value_net(self.trans_value(states_b))
                    v_loss = (pred - returns_b).pow(2).mean()
                    v_loss.backward()
                    self._optim_step(which=(0,))
                s_loss = self.ppo_loss(states_b, actions_b, advantages_b, fixed_b, ind)
                self._zero_grads()
                s_loss.backward()
                self._optim_step(which=(1,))
                v_losses.append(v_loss.detach())
                s_losses.append(s_loss.detach())
        self.update_stats = {"value_loss": [float(v) for v in v_losses], "surr_loss": [float(s) for s in s_losses]}

    def _update_policy_minibatch_fused(self, states, actions, returns, advantages, fixed_log_probs, exps, batch, n_iter):
        """One optim.minibatch_plan per epoch (the permuted columns and every window's exploration-row count, left on the device),
        then per window: both nets on slice views of the plan's buffers, ONE optim.ppo_losses_mb (rows with exps == 0 masked
        instead of gathered away: no nonzero(), no shape that depends on the data), autograd from (values, action mean), and one
        fused step -- critic and actor have disjoint parameters, so the value step and the policy step share it. The host reads
        nothing between the first plan and the losses after the last epoch."""
        dev = states.device
        n, A = states.shape[0], actions.shape[1]
        log_std = self.cn.policy_net.action_log_std
        learn_std = bool(log_std.requires_grad)
        src = [states if states.stride(1) == 1 else states.contiguous(), actions if actions.stride(1) == 1 else actions.contiguous()] + \
              [c.reshape(-1).contiguous() for c in (returns, advantages, fixed_log_probs, exps)]
        buf = [torch.empty(c.shape, dtype=torch.float32, device=dev) for c in src]
        counts = torch.empty(n_iter, dtype=torch.int32, device=dev)
        rec = torch.zeros(max(1, self.opt_num_epochs), n_iter, 2, dtype=torch.float64, device=dev)
        d_pred = torch.empty(batch, 1, dtype=torch.float32, device=dev)
        d_mean = torch.empty(batch, A, dtype=torch.float32, device=dev)
        states_p, actions_p, returns_p, adv_p, fixed_p, exps_p = buf
        cur = np.arange(n)
        for epoch in range(self.opt_num_epochs):
            perm = np.arange(n)
            np.random.shuffle(perm)
            cur = cur[perm]                                  # the reference permutes the permuted columns: compose, gather from the originals
            O.minibatch_plan(*src, torch.from_numpy(cur).to(dev), batch, out=buf, mb_n_exp=counts)
            for i in range(n_iter):
                lo, hi = i * batch, min((i + 1) * batch, n)
                pred = self.cn.value_net(self.trans_value(states_p[lo:hi]))
                mean = self._policy_mean(self.trans_policy(states_p[lo:hi]))
                self._zero_grads()
                _, _, _, d_ls = O.ppo_losses_mb(pred.detach(), returns_p[lo:hi], mean.detach(), actions_p[lo:hi], log_std.detach(), adv_p[lo:hi],
                                                fixed_p[lo:hi], exps_p[lo:hi], counts[i:i + 1], self.clip_epsilon, d_pred=d_pred[:hi - lo],
                                                d_mean=d_mean[:hi - lo], want_d_log_std=learn_std, losses_out=rec[epoch, i])
                torch.autograd.backward([pred, mean], [d_pred[:hi - lo], d_mean[:hi - lo]])
                if learn_std:
                    log_std.grad = d_ls.view_as(log_std)
                self._optim_step()
        self._epochs_enqueued()
        host = rec[:self.opt_num_epochs].reshape(-1, 2).tolist()
        self.update_stats = {"value_loss": [r[0] for r in host], "surr_loss": [r[1] for r in host]}

    def _policy_mean(self, x):
        return self.cn.policy_net.mean_std(x)[0]

    def _epochs_enqueued(self):
        """Hook: every launch of the update is on the stream, its results have not been read yet."""
        return

    def _update_policy_fused(self, states, actions, returns, advantages, ind, n_ind, n_val, n_exp, first_pass):
        """The epochs with optim.ppo_losses: forward passes -> ONE launch for both losses and d loss / d (values, action mean)
        -> autograd from those two tensors -> fused exchange / clip / Adam (`_optim_step`). Epoch 0's forward doubles as the
        pass that fixes the sampling policy's log-probabilities (the weights have not moved since the rollout), whether it
        arrives as `first_pass` or is made here -- unless the nets draw dropout masks in train mode (`_dropout_active`): the
        log-probabilities are then fixed by an eval-mode pass of their own, as the reference's `to_test` block does."""
        dev = states.device
        n, A = states.shape[0], actions.shape[1]
        pol = self.cn.policy_net
        log_std = pol.action_log_std
        learn_std = bool(log_std.requires_grad)
        fixed = torch.empty(n_ind, dtype=torch.float32, device=dev)
        d_pred = torch.empty(n, 1, dtype=torch.float32, device=dev)
        d_mean = torch.empty(n_ind, A, dtype=torch.float32, device=dev)
        mon, gated = self._monitor_on(), self._monitor_gated()
        # one row per epoch: both losses and, with the monitor on, the epoch's record behind them (read together at the end)
        rec = torch.zeros(max(1, self.opt_num_epochs), 2 + (len(O.L.PPO_STATS_FIELDS) if mon else 0), dtype=torch.float64, device=dev)
        figs, reason, epochs_run = [], None, 0
        act = actions if actions.stride(1) == 1 else actions.contiguous()
        eval_fixed = first_pass is None and self._dropout_active()
        if eval_fixed:
            with to_test(*self.update_modules):
                with torch.no_grad():
                    mean = self._policy_head(states, actions, ind, True)
            # (only `fixed` is kept of this launch: the value columns are placeholders, epoch 0 rewrites rec[0] and the gradients)
            O.ppo_losses(returns.reshape(-1, 1), returns, mean, act, log_std.detach(), advantages, fixed, True, self.clip_epsilon, n_val, n_exp,
                         rows=ind, d_pred=d_pred, d_mean=d_mean, losses_out=rec[0, :2])
        for epoch in range(self.opt_num_epochs):
            pred, mean = first_pass[:2] if first_pass is not None and epoch == 0 else self._epoch_forward(states, actions, ind, True)
            self._zero_grads()
            _, _, _, d_ls = O.ppo_losses(pred.detach(), returns, mean.detach(), act, log_std.detach(), advantages, fixed, epoch == 0 and not eval_fixed,
                                         self.clip_epsilon, n_val, n_exp, rows=ind, d_pred=d_pred, d_mean=d_mean,
                                         want_d_log_std=learn_std, losses_out=rec[epoch, :2])
            if mon:
                O.ppo_stats(pred.detach(), returns, mean.detach(), act, log_std.detach(), advantages, fixed, self.clip_epsilon, rows=ind,
                            out=rec[epoch, 2:])
                if gated:
                    fig, reason = self._monitor_gate(rec[epoch, 2:])
                    figs.append(fig)
                    if reason is not None:
                        break
            torch.autograd.backward([pred, mean], [d_pred, d_mean])
            if learn_std:
                log_std.grad = d_ls.view_as(log_std)
            self._optim_step()
            epochs_run += 1
        self._epochs_enqueued()              # (the host would only wait from here on: the GPU still works through the epochs)
        host = rec.tolist()
        self.update_stats = {"value_loss": [r[0] for r in host[:epochs_run]], "surr_loss": [r[1] for r in host[:epochs_run]]}
        if mon:
            if not gated and epochs_run:
                by_rank = [[r[2:] for r in host[:epochs_run]]] if D.world_size() == 1 else self._gather_records(rec[:epochs_run, 2:])
                figs = [O.stats_summary([r[e] for r in by_rank]) for e in range(epochs_run)]
            self._monitor_publish(self.update_stats, figs, epochs_run, reason)


def _quat_v3_marker(fn):
    fn.egp_kernel = "quat_v3"
    return fn


class AgentEgo(AgentPPO):

    def __init__(self, policy_vs_net=None, value_vs_net=None, **kwargs):
        super().__init__(use_mini_batch=False, **kwargs)
        self.traj_cls = TrajBatchEgo
        self.policy_vs_net, self.value_vs_net = policy_vs_net, value_vs_net
        self._bind_compute_nets()

    def _master_nets(self):
        return dict(policy_net=self.policy_net, value_net=self.value_net, policy_vs_net=getattr(self, "policy_vs_net", None),
                    value_vs_net=getattr(self, "value_vs_net", None))

    def _bind_compute_nets(self):
        super()._bind_compute_nets()
        if getattr(self.cn, "policy_vs_net", None) is not None:
            self.sample_modules = [self.cn.policy_net, self.cn.policy_vs_net]
            self.update_modules = [self.cn.policy_net, self.cn.value_net, self.cn.policy_vs_net, self.cn.value_vs_net]
            from .nets import VideoStateNet
            # When a head is an MLP on the HIP GEMMs its first layer can gather the context rows and append the state columns
            # itself: the video net is then asked (per call, `lazy_width`) for the parts instead of the concatenation. (That a
            # VideoStateNet output's state columns need no gradient travels as a tag on the tensor it returns.) Nothing is
            # stored on the caller's modules.
            self._lazy_width = {}
            for key, head, vs in (("policy", self.cn.policy_net, self.cn.policy_vs_net), ("value", self.cn.value_net, self.cn.value_vs_net)):
                layers = getattr(getattr(head, "net", None), "affine_layers", None)
                self._lazy_width[key] = int(layers[0].out_features) if (isinstance(vs, VideoStateNet) and layers is not None and len(layers) > 0) else 0

    def _video_net(self):
        return self.cn.policy_vs_net

    prefetch_rollout = True     # set up the next sampling pass behind the update's last epoch (LockstepRollout.prepare)

    def _epochs_enqueued(self):
        """The reference's loop is sample -> update -> sample (ego_pose/ego_mimic.py:106-118): once the update's launches are
        queued, the set-up of the next sampling pass -- host work the GPU does not wait for -- runs while the GPU finishes the
        update. Only with compute nets that ARE the caller's modules (shadow copies are refreshed at `sample`, which would make
        the set-up stale every time) and only when a sampling pass has told us its batch size."""
        ro, mb = self._rollout, getattr(self, "_last_min_batch", None)
        if not self.prefetch_rollout or ro is None or mb is None or self.shadow is not None or D.world_size() > 1:
            return
        with to_test(*self.sample_modules):
            self.pre_sample()
            ro.noise_rate, ro.mean_action = self.noise_rate, self.mean_action
            ro.prepare(mb, end_reward=float(self.env.end_reward))

    def pre_sample(self):
        # ego_pose/core/agent_ego.py:18-19: the video net leaves the update in 'train' mode; every sampling pass starts in 'test'
        self.cn.policy_vs_net.set_mode("test")

    def pre_episode(self):
        self.cn.policy_vs_net.initialize(torch.as_tensor(self.env.get_episode_cnn_feat()))

    def push_memory(self, memory, state, action, mask, next_state, reward, exp):
        memory.push(state, action, mask, next_state, reward, exp, np.array([self.env.expert_ind, self.env.start_ind]))

    def _group_contexts(self, states=None):
        from .nets import grouped_forecast_context, grouped_video_context
        nets = [self.cn.value_vs_net, self.cn.policy_vs_net]
        return grouped_video_context(nets) or grouped_forecast_context(nets, states)

    def trans_policy(self, states):
        w = getattr(self, "_lazy_width", {}).get("policy", 0)
        return self.cn.policy_vs_net(states, lazy_width=w) if w else self.cn.policy_vs_net(states)

    def trans_value(self, states):
        w = getattr(self, "_lazy_width", {}).get("value", 0)
        return self.cn.value_vs_net(states, lazy_width=w) if w else self.cn.value_vs_net(states)

    @staticmethod
    def _v_metas_of(batch):
        v_metas = batch.device_column("v_metas") if hasattr(batch, "device_column") else None
        return v_metas.cpu().numpy() if v_metas is not None else np.asarray(batch.v_metas)

    def _train_context(self, net, masks, v_metas, adopt_from=None):
        """The video net `net` in train mode on this batch (ego_pose/core/agent_ego.py:34-41): the rollout's feature table
        attached when there is one, then the batch's segmentation adopted from `adopt_from` (a net initialised on the same
        batch and table: segment and gather once) or made by `initialize`."""
        ex = self._rollout.experts if self._rollout is not None else None
        if ex is not None and hasattr(net, "attach_feature_table"):
            net.attach_feature_table(ex.cnn_table(masks.device, next(net.parameters()).dtype), ex.cnn_offset)
        net.set_mode("train")
        x_init = (masks, self.env.cnn_feat, v_metas)
        if adopt_from is not None and self.share_train_context and hasattr(net, "adopt_train_context"):
            net.adopt_train_context(adopt_from, x_init)
        else:
            net.initialize(x_init)

    def update_params(self, batch):
        t0 = time.time()
        to_train(*self.update_modules)
        self._params_stepped()
        c = self._load_batch(batch)
        dev = c["states"].device
        v_metas = self._v_metas_of(batch)
        self._train_context(self.cn.policy_vs_net, c["masks"], v_metas)
        self._train_context(self.cn.value_vs_net, c["masks"], v_metas, adopt_from=self.cn.policy_vs_net)
        n_rows = c["states"].shape[0]
        ind, n_ind = self._exploration_rows(c["exps"], n_rows)
        if self.value_opt_niter == 1 and self.reuse_first_pass and not self._dropout_active():
            # ONE forward pass with autograd on serves three purposes: the values that GAE consumes, the fixed log-probs of
            # the surrogate, and epoch 0's forward (nothing has stepped in between, and no net draws dropout masks: with a
            # TCN video net and dropout > 0 a train-mode pass is not the eval-mode one, and the branch below runs instead)
            pred0, head0 = self._epoch_forward(c["states"], c["actions"], ind, self._fused_losses())
            advantages, returns, counts = self._advantages_with_counts(c["rewards"], c["masks"], pred0.detach(), (n_rows, n_ind))
            self.update_policy(c["states"], c["actions"], returns, advantages, c["exps"], first_pass=(pred0, head0, ind), counts=counts)
        else:
            with to_test(*self.update_modules):
                with torch.no_grad():
                    self._group_contexts(c["states"])       # the policy net's context is consumed by update_policy's first pass
                    values = self.cn.value_net(self.trans_value(c["states"]))
            advantages, returns, counts = self._advantages_with_counts(c["rewards"], c["masks"], values, (n_rows, n_ind))
            self.update_policy(c["states"], c["actions"], returns, advantages, c["exps"], counts=counts)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        return time.time() - t0


class AgentVGAIL(AgentEgo):
    """ego_pose/core/agent_vgail.py:7-88: an AgentEgo whose update also trains a discriminator between the learner's
    observations and the expert's, both seen through a video net of the discriminator's own.

    Constructor keywords are the reference's (:9-18) plus three whose defaults give the reference's behaviour:
      discrim_grad_clip      the constant of :70 (clip_grad_norm_ over discrim_net's parameters only)
      expert_obs             "reference": the expert rows as data_process/gen_expert.py:40-43 wrote them -- `qvel` was never set there,
                             so their velocity columns are ZERO and a discriminator separates the classes by those columns alone;
                             "fd": rows derived with the takes' finite-difference velocities (expert.expert_obs_rows)
      discrim_reward_weight  w > 0: rewards <- (1 - w) rewards + w (-log D(vs(s))) on the device before GAE. No reference code reads
                             the discriminator (as written the class trains a net nobody uses); 0 keeps that.

    `update_discriminator` has two forms behind `use_fused_discrim`: the plain one is the reference's loop in torch ops on any
    device and dtype; the fused one (float32 on the GPU, a `nets.Discriminator`, nn.BCELoss with mean reduction, a VideoStateNet,
    no dropout) sweeps the video net ONCE per step -- in train mode its context rows depend on the CNN features only, so the
    reference's two calls (:60-61) compute the same rows twice -- and runs one stacked [generated; expert] block through the MLP."""

    def __init__(self, discrim_net=None, discrim_vs_net=None, discrim_criterion=None, optimizer_discrim=None, discrim_num_update=10,
                 discrim_grad_clip=40.0, expert_obs="reference", discrim_reward_weight=0.0, **kwargs):
        from .expert import OBS_MODES
        if expert_obs not in OBS_MODES:
            raise ValueError("expert_obs must be one of %s, got %r" % (OBS_MODES, expert_obs))
        if getattr(getattr(kwargs.get("env"), "cfg", None), "obs_phase", False):
            raise NotImplementedError("AgentVGAIL with cfg.obs_phase: the phase column depends on the episode, not on the take's frame, "
                                      "so the expert's rows have no such column")
        self.discrim_net, self.discrim_vs_net = discrim_net, discrim_vs_net          # (before the base classes bind the compute nets)
        super().__init__(**kwargs)
        self.discrim_criterion = discrim_criterion
        self.optimizer_discrim = optimizer_discrim
        self.discrim_num_update = discrim_num_update
        self.discrim_grad_clip = discrim_grad_clip
        self.expert_obs = expert_obs
        self.discrim_reward_weight = float(discrim_reward_weight)
        self.use_fused_discrim = True       # A/B handle: one sweep + one stacked block + HIP loss tail per step instead of the reference's loop
        self._discrim_stepper = {}          # the steppers of (optimizer_discrim,), built on first use (`_get_discrim_stepper`)
        self._expert_rows = None            # host rows of every take (expert.expert_obs_rows)
        self._expert_table = {}
        self._gail_batch = None
        self._prefetch_deferred = False
        self.discrim_stats = {}             # discrim_net's gradient norm of the last step, before and after the clip
        self.last_e_loss = None             # what update_params' update_discriminator returned

    def _master_nets(self):
        nets = super()._master_nets()
        nets.update(discrim_net=getattr(self, "discrim_net", None), discrim_vs_net=getattr(self, "discrim_vs_net", None))
        return nets

    def _bind_compute_nets(self):
        super()._bind_compute_nets()
        extra = [m for m in (getattr(self.cn, "discrim_net", None), getattr(self.cn, "discrim_vs_net", None)) if m is not None]
        self.sample_modules = self.sample_modules + extra          # agent_vgail.py:17-18
        self.update_modules = self.update_modules + extra

    def _epochs_enqueued(self):
        # inside update_params the next sampling pass is set up behind the DISCRIMINATOR's last step, not behind the PPO epochs:
        # the set-up puts policy_vs_net into 'test' mode, and discrim_vs_net adopts its train context of this batch first
        if self._gail_batch is not None:
            self._prefetch_deferred = True
            return
        super()._epochs_enqueued()

    def _discrim_enqueued(self):
        """Hook: every launch of the discriminator update is on the stream, its loss has not been read yet."""
        if self._prefetch_deferred:
            self._prefetch_deferred = False
            super()._epochs_enqueued()

    def pre_sample(self):
        super().pre_sample()
        self.cn.discrim_vs_net.set_mode("test")

    def pre_episode(self):
        super().pre_episode()
        self.cn.discrim_vs_net.initialize(torch.as_tensor(self.env.get_episode_cnn_feat()))

    # -- the expert's rows ------------------------------------------------------------------------------
    def _expert_obs_host(self):
        if self._expert_rows is None:
            from .expert import expert_obs_rows
            arr = self.env.expert_arr
            derived = self.expert_obs != "reference" or not all("obs" in e for e in arr)
            obs_dim = getattr(self.env, "obs_dim", None)
            rows = expert_obs_rows(arr, self._kernel_ctx() if derived else None, self.expert_obs, obs_dim)
            self._expert_rows = (rows, np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64))
        return self._expert_rows

    def _expert_obs_table(self, device, dtype):
        key = (str(device), dtype)
        if key not in self._expert_table:
            ex = self._rollout.experts if self._rollout is not None else None
            if ex is not None and ex.expert_arr is self.env.expert_arr:
                tab = ex.obs_table(self._kernel_ctx(), device, dtype, self.expert_obs, getattr(self.env, "obs_dim", None))[0]
            else:
                tab = torch.as_tensor(np.ascontiguousarray(np.concatenate(self._expert_obs_host()[0], 0)), dtype=dtype, device=device)
            self._expert_table[key] = tab
        return self._expert_table[key]

    def _expert_src(self, v_metas, masks):
        """Table row of every sample (agent_vgail.py:77-85): episode e covers rows [start_ind, start_ind + len_e) of take exp_ind."""
        rows, offset = self._expert_obs_host()
        mk = masks.detach().cpu().numpy() if torch.is_tensor(masks) else np.asarray(masks)
        end = np.where(mk.reshape(-1) == 0)[0]
        if end.size == 0 or end[-1] != mk.size - 1:
            raise ValueError("the batch must end with an episode end: the expert's rows are taken per whole episode")
        meta = np.asarray(v_metas)[end, :].astype(np.int64)
        lens = np.diff(np.insert(end, 0, -1))
        e_ind, s_ind = meta[:, 0], meta[:, 1]
        if e_ind.min() < 0 or e_ind.max() >= len(rows):
            raise ValueError("take index out of range: [%d, %d] with %d takes" % (e_ind.min(), e_ind.max(), len(rows)))
        take_len = np.diff(offset)[e_ind]
        bad = (s_ind < 0) | (s_ind + lens > take_len)
        if bad.any():
            k = int(np.nonzero(bad)[0][0])
            raise ValueError("expert rows [%d, %d) leave take %d (%d frames)" % (s_ind[k], s_ind[k] + lens[k], e_ind[k], take_len[k]))
        return np.repeat(offset[e_ind] + s_ind, lens) + (np.arange(mk.size) - np.repeat(np.insert(end[:-1] + 1, 0, 0), lens))

    def get_expert_states(self, v_metas, masks):
        """agent_vgail.py:75-88: the expert's observation of every sample's frame, normalised with the running filter's mean and
        std (no clip), as a tensor of the agent's dtype on its device. A slice that leaves its take raises ValueError (the
        reference's numpy slice would silently come up short)."""
        src = self._expert_src(v_metas, masks)
        expert_states = np.concatenate(self._expert_obs_host()[0], 0)[src]
        if self.running_state is not None:
            rs = self.running_state.rs
            expert_states = (expert_states - rs.mean[None, :]) / rs.std[None, :]
        return torch.from_numpy(np.ascontiguousarray(expert_states)).to(self.dtype).to(self.device)

    # -- the discriminator update -------------------------------------------------------------------
    def _discrim_clip_list(self):
        c = self.discrim_grad_clip
        return [(list(self.discrim_net.parameters()), float(c))] if c is not None and c > 0 else []

    def _clip_discrim_grad(self):
        """agent_vgail.py:70 -> discrim_net's gradient norm before the clip, or None without a clip."""
        c = self.discrim_grad_clip
        return torch.nn.utils.clip_grad_norm_(self.discrim_net.parameters(), c) if c is not None and c > 0 else None

    def _get_discrim_stepper(self, flat=True):
        """The stepper of (optimizer_discrim,). `flat` False: the plain form's, whose optimizer always steps itself (the
        reference's loop in torch ops is what the fused form is measured against)."""
        if flat not in self._discrim_stepper:
            self._discrim_stepper[flat] = self._build_stepper([self.optimizer_discrim], self._discrim_clip_list(),
                                                              {0: self._clip_discrim_grad}, flat)
        return self._discrim_stepper[flat]

    def _get_discrim_updater(self):
        """optim.FlatUpdater of optimizer_discrim, or None (as `_get_updater`)."""
        up = self._get_discrim_stepper()
        return up if isinstance(up, O.FlatUpdater) else None

    def _fused_discrim(self):
        from .nets import Discriminator, VideoStateNet
        dn, vs, crit = self.cn.discrim_net, self.cn.discrim_vs_net, self.discrim_criterion
        return (self.use_fused_discrim and torch.device(self.device).type == "cuda" and self.cdtype == torch.float32
                and isinstance(dn, Discriminator) and all(p.dtype == torch.float32 for p in dn.parameters())
                and type(crit) is torch.nn.BCELoss and crit.reduction == "mean" and crit.weight is None
                and isinstance(vs, VideoStateNet) and not self._dropout_active())

    def _init_discrim_context(self, masks, v_metas, adopt):
        """discrim_vs_net in train mode on this batch (agent_vgail.py:56-57); inside update_params it adopts the policy net's
        segmentation of the same batch instead of repeating it."""
        self._train_context(self.cn.discrim_vs_net, masks, v_metas, adopt_from=self.cn.policy_vs_net if adopt else None)

    def update_discriminator(self, states, masks, v_metas, _adopt=False):
        """perform discriminator update (agent_vgail.py:54-73) -> e_loss, the last step's expert loss, as a float."""
        to_train(self.cn.discrim_net, self.cn.discrim_vs_net)
        self._params_stepped()              # (a call of its own, after a checkpoint load: the compute copies follow the caller's modules)
        dev = torch.device(self.device)
        states, masks = states.to(dev).to(self.cdtype), masks.to(dev).to(self.cdtype)
        v_metas = np.asarray(v_metas.cpu() if torch.is_tensor(v_metas) else v_metas)
        src_host = self._expert_src(v_metas, masks)         # (first: a slice that leaves its take is reported as such)
        self._init_discrim_context(masks, v_metas, _adopt)
        vs = self.cn.discrim_vs_net
        if self._fused_discrim() and vs._gather_unique and states.shape[0] > 0:
            return self._update_discriminator_fused(states, src_host)
        return self._update_discriminator_plain(states, masks, v_metas)

    def _update_discriminator_plain(self, states, masks, v_metas):
        dev = states.device
        expert_states = self.get_expert_states(v_metas, masks).to(self.cdtype)
        vs, dn, crit = self.cn.discrim_vs_net, self.cn.discrim_net, self.discrim_criterion
        n = states.shape[0]
        multi = D.world_size() > 1
        share = n / D.global_count(n, dev) if multi else None          # mean over this rank's rows -> its share of the global mean
        up = self._get_discrim_stepper(flat=False)
        l_e = None
        for _ in range(self.discrim_num_update):
            g_vs_out = vs(states)
            e_vs_out = vs(expert_states)
            g_o = dn(g_vs_out)
            e_o = dn(e_vs_out)
            up.zero_grad()
            l_g = crit(g_o, torch.ones((g_o.size(0), 1), dtype=g_o.dtype, device=dev))
            l_e = crit(e_o, torch.zeros((e_o.size(0), 1), dtype=e_o.dtype, device=dev))
            if multi:
                l_g, l_e = l_g * share, l_e * share
            discrim_loss = l_g + l_e
            discrim_loss.backward()
            up.collect_grads()
            up.all_reduce()
            up.step()
        self._discrim_enqueued()
        if l_e is None:
            return 0.0
        l_e = l_e.detach().double()
        if multi:
            l_e = l_e.to(D._comm_device(dev))
            torch.distributed.all_reduce(l_e)
            D._note()
        self._record_discrim_norm(up)
        return l_e.item()

    def _record_discrim_norm(self, up):
        """discrim_stats: discrim_net's gradient norm of the last step, before and after the clip (read once, after the last
        step is queued)."""
        norm = up.grad_norm(1)
        if norm is None:
            self.discrim_stats = {}
            return
        norm = float(norm)
        self.discrim_stats = {"grad_norm": norm, "clipped_norm": norm * min(1.0, float(self.discrim_grad_clip) / (norm + 1e-6))}

    def _update_discriminator_fused(self, states, src_host):
        """Per step: ONE sweep of discrim_vs_net -> optim.gail_rows (the [generated; expert] block from the context rows, the
        states and the expert table) -> Discriminator.logits on the 2n rows -> optim.bce_logits (both losses, d loss / d logits)
        -> autograd from (logits, dz) through the MLP and GailRows into the sweep -> clip + Adam (FlatUpdater; the clip group
        holds discrim_net's parameters only, :70). The host reads nothing until the last step is queued."""
        from .nets import grouped_video_context
        dev = states.device
        vs, dn = self.cn.discrim_vs_net, self.cn.discrim_net
        n = states.shape[0]
        src = torch.as_tensor(src_host, dtype=torch.int64, device=dev)
        tab = self._expert_obs_table(dev, torch.float32)
        mean = inv_std = None
        if self.running_state is not None:
            rs = self.running_state.rs
            mean = torch.as_tensor(np.asarray(rs.mean, np.float64), dtype=torch.float32, device=dev).contiguous()
            inv_std = torch.as_tensor(1.0 / np.asarray(rs.std, np.float64), dtype=torch.float32, device=dev).contiguous()
        x = states if states.stride(1) == 1 else states.contiguous()
        n_glob = D.global_count(n, dev)
        up = self._get_discrim_stepper()
        steps = int(self.discrim_num_update)
        rec = torch.zeros(max(1, steps), 2, dtype=torch.float64, device=dev)
        dz = torch.empty(2 * n, 1, dtype=torch.float32, device=dev)
        for step in range(steps):
            grouped_video_context([vs])                     # (a bi-LSTM's two directions in one grouped launch; else the net runs itself)
            ctx2d = vs.context_rows().contiguous()
            X = O.GailRows.apply(ctx2d, vs._gather_tm, x, tab, src, mean, inv_std)
            X._egp_ctx_cols = vs.v_hdim                     # the trailing columns are data: no input gradient needed there
            z = dn.logits(X)
            up.zero_grad()
            O.bce_logits(z.detach(), n_glob, n_glob, dz=dz, losses_out=rec[step])
            torch.autograd.backward([z], [dz])
            up.collect_grads()
            up.all_reduce()
            up.step()
        self._discrim_enqueued()
        if steps < 1:
            return 0.0
        e_loss = rec[steps - 1, 1]
        if D.world_size() > 1:
            e_loss = e_loss.to(D._comm_device(dev))
            torch.distributed.all_reduce(e_loss)
            D._note()
        self._record_discrim_norm(up)
        return e_loss.item()

    # -- the discriminator as a reward ----------------------------------------------------------------
    def discriminator_scores(self, batch):
        """-log D(vs(s)) of every row of the batch from one no-grad pass of the current discriminator, on the device. D is trained
        towards 1 on generated rows (agent_vgail.py:66-67), so a row the discriminator takes for the expert's scores high."""
        c = self._cols if self._gail_batch is batch and getattr(self, "_cols", None) is not None else self._load_batch(batch)
        v_metas = self._v_metas_of(batch)
        vs, dn = self.cn.discrim_vs_net, self.cn.discrim_net
        with to_test(dn, vs):
            with torch.no_grad():
                self._init_discrim_context(c["masks"], v_metas, adopt=self._gail_batch is batch)
                x = vs(c["states"])
                if hasattr(dn, "logits"):
                    z = dn.logits(x)
                    if z.is_cuda and z.dtype == torch.float32:
                        return O.bce_scores(z)
                    return torch.nn.functional.softplus(-z).reshape(-1)
                return -torch.log(dn(x)).reshape(-1)

    def _load_batch(self, batch):
        self._cols = super()._load_batch(batch)
        return self._cols

    def _advantages_with_counts(self, rewards, masks, values, counts):
        w = self.discrim_reward_weight
        if w > 0 and self._gail_batch is not None:
            rewards = (1.0 - w) * rewards + w * self.discriminator_scores(self._gail_batch).to(rewards.dtype)
        return super()._advantages_with_counts(rewards, masks, values, counts)

    def update_params(self, batch):
        """AgentEgo.update_params followed by update_discriminator (agent_vgail.py:28-52); the returned time covers both."""
        t0 = time.time()
        self._gail_batch, self._cols = batch, None
        try:
            super().update_params(batch)
            c = self._cols if self._cols is not None else self._load_batch(batch)
            self.last_e_loss = self.update_discriminator(c["states"], c["masks"], self._v_metas_of(batch), _adopt=True)
        finally:
            self._gail_batch, self._cols, self._prefetch_deferred = None, None, False
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize(torch.device(self.device))
        return time.time() - t0
