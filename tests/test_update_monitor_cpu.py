"""The PPO update monitor on the plain path (CPU, float64): AgentPPO(target_kl, update_diagnostics, stop_on_nonfinite) over
optim.ppo_stats_torch / optim.stats_summary -- off means off, diagnostics do not move the update, every figure against a
statement written here from the per-epoch policy outputs, the KL stop and the non-finite stop leave exactly the state of the
previous epoch, and two gloo ranks decide together from the global figures. The GAE kernel is HIP-only: the oracle's GAE
stands in for K5, as in test_agent_update_cpu.py."""
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from conftest import load_golden                                           # noqa: E402
import minibatch_fixture as MB                                             # noqa: E402
import update_fixture as UF                                                # noqa: E402
import vgail_fixture as VG                                                 # noqa: E402
from egopose_amd import optim as O                                         # noqa: E402
from oracle.gae import estimate_advantages as oracle_gae                   # noqa: E402

FIXTURE = "ppo_update.npz"
LR_POLICY = 5e-3            # the fixture's own policy_lr: KL_0 == 0 < KL_1 < KL_2 with it (asserted in the KL-stop test)
FIGURES = ("approx_kl", "approx_kl_k1", "clip_frac", "ratio_min", "ratio_max", "explained_var", "entropy", "nonfinite_rows")


@pytest.fixture(autouse=True)
def _float64_default():
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


def _oracle_gae(agent, poison=None):
    """The oracle's GAE in K5's place; `poison(adv, exps)` may edit the advantages before the update sees them."""
    def adv_fn(rewards, masks, values):
        a, r, _ = oracle_gae(rewards.cpu().numpy(), masks.cpu().numpy(), values.cpu().numpy(), agent.gamma, agent.tau)
        a = np.array(a, np.float64)
        if poison is not None:
            poison(a)
        agent._seen = (a.copy(), np.array(r, np.float64))
        return torch.as_tensor(a, device=rewards.device), torch.as_tensor(r, device=rewards.device)
    agent._advantages = adv_fn
    return agent


def _agent(g, epochs=None, poison=None, **monitor):
    agent, mods = UF.build_agent(g)
    for group in agent.optimizer_policy.param_groups:
        group["lr"] = LR_POLICY
    if epochs is not None:
        agent.opt_num_epochs = epochs
    for k, v in monitor.items():
        assert hasattr(agent, k), k
        setattr(agent, k, v)
    return _oracle_gae(agent, poison), mods


def _state(mods):
    return {"%s.%s" % (n, k): v.detach().clone() for n, m in mods.items() for k, v in m.state_dict().items()}


def _optimizer_state(agent):
    out = {}
    for name, opt in (("policy", agent.optimizer_policy), ("value", agent.optimizer_value)):
        for gi, group in enumerate(opt.param_groups):
            for pi, p in enumerate(group["params"]):
                st = opt.state.get(p, {})
                for k in ("exp_avg", "exp_avg_sq", "step"):
                    if k in st:
                        out["%s.%d.%d.%s" % (name, gi, pi, k)] = torch.as_tensor(st[k]).detach().clone()
    return out


def _assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _run(g, **kw):
    agent, mods = _agent(g, **kw)
    agent.update_params(UF.batch_of(g))
    return agent, mods


def test_off_means_off(monkeypatch):
    calls = []
    for name in ("ppo_stats", "ppo_stats_torch"):
        inner = getattr(O, name)
        monkeypatch.setattr(O, name, lambda *a, _inner=inner, _name=name, **k: (calls.append(_name), _inner(*a, **k))[1])
    g = load_golden(FIXTURE)
    agent, _ = _run(g)
    assert calls == []
    assert set(agent.update_stats) == {"value_loss", "surr_loss"}
    assert (agent.target_kl, agent.update_diagnostics, agent.stop_on_nonfinite) == (None, False, False)
    agent, _ = _run(g, update_diagnostics=True)
    assert calls == ["ppo_stats_torch"] * agent.opt_num_epochs          # (the stub does count when the monitor is on)


@pytest.mark.parametrize("monitor", [dict(update_diagnostics=True), dict(target_kl=float("inf")), dict(stop_on_nonfinite=True)])
def test_monitor_does_not_move_the_update(monitor):
    g = load_golden(FIXTURE)
    off, off_mods = _run(g)
    on, on_mods = _run(g, **monitor)
    _assert_same_bits(_state(off_mods), _state(on_mods))
    _assert_same_bits(_optimizer_state(off), _optimizer_state(on))
    assert on.update_stats["value_loss"] == off.update_stats["value_loss"] and on.update_stats["surr_loss"] == off.update_stats["surr_loss"]
    assert on.update_stats["epochs_run"] == off.opt_num_epochs and on.update_stats["stop_reason"] is None and on.update_stats["stop_figures"] is None
    for k in FIGURES:
        assert len(on.update_stats[k]) == off.opt_num_epochs, k


def _spy_forward(agent):
    """Keep (values, log-probabilities) of every epoch's forward pass (epoch 0's is the pass that fixes the log-probabilities)."""
    seen, inner = [], agent._epoch_forward

    def forward(states, actions, ind, fused):
        pred, logp = inner(states, actions, ind, fused)
        assert not fused
        # the reference's formula on its own: DiagGaussian.log_prob of the rows `ind`
        x = agent.trans_policy(states)
        x, a = (x, actions) if ind is None else (x[ind], actions[ind])
        with torch.no_grad():
            ref_logp = agent.cn.policy_net(x).log_prob(a)
        assert torch.equal(ref_logp, logp.detach())
        seen.append((pred.detach().clone().reshape(-1).numpy(), ref_logp.clone().reshape(-1).numpy()))
        return pred, logp
    agent._epoch_forward = forward
    return seen


def test_diagnostics_equal_the_definitions():
    g = load_golden(FIXTURE)
    agent, mods = _agent(g, update_diagnostics=True)
    seen = _spy_forward(agent)
    agent.update_params(UF.batch_of(g))
    st = agent.update_stats
    E = agent.opt_num_epochs
    assert st["epochs_run"] == E == len(seen) and E >= 3
    adv, ret = (np.asarray(x, np.float64).reshape(-1) for x in agent._seen)
    exps = np.asarray(g["exps"]).reshape(-1)
    assert 0 < exps.sum() < exps.size                                   # a strict subset explores: `rows` matters
    eps = agent.clip_epsilon
    log_std = mods["p"].action_log_std.detach().numpy().reshape(-1)
    entropy = float(torch.distributions.Normal(torch.zeros(log_std.size), torch.as_tensor(np.exp(log_std))).entropy().sum())
    fixed = seen[0][1]
    for e, (pred, logp) in enumerate(seen):
        lr = logp - fixed
        r = np.exp(lr)
        d = ret - pred
        want = dict(approx_kl=np.mean(np.expm1(lr) - lr), approx_kl_k1=np.mean(-lr), clip_frac=np.mean(np.abs(r - 1.0) > eps), ratio_min=r.min(),
                    ratio_max=r.max(), explained_var=1.0 - np.var(d) / np.var(ret), entropy=entropy, nonfinite_rows=0)
        for k in FIGURES:
            np.testing.assert_allclose(st[k][e], want[k], rtol=1e-10, atol=0, err_msg="%s, epoch %d" % (k, e))
    assert st["approx_kl"][0] == 0.0 and st["approx_kl_k1"][0] == 0.0 and st["clip_frac"][0] == 0.0
    assert st["ratio_min"][0] == st["ratio_max"][0] == 1.0
    assert st["nonfinite_rows"] == [0] * E and all(isinstance(v, int) for v in st["nonfinite_rows"])


def _kl_target(g):
    """Diagnostics only -> (KL per epoch, a target between KL_1 and KL_2). The fixture must show KL_0 == 0 < KL_1 < KL_2."""
    agent, _ = _run(g, update_diagnostics=True)
    kl = agent.update_stats["approx_kl"]
    assert len(kl) >= 3 and kl[0] == 0.0 and 0.0 < kl[1] < kl[2], kl
    return kl, 0.5 * (kl[1] + kl[2])


def test_kl_stop_leaves_the_state_of_the_previous_epoch():
    g = load_golden(FIXTURE)
    kl, target = _kl_target(g)
    stopped, s_mods = _run(g, target_kl=target)
    st = stopped.update_stats
    assert st["stop_reason"] == "kl" and st["epochs_run"] == 2 and stopped.opt_num_epochs >= 3
    assert st["approx_kl"] == kl[:2] and st["stop_figures"]["approx_kl"] == kl[2] > target
    assert len(st["value_loss"]) == len(st["surr_loss"]) == 2
    two, t_mods = _run(g, epochs=2)
    assert set(two.update_stats) == {"value_loss", "surr_loss"}
    _assert_same_bits(_state(s_mods), _state(t_mods))
    so, to = _optimizer_state(stopped), _optimizer_state(two)
    assert any(k.endswith("exp_avg") for k in so) and any(k.endswith("step") for k in so)
    _assert_same_bits(so, to)
    assert all(float(v) == 2.0 for k, v in so.items() if k.endswith("step"))
    assert st["value_loss"] == two.update_stats["value_loss"] and st["surr_loss"] == two.update_stats["surr_loss"]


def _poison_exploration_row(g, explore=True):
    exps = np.asarray(g["exps"]).reshape(-1)
    row = int(np.nonzero(exps == (1 if explore else 0))[0][1])

    def poison(adv):
        adv.reshape(-1)[row] = np.nan
    return poison


def test_nonfinite_stop_takes_no_step():
    g = load_golden(FIXTURE)
    agent, mods = _agent(g, poison=_poison_exploration_row(g), stop_on_nonfinite=True)
    before = _state(mods)
    agent.update_params(UF.batch_of(g))
    st = agent.update_stats
    assert st["stop_reason"] == "nonfinite" and st["epochs_run"] == 0 and st["stop_figures"]["nonfinite_rows"] == 1
    assert st["value_loss"] == [] and st["approx_kl"] == []
    _assert_same_bits(before, _state(mods))
    assert all(torch.isfinite(v).all() for v in before.values())
    assert _optimizer_state(agent) == {}                                 # no optimizer state was ever created
    # a NaN advantage on a row that does not explore is no input of the surrogate: not counted, no stop
    agent, _ = _run(g, poison=_poison_exploration_row(g, explore=False), stop_on_nonfinite=True)
    assert agent.update_stats["stop_reason"] is None and agent.update_stats["nonfinite_rows"] == [0] * agent.opt_num_epochs
    # without the option the update runs as it always did: every epoch, NaN into the policy's parameters
    agent, mods = _run(g, poison=_poison_exploration_row(g))
    assert set(agent.update_stats) == {"value_loss", "surr_loss"} and len(agent.update_stats["surr_loss"]) == agent.opt_num_epochs
    assert math.isnan(agent.update_stats["surr_loss"][0])
    assert not all(torch.isfinite(v).all() for v in _state(mods).values())
    # diagnostics alone count the row and go on
    agent, _ = _run(g, poison=_poison_exploration_row(g), update_diagnostics=True)
    assert agent.update_stats["stop_reason"] is None and agent.update_stats["nonfinite_rows"][0] == 1


def test_without_exploration_rows_the_kl_never_stops():
    g = load_golden(FIXTURE)
    h = {k: g[k] for k in g.files}
    h["exps"] = np.zeros_like(g["exps"])
    agent, mods = UF.build_agent(g)
    agent.target_kl = 0.0
    _oracle_gae(agent).update_params(UF.batch_of(_Npz(h)))
    st = agent.update_stats
    assert st["stop_reason"] is None and st["epochs_run"] == agent.opt_num_epochs
    assert all(math.isnan(v) for v in st["approx_kl"]) and all(math.isnan(v) for v in st["clip_frac"])
    assert st["ratio_min"] == [math.inf] * agent.opt_num_epochs and st["ratio_max"] == [-math.inf] * agent.opt_num_epochs
    assert all(math.isfinite(v) for v in st["explained_var"])


class _Npz(dict):
    @property
    def files(self):
        return list(self)


@pytest.mark.parametrize("monitor", [dict(target_kl=0.02), dict(update_diagnostics=True), dict(stop_on_nonfinite=True)])
def test_mini_batch_updates_refuse_the_monitor(monitor):
    g = load_golden(MB.FIXTURES[0])
    with pytest.raises(ValueError, match="use_mini_batch"):
        MB.build_agent(g, **monitor)
    agent, _ = MB.build_agent(g, use_mini_batch=False, **monitor)        # the same agent with full-batch epochs takes it
    assert agent._monitor_on()
    with pytest.raises(ValueError, match="target_kl"):
        MB.build_agent(g, use_mini_batch=False, target_kl=-1.0)


def test_stats_summary_combines_ranks_and_handles_empty_sets():
    I = O.L.PPO_STATS
    assert len(I) == 13 and O.STATS_KEYS == FIGURES
    a, b = [0.0] * 13, [0.0] * 13
    a[I["n_pol"]], a[I["k3"]], a[I["k1"]], a[I["clipped"]], a[I["ratio_min"]], a[I["ratio_max"]] = 4.0, 0.4, -0.2, 1.0, 0.5, 1.5
    b[I["n_pol"]], b[I["k3"]], b[I["k1"]], b[I["clipped"]], b[I["ratio_min"]], b[I["ratio_max"]] = 0.0, 0.0, 0.0, 0.0, math.inf, -math.inf
    for r, (n, sy, syy, sd, sdd) in ((a, (2.0, 3.0, 5.0, 1.0, 1.0)), (b, (2.0, 7.0, 25.0, 1.0, 0.5))):
        r[I["n"]], r[I["sum_y"]], r[I["sum_yy"]], r[I["sum_d"]], r[I["sum_dd"]] = n, sy, syy, sd, sdd
    a[I["entropy"]] = b[I["entropy"]] = 2.5
    b[I["nonfinite"]] = 2.0
    s = O.stats_summary([a, b])
    assert s == O.stats_summary(torch.tensor([a, b]))
    assert (s["approx_kl"], s["approx_kl_k1"], s["clip_frac"], s["ratio_min"], s["ratio_max"]) == (0.1, -0.05, 0.25, 0.5, 1.5)
    assert s["explained_var"] == 1.0 - (1.5 / 4 - 0.25) / (30.0 / 4 - 6.25) and s["entropy"] == 2.5 and s["nonfinite_rows"] == 2
    one = O.stats_summary(b)
    assert math.isnan(one["approx_kl"]) and math.isnan(one["clip_frac"]) and one["ratio_min"] == math.inf
    empty = O.stats_summary([0.0] * 13)
    assert math.isnan(empty["explained_var"]) and math.isnan(empty["approx_kl"])


def test_vgail_with_target_kl_still_trains_its_discriminator():
    g = load_golden(VG.FIXTURES[0])
    batch = VG.ppo_batch(g)
    agent, mods = VG.build_agent(g, update_diagnostics=True, opt_num_epochs=3)
    for group in agent.optimizer_policy.param_groups:
        group["lr"] = 2e-2
    _oracle_gae(agent).update_params(batch)
    kl = agent.update_stats["approx_kl"]
    assert kl[0] == 0.0 < kl[1], kl
    agent, mods = VG.build_agent(g, target_kl=0.5 * kl[1], opt_num_epochs=3)
    for group in agent.optimizer_policy.param_groups:
        group["lr"] = 2e-2
    before = _state(mods)
    _oracle_gae(agent).update_params(batch)
    assert agent.update_stats["stop_reason"] == "kl" and agent.update_stats["epochs_run"] == 1
    after = _state(mods)
    assert agent.last_e_loss is not None and math.isfinite(agent.last_e_loss)
    assert any(not torch.equal(before[k], after[k]) for k in before)     # the discriminator's nets moved
    steps = [float(st["step"]) for st in agent.optimizer_discrim.state.values()]
    assert steps and all(s == float(agent.discrim_num_update) for s in steps)


def test_cli_flags_and_trainer_argument_reach_the_agent(monkeypatch):
    from egopose_amd import train
    ap = train.build_parser()
    assert train.monitor_from_args(ap.parse_args([])) is None
    args = ap.parse_args(["--target-kl", "0.03", "--diagnostics", "--stop-on-nonfinite"])
    monitor = train.monitor_from_args(args)
    assert monitor == dict(target_kl=0.03, update_diagnostics=True, stop_on_nonfinite=True)
    assert train.monitor_from_args(ap.parse_args(["--target-kl", "0.5"])) == dict(target_kl=0.5)
    with pytest.raises(ValueError, match="unknown keys"):
        train.monitor_keywords(dict(target_kI=0.1))
    # Trainer hands the dict to the agent it builds (captured at the constructor: no environment, no rollout)
    seen = {}

    class Stop(Exception):
        pass

    def capture(**kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(train, "AgentEgo", capture)
    monkeypatch.setattr(train, "HumanoidEnv", lambda cfg: _StubEnv())
    cfg = _stub_cfg()
    with pytest.raises(Stop):
        train.Trainer(cfg, "cpu", torch.float64, num_envs=2, num_threads=1, num_groups=1, monitor=monitor)
    assert {k: seen[k] for k in monitor} == monitor
    seen.clear()
    with pytest.raises(Stop):
        train.Trainer(cfg, "cpu", torch.float64, num_envs=2, num_threads=1, num_groups=1)
    assert not set(seen) & set(train.MONITOR_KEYS)
    # the log line's fields
    assert train.monitor_log_fields({"value_loss": [1.0], "surr_loss": [0.1]}) == []
    st = {k: [0.0, 0.25] for k in FIGURES}
    st.update(epochs_run=2, stop_reason=None)
    assert train.monitor_log_fields(st) == [("approx_kl", 0.25), ("clip_frac", 0.25), ("explained_var", 0.25), ("entropy", 0.25), ("epochs_run", 2)]


class _StubEnv:
    """What Trainer.__init__ asks of the environment before it builds the agent."""
    import types as _t
    observation_space = _t.SimpleNamespace(shape=(7,))
    action_space = _t.SimpleNamespace(shape=(3,))
    cnn_feat = [np.zeros((4, 5))]

    def seed(self, s):
        return

    def load_experts(self, *a):
        return


def _stub_cfg():
    import types
    return types.SimpleNamespace(seed=1, takes={"train": []}, expert_feat_file=None, cnn_feat_file=None, fr_margin=2, causal=False,
                                 policy_v_hdim=4, policy_v_net="lstm", policy_v_net_param=None, value_v_hdim=4, value_v_net="lstm",
                                 value_v_net_param=None, policy_hsize=[8], policy_htype="relu", value_hsize=[8], value_htype="relu",
                                 log_std=-1.0, fix_std=True, policy_optimizer="Adam", policy_lr=1e-3, policy_momentum=0.0,
                                 policy_weightdecay=0.0, value_optimizer="Adam", value_lr=1e-3, value_momentum=0.0, value_weightdecay=0.0,
                                 reward_id="quat_v3", num_optim_epoch=3, gamma=0.95, tau=0.95, clip_epsilon=0.2)


# ---------------------------------------------------------------------------------------------------- two ranks (gloo)
CUT = 21            # episodes [10, 4, 7] -> rank 0, [10, 2, 10, 5] -> rank 1 (tests/test_dist_gloo.py): unequal shards


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, target):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(1)
    from egopose_amd import dist as D
    from egopose_amd.rl_core import TrajBatchEgo
    g = load_golden(FIXTURE)
    agent, mods = UF.build_agent(g)
    for group in agent.optimizer_policy.param_groups:
        group["lr"] = LR_POLICY
    agent.target_kl = target
    sl = slice(0, CUT) if rank == 0 else slice(CUT, None)
    cols = {k: torch.as_tensor(g[k][sl]) for k in ("states", "actions", "masks", "rewards", "exps", "v_metas")}
    cols["next_states"] = cols["states"]

    def adv_fn(rewards, masks, values):                               # global standardisation, as tests/test_dist_gloo.py
        _, ret, raw = oracle_gae(rewards.numpy(), masks.numpy(), values.numpy(), agent.gamma, agent.tau)
        raw = raw.ravel()
        st = D.merge_moments(torch.tensor([raw.size, raw.mean(), ((raw - raw.mean()) ** 2).sum()], dtype=torch.float64))
        a = (raw - st[1].item()) / np.sqrt(st[2].item() / (st[0].item() - 1.0))
        return torch.as_tensor(a).unsqueeze(1), torch.as_tensor(ret)
    agent._advantages = adv_fn
    agent.update_params(TrajBatchEgo.from_device(**cols))
    with open(os.path.join(out_dir, "stats%d.json" % rank), "w") as f:
        json.dump(agent.update_stats, f)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **{k: v.numpy() for k, v in _state(mods).items()})
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_stop_together_on_the_global_kl(tmp_path):
    g = load_golden(FIXTURE)
    kl, target = _kl_target(g)                                          # the GLOBAL KL: one process, the whole batch
    single, _ = _run(g, target_kl=target)
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), target), nprocs=2, join=True)
    st = [json.load(open(tmp_path / ("stats%d.json" % r))) for r in (0, 1)]
    # same epoch, same figures, to the bit (json keeps float64). value_loss / surr_loss are, as without the monitor, each rank's
    # SHARE of the global loss (its rows over the global count): they add up to the single process's and are not compared here
    added = set(st[0]) - {"value_loss", "surr_loss"}
    assert added == set(FIGURES) | {"epochs_run", "stop_reason", "stop_figures"} and set(st[0]) == set(st[1])
    assert {k: st[0][k] for k in added} == {k: st[1][k] for k in added}
    for k in ("value_loss", "surr_loss"):
        np.testing.assert_allclose(np.add(st[0][k], st[1][k]), single.update_stats[k], rtol=1e-9)
    assert st[0]["stop_reason"] == "kl" and st[0]["epochs_run"] == 2 == single.update_stats["epochs_run"]
    ref = single.update_stats
    for k in FIGURES:
        np.testing.assert_allclose(st[0][k], ref[k], rtol=1e-12, atol=0, err_msg=k)
        np.testing.assert_allclose(st[0]["stop_figures"][k], ref["stop_figures"][k], rtol=1e-12, atol=0, err_msg=k)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert set(r0.files) == set(r1.files) and len(r0.files) > 0
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)
