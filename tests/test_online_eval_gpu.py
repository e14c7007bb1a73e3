"""BatchedOnlineEvaluator (egopose_amd/evaluate.py): the online evaluation of the reference (ego_pose/ego_mimic_eval.py --causal,
:143-145: the policy's video net re-initialised at every tick on the frames seen so far) with the takes on lockstep slots. Its
traced actions against a float64 policy chain on the online contexts BY THE DEFINITION (a float64 net re-initialised prefix by
prefix), far from the same chain on the offline contexts; its values on the offline value contexts; independence of the slot count;
the `valuefs` decisions; the pickle's name; the selection helper. The fixture repeats the recipe of test_mimic_eval_batched_gpu.py."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FAIL_SAFES = ("valuefs", "naivefs", "none")


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """3 takes of 60 frames (test_len 40), take 1 cut to 45 (test_len 25); a trainer whose running filter has seen a sampling
    pass; a state regressor; the value head calibrated so that `valuefs` fires now and then.

    A freshly initialised bi-LSTM forgets within a few frames and the fresh policy hardly reads its context: online and offline
    actions then differ by ~1e-5 (float64, these shapes), below what the fused step's float32 can show. So the policy's side is
    made to depend on the look-ahead: W_hh of its backward cell x 4 (a longer memory), the first layer's columns for the backward
    half x 8, the action head x 4. With that the float64 chains differ by 4e-3 .. 2e-2 on most ticks of a take (|action| ~ 0.15),
    which is what the 2e-3 assertion below needs; the weights are fixed by cfg.seed, the features by the dataset's seed."""
    from egopose_amd.bench_support import write_synthetic_dataset
    from egopose_amd.config import Config
    from egopose_amd.nets import VideoRegNet
    from egopose_amd.train import Trainer
    root = str(tmp_path_factory.mktemp("egp_ws_oneval"))
    write_synthetic_dataset(root, "subject_03", n_takes=3, n_frames=60, seed=6)
    os.chdir(root)
    cfg = Config("subject_03", create_dirs=False)
    cfg.env_episode_len = 15
    cfg.num_optim_epoch = 2
    tr = Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=8, num_threads=2, num_groups=1)
    cfg.env_init_noise = 0.0
    tr.agent.sample(8 * 20)
    assert tr.running_state.rs.n > 100
    env = tr.env
    assert env.cnn_feat[0].shape[0] == 60 and cfg.fr_margin == 10
    env.cnn_feat[1] = env.cnn_feat[1][:45]
    env.expert_arr[1] = {k: (v[:45] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == 60 else v) for k, v in env.expert_arr[1].items()}
    if "len" in env.expert_arr[1]:
        env.expert_arr[1]["len"] = 45
    torch.manual_seed(11)
    state_net = VideoRegNet(115, 128, env.cnn_feat[0].shape[-1]).cuda()
    ex = env.expert_arr[0]
    obs_like = np.concatenate([ex["qpos"][10:, 2:], ex["qvel"][10:]], 1)
    assert tr.policy_vs_net.v_net.bi_dir and tr.policy_vs_net.v_hdim == 128
    with torch.no_grad():
        tr.policy_vs_net.v_net.rnn_b.weight_hh.mul_(4.0)
        tr.policy_net.net.affine_layers[0].weight[:, 64:128].mul_(8.0)
        tr.policy_net.action_mean.weight.mul_(4.0)
        tr.value_net.value_head.weight.mul_(30.0)
        tr.value_net.value_head.bias.fill_(1.0)
    out = dict(tr=tr, cfg=cfg, env=env, root=root, state_net=state_net, mean=obs_like.mean(0), std=np.full(115, 0.02))
    # the head being linear: moved to mean 1 / standard deviation 1 over a run without fail-safe, so that a good part of the
    # values, not all, lies below 0.6 x the running mean
    from egopose_amd.evaluate import BatchedOnlineEvaluator
    ev = BatchedOnlineEvaluator(cfg, env, tr.policy_net, tr.policy_vs_net, tr.value_net, tr.value_vs_net, state_net, out["mean"], out["std"],
                                running_state=tr.running_state, fail_safe="none", keep_trace=True, num_envs=3, n_threads=2)
    ev.run()
    v = np.concatenate([ev.trace[t]["values"] for t in env.expert_list])
    print("value head before calibration: mean %.4f std %.4f" % (v.mean(), v.std()))
    with torch.no_grad():
        head = tr.value_net.value_head
        head.bias.copy_(1.0 + (head.bias - float(v.mean())) / float(v.std()))
        head.weight.div_(float(v.std()))
    yield out
    tr.close()


_RUNS = {}


def _run(setup, fail_safe, n_slots):
    """One BatchedOnlineEvaluator run per (fail_safe, slot count), shared by the tests (a fresh evaluator: a fresh value statistic)."""
    from egopose_amd.evaluate import BatchedOnlineEvaluator
    key = (fail_safe, n_slots)
    if key not in _RUNS:
        tr = setup["tr"]
        ev = BatchedOnlineEvaluator(setup["cfg"], setup["env"], tr.policy_net, tr.policy_vs_net, tr.value_net, tr.value_vs_net, setup["state_net"],
                                    setup["mean"], setup["std"], running_state=tr.running_state, fail_safe=fail_safe, keep_trace=True,
                                    num_envs=n_slots, n_threads=2)
        results, meta = ev.run()
        _RUNS[key] = (ev, results, meta)
    return _RUNS[key]


_CTX = {}


def _contexts64(setup):
    """Per take, once: (online policy contexts by the float64 definition loop, offline policy contexts in float64), on the CPU."""
    if not _CTX:
        net = copy.deepcopy(setup["tr"].policy_vs_net).double().cpu()
        net.eval()
        net.set_mode("test")
        m = setup["cfg"].fr_margin
        for i, take in enumerate(setup["env"].expert_list):
            x = torch.as_tensor(np.asarray(setup["env"].cnn_feat[i]), dtype=torch.float64)
            rows = []
            with torch.no_grad():
                for t in range(x.shape[0] - 2 * m):
                    net.initialize(x[:t + 2 * m + 1])
                    rows.append(net.v_out[t].clone())
                net.initialize(x)
            _CTX[take] = (torch.stack(rows, 0), net.v_out.clone())
    return _CTX


@pytest.mark.parametrize("fail_safe", FAIL_SAFES)
def test_results_do_not_depend_on_the_slot_count(setup, fail_safe):
    ev2, r2, m2 = _run(setup, fail_safe, 2)
    ev3, r3, m3 = _run(setup, fail_safe, 3)
    ev5, r5, m5 = _run(setup, fail_safe, 5)            # more slots than takes: the first pass leaves two slots without a take
    assert ev2.causal is True and m2 == m3 == m5 and ev3.timing["passes"] < ev2.timing["passes"]
    if fail_safe == "none":
        assert m2["num_reset"] == 0
    for i, take in enumerate(setup["env"].expert_list):
        test_len = 25 if i == 1 else 40
        assert r2["traj_pred"][take].shape == r2["traj_orig"][take].shape == (test_len, 59) and r2["vel_pred"][take].shape == (test_len, 58)
    for evn, rn in ((ev3, r3), (ev5, r5)):
        for take in setup["env"].expert_list:
            for k in ("traj_pred", "vel_pred", "traj_orig"):
                np.testing.assert_array_equal(r2[k][take], rn[k][take])
            a, b = ev2.trace[take], evn.trace[take]
            np.testing.assert_array_equal(a["actions"], b["actions"])
            np.testing.assert_array_equal(a["values"], b["values"])
            np.testing.assert_array_equal(a["states"], b["states"])
            assert list(a["resets"]) == list(b["resets"])


@pytest.mark.parametrize("fail_safe", FAIL_SAFES)
def test_traced_actions_are_online_and_values_offline(setup, fail_safe):
    """Actions: the float64 policy chain on cat(online context by the definition, traced state), at the fused step's tolerance
    against float64 -- and NOT the chain on the offline contexts. Values: the float64 value chain on the offline value contexts."""
    ev, results, meta = _run(setup, fail_safe, 2)
    tr, env = setup["tr"], setup["env"]
    pol64, val64 = copy.deepcopy(tr.policy_net).double(), copy.deepcopy(tr.value_net).double()
    ctx = _contexts64(setup)
    for i, take in enumerate(env.expert_list):
        trc = ev.trace[take]
        feat = torch.as_tensor(env.cnn_feat[i], dtype=torch.float32, device="cuda")
        st = dev(trc["states"])
        assert np.abs(trc["states"]).max() <= 5.0
        on, off = ctx[take][0].cuda(), ctx[take][1].cuda()
        assert on.shape == off.shape == (st.shape[0], 128)
        with torch.no_grad():
            tr.value_vs_net.initialize(feat)
            mean_on, _ = pol64.mean_std(torch.cat((on, st), 1))
            mean_off, _ = pol64.mean_std(torch.cat((off, st), 1))
            value = val64.value_head(val64.net(torch.cat((tr.value_vs_net.v_out.double(), st), 1))).reshape(-1)
        mean_on, mean_off = mean_on.cpu().numpy(), mean_off.cpu().numpy()
        gap_on = np.abs(trc["actions"] - mean_on).max(1)
        gap_off = np.abs(trc["actions"] - mean_off).max(1)
        print("%s %s: |action - online chain| max %.3g, |action - offline chain| max %.3g median %.3g, |action| max %.3g"
              % (fail_safe, take, gap_on.max(), gap_off.max(), np.median(gap_off), np.abs(trc["actions"]).max()))
        np.testing.assert_allclose(trc["actions"], mean_on, rtol=2e-4, atol=2e-4, err_msg=take)
        np.testing.assert_allclose(trc["values"], value.cpu().numpy(), rtol=2e-4, atol=2e-4, err_msg=take)
        assert gap_off.max() > 2e-3, "take %s was evaluated on the offline contexts" % take
        np.testing.assert_allclose(trc["actions"][-1], mean_off[-1], rtol=2e-4, atol=2e-4)       # the last tick has seen the whole take
        assert np.abs(trc["actions"]).max() > 1e-3


def test_valuefs_decisions_are_the_sequential_statistic(setup):
    from egopose_amd.zfilter import RunningStat
    ev, results, meta = _run(setup, "valuefs", 2)
    stat = RunningStat(1)
    n_reset = n_kept = 0
    for take in setup["env"].expert_list:
        trc = ev.trace[take]
        want = []
        for t, v in enumerate(trc["values"]):
            stat.push(np.array([float(v)]))
            if t == len(trc["values"]) - 1:
                break
            if v < 0.6 * stat.mean[0]:
                want.append(t)
            else:
                n_kept += 1
        assert want == list(trc["resets"]), take
        n_reset += len(want)
    print("valuefs: %d re-seats, %d decisions without, scheduler passes %s" % (n_reset, n_kept, ev.timing["fs_pass_takes"]))
    assert meta["num_reset"] == n_reset and n_reset >= 1 and n_kept >= 1
    assert ev.value_stat.n == stat.n == 105 and ev.value_stat.mean[0] == stat.mean[0]


@pytest.mark.parametrize("fail_safe", FAIL_SAFES)
def test_saved_file_is_the_causal_one(setup, fail_safe):
    from egopose_amd.evaluate import Evaluator
    ev, results, meta = _run(setup, fail_safe, 2)
    cfg = copy.copy(setup["cfg"])
    cfg.result_dir = os.path.join(setup["root"], "results_oneval")
    ev_cfg, ev.cfg = ev.cfg, cfg
    try:
        path = ev.save(results, meta, 7, data="test")
    finally:
        ev.cfg = ev_cfg
    assert path.endswith("iter_0007_test%s_causal.p" % ("" if fail_safe == "valuefs" else "_" + fail_safe))
    assert type(ev).save is Evaluator.save
    r2, m2 = pickle.load(open(path, "rb"))
    assert m2 == meta and set(r2) == {"traj_pred", "traj_orig", "vel_pred"} and set(m2) == {"algo", "num_reset"}
    assert m2["algo"] == "ego_mimic" and list(r2["traj_pred"]) == list(setup["env"].expert_list)
    for take in setup["env"].expert_list:
        for k in r2:
            np.testing.assert_array_equal(r2[k][take], results[k][take])


def test_selection_and_the_refusal_that_stays(setup):
    from egopose_amd.evaluate import BatchedEvaluator, BatchedOnlineEvaluator, Evaluator, select_evaluator
    tr = setup["tr"]
    args = (setup["cfg"], setup["env"], tr.policy_net, tr.policy_vs_net, tr.value_net, tr.value_vs_net, setup["state_net"], setup["mean"], setup["std"])
    assert select_evaluator(tr.policy_net, tr.value_net, num_envs=4, causal=True, batched_online=True) == (BatchedOnlineEvaluator, None)
    assert select_evaluator(tr.policy_net, tr.value_net, num_envs=4, batched_online=True) == (BatchedEvaluator, None)
    cls, why = select_evaluator(tr.policy_net, tr.value_net, num_envs=4, causal=True)
    assert cls is Evaluator and why
    cls, why = select_evaluator(tr.policy_net, tr.value_net, num_envs=4, causal=True, show_noise=True, batched_online=True)
    assert cls is Evaluator and why
    assert select_evaluator(tr.policy_net, tr.value_net, num_envs=4, sequential=True, causal=True, batched_online=True) == (Evaluator, None)
    with pytest.raises(NotImplementedError, match="Evaluator"):
        BatchedEvaluator(*args, causal=True)
    with pytest.raises(TypeError):
        BatchedOnlineEvaluator(*args, causal=True)           # the constructor has no `causal` / `show_noise` to set
    with pytest.raises(TypeError):
        BatchedOnlineEvaluator(*args, show_noise=True)
    with pytest.raises(NotImplementedError, match="Evaluator"):
        BatchedOnlineEvaluator(*args[:4], copy.deepcopy(tr.value_net).double(), *args[5:])
