"""TCN video nets on the HIP path (csrc/egp_tcn.hip), float32 on the device, against the reference's float64 runs
(tests/golden/tcn.npz) and against the torch path in float64."""
import copy
import os

import numpy as np
import pytest
import torch
import yaml

import tcn_fixture as F
from conftest import REPO

pytestmark = pytest.mark.gpu
TOL = 1e-4          # north_star's tolerance for the float32 HIP path (tests/test_update_gpu.py)
DEV = "cuda"


def _figures(net, y, dx, case):
    z = F.golden()
    fig = {"y": F.rel(y, z[case + "__y"])}
    if dx is not None:
        fig["dx"] = F.rel(dx, z[case + "__dx"])
    want, have = F.grads(case), dict(net.named_parameters())
    assert set(want) == set(have)
    for k, g in want.items():
        fig[k] = F.rel(have[k].grad, g)
    return fig


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_plain_nets_on_the_hip_path_match_the_reference(case):
    from egopose_amd import tcn
    calls = tcn.HIP_CALLS
    net, y, dx = F.run_plain(case, torch.float32, DEV)
    n_blocks = len(F.CASES[case][1])
    assert tcn.HIP_CALLS - calls == 4 * n_blocks          # two launches forward, two backward per block: the HIP path ran
    fig = _figures(net, y, dx, case)
    print(case, fig)
    assert max(fig.values()) <= TOL, fig


def test_the_reference_s_toy_shape_takes_the_torch_path():
    from egopose_amd import tcn
    calls = tcn.HIP_CALLS
    net, y, dx = F.run_plain("g", torch.float32, DEV)
    assert tcn.HIP_CALLS == calls
    fig = _figures(net, y, dx, "g")
    assert max(fig.values()) <= TOL, fig


def test_train_mode_video_state_net_on_the_hip_path_matches_the_reference():
    from egopose_amd import tcn
    calls = tcn.HIP_CALLS
    net, y = F.run_case_f(torch.float32, DEV)
    assert tcn.HIP_CALLS - calls == 2 * 2 + 2 * 2 - 1          # the first block's input needs no gradient: one launch fewer
    fig = _figures(net, y, None, "f")
    print(fig)
    assert max(fig.values()) <= TOL, fig


def test_forced_torch_path(monkeypatch):
    from egopose_amd import tcn
    monkeypatch.setattr(tcn, "_IMPL", "torch")          # what EGP_TCN=torch sets at import
    calls = tcn.HIP_CALLS
    net, y, dx = F.run_plain("a", torch.float32, DEV)
    assert tcn.HIP_CALLS == calls
    assert max(_figures(net, y, dx, "a").values()) <= TOL


def _guarded(rows, width, lead, tail, fill):
    buf = torch.full((lead + rows + tail, width), fill, dtype=torch.float32, device=DEV)
    return buf, buf[lead:lead + rows]


@pytest.mark.parametrize("dgrad", [False, True])
def test_rows_outside_the_batch_are_neither_read_nor_written(dgrad):
    """Case a's first convolution (and the data-gradient launch of the same shape) with X between NaN rows and the result
    inside a larger buffer of sentinels: no tap may reach a row outside [0, T*B), no store may leave the result's rows."""
    from egopose_amd import tcn
    z = F.golden()
    T, B = 23, 3
    M = T * B
    net = F.plain_net("a", torch.float32, DEV)
    blk = net.network[1]                                   # 16 -> 32, dilation 2: shifts of +-6 rows
    with torch.no_grad():
        w = blk.conv1.weight.detach()
        x = torch.from_numpy(z["a__x"]).to(DEV, torch.float32).reshape(M, 16)
        if dgrad:
            torch.manual_seed(3)
            x, w_p = torch.randn(M, 32, device=DEV), tcn._pack(w, True)
            kw = dict(shift0=2, dshift=-2)
        else:
            w_p = tcn._pack(w, False)
            kw = dict(shift0=-2, dshift=2, bias=blk.conv1.bias.detach(), relu=True)
        plain = tcn.conv_rows(x.contiguous(), T, B, w_p, **kw)
        xbuf, xv = _guarded(M, x.shape[1], 7, 9, float("nan"))
        xv.copy_(x)
        obuf, ov = _guarded(M, plain.shape[1], 5, 11, -77.0)
        o2buf, o2v = _guarded(M, plain.shape[1], 2, 3, -55.0)
        tcn.conv_rows(xv, T, B, w_p, out=ov, out2=o2v, **kw)
        torch.cuda.synchronize()
    assert torch.isfinite(plain).all() and torch.equal(ov, plain) and torch.equal(o2v, plain)
    assert (obuf[:5] == -77.0).all() and (obuf[5 + M:] == -77.0).all()
    assert (o2buf[:2] == -55.0).all() and (o2buf[2 + M:] == -55.0).all()
    assert torch.isnan(xbuf[:7]).all() and torch.isnan(xbuf[7 + M:]).all()


@pytest.mark.parametrize("launch", ["conv2_forward", "dgrad_downsample", "dgrad_identity"])
def test_block_launches_with_every_operand_between_guard_rows(launch):
    """The launches a block really issues -- conv2 forward with the dropout mask, the second output and the residual product
    on top of the activation; the data gradients with gate, mask and the residual branch in the same sum -- with X, X2, mask
    and gate each between NaN rows and both outputs between sentinels: same result as on plain buffers, nothing outside the
    batch's rows read into it or written."""
    from egopose_amd import tcn
    T, B = 23, 3
    M = T * B
    torch.manual_seed(13)
    r = lambda *shape: torch.randn(*shape, device=DEV)
    keep = lambda c: torch.empty(M, c, device=DEV).bernoulli_(0.8).div_(0.8)
    if launch == "conv2_forward":
        x, w, n_out = r(M, 32), r(3, 32, 32) * 0.1, 32
        kw = dict(shift0=-2, dshift=2, bias=r(32), relu=True, mask=keep(32), x2=r(M, 16), w2=r(32, 16) * 0.1, b2=r(32), x2_after_act=True)
    elif launch == "dgrad_downsample":
        x, w, n_out = r(M, 32), r(3, 16, 32) * 0.1, 16
        kw = dict(shift0=2, dshift=-2, mask=keep(16), gate=r(M, 16), x2=r(M, 32), w2=r(16, 32) * 0.1)
    else:
        x, w, n_out = r(M, 32), r(3, 32, 32) * 0.1, 32
        kw = dict(shift0=2, dshift=-2, mask=keep(32), gate=r(M, 32), x2=r(M, 32))
    plain2 = torch.empty(M, n_out, device=DEV)
    plain = tcn.conv_rows(x, T, B, w, out2=plain2, **kw)
    guarded, bufs = dict(kw), []
    for i, name in enumerate(("mask", "gate", "x2")):
        if kw.get(name) is not None:
            buf, view = _guarded(M, kw[name].shape[1], 3 + i, 4 + i, float("nan"))
            view.copy_(kw[name])
            guarded[name] = view
            bufs.append(buf)
    xbuf, xv = _guarded(M, 32, 7, 9, float("nan"))
    xv.copy_(x)
    obuf, ov = _guarded(M, n_out, 5, 11, -77.0)
    o2buf, o2v = _guarded(M, n_out, 2, 3, -55.0)
    tcn.conv_rows(xv, T, B, w, out=ov, out2=o2v, **guarded)
    torch.cuda.synchronize()
    assert torch.isfinite(plain).all() and torch.isfinite(plain2).all()
    assert torch.equal(ov, plain) and torch.equal(o2v, plain2)
    if launch == "conv2_forward":
        assert not torch.equal(plain, plain2)              # out2 is the activation before the residual
    assert (obuf[:5] == -77.0).all() and (obuf[5 + M:] == -77.0).all()
    assert (o2buf[:2] == -55.0).all() and (o2buf[2 + M:] == -55.0).all()


def test_unsupported_launches_are_refused():
    from egopose_amd import tcn
    x = torch.zeros(12, 16, device=DEV)
    with pytest.raises(ValueError):
        tcn.conv_rows(torch.zeros(12, 24, device=DEV), 4, 3, torch.zeros(3, 16, 24, device=DEV), -1, 1)          # C_in % 16
    with pytest.raises(ValueError):
        tcn.conv_rows(x, 4, 3, torch.zeros(9, 16, 16, device=DEV), -4, 1)                                        # 9 taps
    with pytest.raises(ValueError):
        tcn.conv_rows(x, 4, 3, torch.zeros(3, 32, 16, device=DEV), -1, 1, x2=x)                                  # identity with C2 != C_out


def test_block_with_explicit_dropout_masks_hip_vs_torch_float64():
    from egopose_amd import tcn
    torch.manual_seed(11)
    T, B, p = 23, 3, 0.2
    blk = tcn.TemporalBlock(16, 32, 3, 2, p, False).to(DEV).train()
    with torch.no_grad():
        blk.conv1.weight_g.mul_(1.3)
        blk.downsample.weight.normal_(0.0, 0.3)
    ref = copy.deepcopy(blk).double()
    x = torch.randn(T, B, 16, device=DEV)
    masks = [torch.empty(T, B, 32, device=DEV).bernoulli_(1 - p).div_(1 - p) for _ in range(2)]
    R = torch.randn(T, B, 32, device=DEV)
    assert 0.1 < float((masks[0] == 0).float().mean()) < 0.3
    calls = tcn.HIP_CALLS
    xh = x.clone().requires_grad_(True)
    yh = blk.forward_tm(xh, masks=tuple(masks))
    (yh * R).sum().backward()
    assert tcn.HIP_CALLS - calls == 4
    xr = x.double().requires_grad_(True)
    yr = ref.forward_tm(xr, masks=tuple(m.double() for m in masks))
    (yr * R.double()).sum().backward()
    assert tcn.HIP_CALLS - calls == 4
    fig = {"y": F.rel(yh, yr.detach().cpu()), "dx": F.rel(xh.grad, xr.grad.cpu())}
    have = dict(blk.named_parameters())
    for k, q in ref.named_parameters():
        fig[k] = F.rel(have[k].grad, q.grad.cpu())
    print(fig)
    assert max(fig.values()) <= TOL, fig


def test_video_nets_on_the_device():
    from egopose_amd import tcn
    z = F.golden()
    calls = tcn.HIP_CALLS
    vs = F.video_state_net(torch.float32, DEV)
    with torch.no_grad():
        vs.initialize(torch.from_numpy(z["e_vs__x"]))
    assert tcn.HIP_CALLS - calls == 4 and F.rel(vs.v_out, z["e_vs__v_out"]) <= TOL
    fc = F.forecast_net(torch.float32, DEV)
    with torch.no_grad():
        fc.initialize(torch.from_numpy(z["e_fc__x"]))
        y = fc(torch.from_numpy(z["e_fc__state"]).to(DEV, torch.float32))
    assert F.rel(fc.v_out, z["e_fc__v_out"]) <= TOL and F.rel(y, z["e_fc__y"]) <= TOL
    # a batch of windows == the windows one by one
    torch.manual_seed(7)
    win = torch.randn(28, 6, 16, device=DEV)
    with torch.no_grad():
        vs.initialize(win)
        batched = vs.v_out.clone()
        assert tuple(batched.shape) == (20, 6, 32)
        for b in range(6):
            vs.initialize(win[:, b].contiguous())
            assert torch.equal(vs.v_out, batched[:, b]), b


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def workspace(tmp_path_factory):
    from egopose_amd.bench_support import write_synthetic_dataset
    root = str(tmp_path_factory.mktemp("egp_tcn_ws"))
    write_synthetic_dataset(root, "subject_03", n_takes=3, n_frames=300, seed=4)
    return root


def _tcn_trainer(workspace, task, episode_len, dropout=0.0, **extra):
    from egopose_amd.config import Config, ForecastConfig
    from egopose_amd.train import Trainer
    os.chdir(workspace)
    with open(os.path.join(REPO, "egopose_amd", "assets", "config", task, "subject_03.yml")) as f:
        cfg_dict = yaml.safe_load(f)
    param = {"size": [64, 128], "dropout": dropout}
    cfg_dict.update(policy_v_net="tcn", value_v_net="tcn", policy_v_net_param=dict(param), value_v_net_param=dict(param), **extra)
    cfg = (ForecastConfig if task == "egoforecast" else Config)("subject_03", create_dirs=False, cfg_dict=cfg_dict)
    cfg.env_episode_len = episode_len
    cfg.num_optim_epoch = 2
    return Trainer(cfg, torch.device("cuda", 0), torch.float32, num_envs=8, num_threads=2, num_groups=1), cfg


def _tcn_params(tr):
    return [(n + "." + k, p) for n in ("policy_vs_net", "value_vs_net") for k, p in getattr(tr, n).v_net.named_parameters()]


def _finite_stats(tr):
    stats = tr.agent.update_stats
    assert stats and all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for v in stats.values()), stats


def test_ego_mimic_trainer_with_tcn_video_nets(workspace, monkeypatch):
    from egopose_amd import tcn
    tr, cfg = _tcn_trainer(workspace, "egomimic", 10)
    try:
        assert isinstance(tr.policy_vs_net.v_net, tcn.TemporalConvNet) and not tr.policy_vs_net.v_net.causal
        tr.pre_iter_update(0)
        batch, log = tr.agent.sample(8 * 12)
        before = [p.detach().clone() for _, p in _tcn_params(tr)]
        calls = tcn.HIP_CALLS
        tr.agent.update_params(batch)
        torch.cuda.synchronize()
        assert tcn.HIP_CALLS > calls
        _finite_stats(tr)
        for (name, p), b in zip(_tcn_params(tr), before):
            assert torch.isfinite(p).all() and not torch.equal(p.detach(), b), name
        # the train-mode context of the same batch: HIP float32 against the torch path in float64, gradients compared
        net = tr.agent.cn.policy_vs_net
        masks = torch.as_tensor(np.asarray(batch.masks), dtype=torch.float32, device=DEV)
        v_metas = batch.device_column("v_metas") if hasattr(batch, "device_column") else None
        v_metas = v_metas.cpu().numpy() if v_metas is not None else batch.v_metas
        net.set_mode("train")
        net.initialize((masks, tr.env.cnn_feat, v_metas))
        torch.manual_seed(5)
        n = masks.shape[0]
        sdim = tr.env.observation_space.shape[0]
        states = torch.randn(n, sdim, device=DEV)
        R = torch.randn(n, 128 + sdim, device=DEV)
        net.zero_grad()
        calls = tcn.HIP_CALLS
        out = net(states)
        (out * R).sum().backward()
        assert tcn.HIP_CALLS - calls == 7
        ref = copy.deepcopy(net).double()
        ref.cnn_feat_ctx = net.cnn_feat_ctx.double()
        ref.zero_grad()
        monkeypatch.setattr(tcn, "_IMPL", "torch")
        calls = tcn.HIP_CALLS
        out64 = ref(states.double())
        (out64 * R.double()).sum().backward()
        assert tcn.HIP_CALLS == calls
        monkeypatch.setattr(tcn, "_IMPL", "hip")
        fig = {"ctx": F.rel(out, out64.detach().cpu())}
        have = dict(net.named_parameters())
        for k, q in ref.named_parameters():
            fig[k] = F.rel(have[k].grad, q.grad.cpu())
        print(fig)
        assert max(fig.values()) <= TOL, fig
        # dropout on: masks are drawn in the update, the second update stays finite
        for vs in (tr.policy_vs_net, tr.value_vs_net):
            for blk in vs.v_net.network:
                blk.dropout = 0.2
        tr.agent.update_params(batch)
        torch.cuda.synchronize()
        _finite_stats(tr)
        assert all(torch.isfinite(p).all() for _, p in _tcn_params(tr))
    finally:
        tr.close()


def test_ego_forecast_trainer_with_a_tcn_video_side(workspace):
    from egopose_amd import tcn
    tr, cfg = _tcn_trainer(workspace, "egoforecast", 10, policy_s_net="lstm", value_s_net="lstm")
    try:
        assert tr.policy_vs_net.v_net.causal and tr.policy_vs_net.s_net_type == "lstm"
        tr.pre_iter_update(0)
        batch, log = tr.agent.sample(8 * 12)
        calls = tcn.HIP_CALLS
        tr.agent.update_params(batch)
        torch.cuda.synchronize()
        assert tcn.HIP_CALLS > calls
        _finite_stats(tr)
        assert all(torch.isfinite(p).all() for _, p in _tcn_params(tr))
    finally:
        tr.close()


@pytest.mark.parametrize("task", ["egomimic", "egoforecast"])
def test_update_with_dropout_takes_gae_values_and_fixed_log_probs_in_eval_mode(workspace, monkeypatch, task):
    """With dropout 0.2 in the video nets the values GAE consumes and the action means that fix the sampling policy's
    log-probabilities are the eval-mode ones (the reference computes both under to_test, agents/agent_pg.py:40-46,
    agents/agent_ppo.py:16-22), not those of a train-mode pass that drew masks. Both are recomputed here in eval mode at the
    moment the update uses them (nothing has stepped yet). Same weights, same kernels, same inputs: the bound 1e-6 of the
    largest reference element leaves room for nothing but a reordered sum; a context under dropout differs by orders more."""
    from egopose_amd import agent as A
    from egopose_amd.torch_utils import to_test
    extra = dict(policy_s_net="lstm", value_s_net="lstm") if task == "egoforecast" else {}
    tr, cfg = _tcn_trainer(workspace, task, 10, dropout=0.2, **extra)
    try:
        ag = tr.agent
        assert ag._dropout_active() and tr.policy_vs_net.v_net.network[0].dropout == 0.2
        tr.pre_iter_update(0)
        batch, log = ag.sample(8 * 12)
        seen = {}
        real_load, real_adv, real_losses = ag._load_batch, ag._advantages_with_counts, A.O.ppo_losses

        def spy_load(b):
            seen["c"] = real_load(b)
            return seen["c"]

        def spy_adv(rewards, masks, values, counts):
            with to_test(*ag.update_modules), torch.no_grad():
                ref = ag.cn.value_net(ag.trans_value(seen["c"]["states"]))
            seen["values"] = (values.detach().clone(), ref.clone())
            return real_adv(rewards, masks, values, counts)

        def spy_losses(pred, returns, mean, actions, log_std, adv, fixed, write_fixed, *a, **k):
            if write_fixed:
                assert "mean" not in seen, "the log-probabilities are fixed once"
                rows = k.get("rows")
                with to_test(*ag.update_modules), torch.no_grad():
                    x = ag.trans_policy(seen["c"]["states"])
                    ref = ag._policy_mean(x if rows is None else x[rows])
                seen["mean"] = (mean.detach().clone(), ref.clone())
            return real_losses(pred, returns, mean, actions, log_std, adv, fixed, write_fixed, *a, **k)

        monkeypatch.setattr(ag, "_load_batch", spy_load)
        monkeypatch.setattr(ag, "_advantages_with_counts", spy_adv)
        monkeypatch.setattr(A.O, "ppo_losses", spy_losses)
        ag.update_params(batch)
        torch.cuda.synchronize()
        _finite_stats(tr)
        for what in ("values", "mean"):
            got, ref = seen[what]
            err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
            print(task, what, err)
            assert got.shape == ref.shape and err <= 1e-6, (what, err)
    finally:
        tr.close()
