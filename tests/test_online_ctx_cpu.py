"""VideoStateNet.online_contexts against its definition, float64 on the CPU: row t is what the reference's online evaluation
(ego_pose/ego_mimic_eval.py:143-145) gets from `initialize(x[:t + 2m + 1]); v_out[t]`, for every kind of video net, and what
tells it from the offline contexts."""
import numpy as np
import pytest
import torch

D, HD, T = 8, 8, 9


def _net(kind, m, causal=False, seed=3):
    from egopose_amd.nets import VideoStateNet
    torch.manual_seed(seed)
    param = {"size": [8, 8], "kernel_size": 3, "dropout": 0.2} if kind == "tcn" else None
    net = VideoStateNet(D, HD, m, kind, param, causal).double()
    net.eval()
    net.set_mode("test")
    x = torch.randn(T + 2 * m, D, dtype=torch.float64)
    return net, x


def _definition(net, x):
    m = net.v_margin
    rows = []
    with torch.no_grad():
        for t in range(x.shape[0] - 2 * m):
            net.initialize(x[:t + 2 * m + 1])
            rows.append(net.v_out[t].clone())
    return torch.stack(rows, 0).numpy()


def _offline(net, x):
    with torch.no_grad():
        net.initialize(x)
    return net.v_out.clone().numpy()


@pytest.mark.parametrize("m", [3, 1])
def test_bilstm_is_the_definition_and_not_the_offline_context(m):
    net, x = _net("lstm", m)
    want, off = _definition(net, x), _offline(net, x)
    # the reference loop alone: the last tick has seen the whole take, every earlier one has a backward direction of its own
    np.testing.assert_allclose(want[-1], off[-1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(want[:, :HD // 2], off[:, :HD // 2], rtol=0, atol=1e-12)
    gap = np.abs(want[:-1, HD // 2:] - off[:-1, HD // 2:]).max(1)
    print("bi-LSTM m=%d: right half online - offline, per row" % m, gap)
    assert (gap > 1e-3).all()
    net.v_out, net.t = None, 5
    got = net.online_contexts(x)
    assert net.v_out is None and net.t == 5                   # the test-mode state of the net is left alone
    assert got.shape == (T, HD) and got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[-1].numpy(), off[-1], rtol=0, atol=1e-12)
    assert (np.abs(got.numpy()[:-1, HD // 2:] - off[:-1, HD // 2:]).max(1) > 1e-3).all()


@pytest.mark.parametrize("kind", ["lstm", "tcn"])
def test_causal_nets_online_equals_offline(kind):
    net, x = _net(kind, 3, causal=True)
    want = _definition(net, x)
    got = net.online_contexts(x).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got, _offline(net, x), rtol=0, atol=1e-12)


def test_tcn_inside_its_reach_is_the_offline_context():
    """[8, 8], k = 3: one-sided reach (3 - 1) * (2**2 - 1) = 6 frames = the margin."""
    net, x = _net("tcn", 6)
    want = _definition(net, x)
    got = net.online_contexts(x).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got, _offline(net, x))


def test_tcn_beyond_its_reach_goes_by_the_definition():
    net, x = _net("tcn", 3)
    want, off = _definition(net, x), _offline(net, x)
    got = net.online_contexts(x).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    gap = np.abs(want - off).max(1)
    print("TCN reach 6, m = 3: online - offline per row", gap)
    assert (gap > 1e-6).any()                                 # the shortcut would have been wrong here
    np.testing.assert_allclose(want[-1], off[-1], rtol=0, atol=1e-12)


def test_bad_input_and_mode():
    net, x = _net("lstm", 3)
    with pytest.raises(ValueError):
        net.online_contexts(x[:6])                            # 2m frames: no tick
    with pytest.raises(ValueError):
        net.online_contexts(x.unsqueeze(1))
    net.set_mode("train")
    with pytest.raises(RuntimeError):
        net.online_contexts(x)


def test_select_evaluator_keeps_its_answers_without_the_keyword():
    from egopose_amd.evaluate import BatchedEvaluator, BatchedOnlineEvaluator, Evaluator, select_evaluator
    from egopose_amd.nets import MLP, PolicyGaussian, Value
    torch.manual_seed(0)
    pol, val = PolicyGaussian(MLP(12, (16, 8), "relu"), 4), Value(MLP(12, (16, 8), "relu"))
    assert select_evaluator(pol, val, num_envs=4) == (BatchedEvaluator, None)
    assert select_evaluator(pol, val, num_envs=1) == (Evaluator, None)
    assert select_evaluator(pol, val, num_envs=4, sequential=True) == (Evaluator, None)
    for kw in (dict(causal=True), dict(show_noise=True), dict(causal=True, show_noise=True)):
        cls, why = select_evaluator(pol, val, num_envs=4, **kw)
        assert cls is Evaluator and why
    cls, why = select_evaluator(pol, val.double(), num_envs=4)
    assert cls is Evaluator and "float32" in why
    # the new keyword alone changes nothing; with `causal` it picks the online class, unless something else needs the old path
    val = val.float()
    assert select_evaluator(pol, val, num_envs=4, batched_online=True) == (BatchedEvaluator, None)
    assert select_evaluator(pol, val, num_envs=4, causal=True, batched_online=True) == (BatchedOnlineEvaluator, None)
    assert select_evaluator(pol, val, num_envs=1, causal=True, batched_online=True) == (Evaluator, None)
    assert select_evaluator(pol, val, num_envs=4, sequential=True, causal=True, batched_online=True) == (Evaluator, None)
    cls, why = select_evaluator(pol, val, num_envs=4, causal=True, show_noise=True, batched_online=True)
    assert cls is Evaluator and why
    cls, why = select_evaluator(pol, val.double(), num_envs=4, causal=True, batched_online=True)
    assert cls is Evaluator and "float32" in why
    assert issubclass(BatchedOnlineEvaluator, BatchedEvaluator) and BatchedOnlineEvaluator.save is Evaluator.save
