"""`nets.mlp_head(net, head, x)`, the one dispatch behind PolicyGaussian.mean_std, Value.forward and Discriminator.logits.

CPU: no HIP product is available, so the three modules take the shared fallback and return exactly head(net(x)).

GPU: the two fused forms of the update path -- a `gemm.GatheredInput` ([context | state] never formed: GatherMlpHead) and the
materialised tensor tagged `_egp_ctx_cols` = H (GatherConcat + MlpHead) -- are the same products in the same order: outputs and
every parameter and context gradient are bit-equal, and both agree with float64 autograd of the same modules.
Shapes: n = 70 rows (a full 64-row block and a ragged tail), context width H = 128, S = 32 state columns, hidden (64, 32),
distinct indices into 90 context rows (the other rows' gradient must stay zero), three-piece products.
Tolerances: those of tests/test_mlp_act_gpu.py for these products, 2e-5 on the output and 5e-5 on every gradient, relative in the
Frobenius norm. They hold where no float32 pre-activation falls on the other side of a relu than its float64 value; the relu case
asserts that of its own inputs (every float64 pre-activation at least KINK from zero, ten times the products' error).
"""
import copy

import pytest
import torch

H, S, HIDDEN, N_ROWS, N_CTX = 128, 32, (64, 32), 70, 90
KINK = 1e-5       # a float32 pre-activation of these widths is within ~1e-6 of its float64 value: no relu gate differs beyond this


CALLS = [lambda m, x: m.mean_std(x)[0], lambda m, x: m(x), lambda m, x: m.logits(x)]       # with the heads of _heads, in its order


def _heads(act, in_dim, hidden, seed):
    from egopose_amd.nets import MLP, Discriminator, PolicyGaussian, Value
    torch.manual_seed(seed)
    mods = [PolicyGaussian(MLP(in_dim, list(hidden), act), 6), Value(MLP(in_dim, list(hidden), act)), Discriminator(MLP(in_dim, list(hidden), act))]
    return mods, [mods[0].action_mean, mods[1].value_head, mods[2].logic]


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_cpu_heads_return_head_of_net(act):
    mods, heads = _heads(act, 11, (7, 5), seed=0)
    x = torch.randn(5, 11)
    with torch.no_grad():
        for m, head, fn in zip(mods, heads, CALLS):
            out = fn(m, x)
            assert out.shape == (5, head.out_features) and torch.equal(out, head(m.net(x)))


def _inputs():
    torch.manual_seed(2)                 # (host generator: the same operands wherever the test runs)
    ctx2d, state, idx = torch.randn(N_CTX, H), torch.randn(N_ROWS, S), torch.randperm(N_CTX)[:N_ROWS].contiguous()
    return ctx2d.cuda(), state.cuda(), idx.cuda()


def _min_abs_preactivation(net, x):
    lo = float("inf")
    with torch.no_grad():
        for layer in net.affine_layers:
            pre = layer(x)
            lo, x = min(lo, float(pre.abs().min())), net.activation(pre)
    return lo


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _grads(m, c):
    return [c.grad] + [p.grad for k, p in m.named_parameters() if k != "action_log_std"]


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_gathered_and_tagged_inputs_are_the_same_products(act, monkeypatch):
    from egopose_amd import gemm as G
    monkeypatch.setenv("EGP_GEMM_WS", "1")
    monkeypatch.setenv("EGP_GEMM_TERMS", "6")
    monkeypatch.delenv("EGP_GEMM", raising=False)
    assert G.fused_gather_available(H, HIDDEN[0], S)
    mods, heads = _heads(act, H + S, HIDDEN, seed=1)
    ctx2d, state, idx = _inputs()
    unused = torch.ones(N_CTX, dtype=torch.bool, device="cuda")
    unused[idx] = False
    for m, head, fn in zip(mods, heads, CALLS):
        m.cuda()
        w = torch.randn(N_ROWS, head.out_features).cuda()
        # float64 autograd of a copy of the module (float64 takes the plain path: nn.Linear)
        m64 = copy.deepcopy(m).double()
        c64 = ctx2d.double().requires_grad_(True)
        x64 = torch.cat((c64.index_select(0, idx), state.double()), 1)
        if act == "relu":
            assert _min_abs_preactivation(m64.net, x64.detach()) > KINK, "test input: a pre-activation too close to the relu's kink"
        out64 = fn(m64, x64)
        (out64 * w.double()).sum().backward()
        out64, ref = out64.detach(), _grads(m64, c64)

        c1 = ctx2d.clone().requires_grad_(True)
        out1 = fn(m, G.GatheredInput(c1, idx, state))
        (out1 * w).sum().backward()
        got1 = _grads(m, c1)
        m.zero_grad(set_to_none=True)

        c2 = ctx2d.clone().requires_grad_(True)
        x2 = G.GatheredInput(c2, idx, state).materialize()
        x2._egp_ctx_cols = H
        out2 = fn(m, x2)
        (out2 * w).sum().backward()
        got2 = _grads(m, c2)

        print("  %s %s: out %.2e  grads %s" % (act, type(m).__name__, _rel(out1.detach(), out64), " ".join("%.2e" % _rel(a, r) for a, r in zip(got1, ref))))
        assert out1.shape == out64.shape and torch.equal(out1, out2)
        assert len(got1) == len(got2) == len(ref) == 1 + 2 * (len(HIDDEN) + 1)
        for a, b in zip(got1, got2):
            assert a is not None and torch.equal(a, b)
        assert float(c1.grad[unused].abs().max()) == 0.0
        assert _rel(out1.detach(), out64) < 2e-5
        for a, r in zip(got1, ref):
            assert a.shape == r.shape and _rel(a, r) < 5e-5, (tuple(r.shape), _rel(a, r))
