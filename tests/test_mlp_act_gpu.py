"""`gemm.MlpHead` / `gemm.GatherMlpHead` with tanh and with sigmoid hidden layers against float64 autograd of the same module:
the output, the input gradient (context columns only, zeros elsewhere), every dW and db.

Shapes: context width H = 128, S = 32 state columns, hidden (36, 20), heads of 6 outputs and of 1, n = 131 rows (one 128-row
tile and a ragged second one), distinct indices into 150 context rows. The one-output head puts k_gemv_rows (its forward) and
k_rank1 (its data gradient, K = 1, with the derivative mask) on the path; GatherMlpHead puts a_rows / a2 (first layer),
b_krows / b2 (its weight gradient) and c_rows (its data gradient) on the path.

Tolerances: those of the relu forms in tests/test_gemm_gpu.py where no activation-derivative flip is in the way (tanh and
sigmoid have none): 2e-5 on the output, 5e-5 on every gradient, relative in the Frobenius norm.

And the gate: `gemm.mlp_head_available` accepts the three activations of models/mlp.py, and a tanh / sigmoid actor, critic
and discriminator run their update-path forward and backward without entering `nn.Linear.forward`.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, S, HIDDEN, N_ROWS, N_CTX = 128, 32, (36, 20), 131, 150
ACTS = {"tanh": torch.tanh, "sigmoid": torch.sigmoid}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _modules(act, head_dim, seed):
    from egopose_amd.nets import MLP
    torch.manual_seed(seed)
    net = MLP(H + S, list(HIDDEN), act).cuda()
    head = torch.nn.Linear(HIDDEN[-1], head_dim).cuda()
    net64, head64 = MLP(H + S, list(HIDDEN), act).cuda().double(), torch.nn.Linear(HIDDEN[-1], head_dim).cuda().double()
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    head64.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    return net, head, net64, head64


def _inputs(head_dim, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ctx2d = torch.randn(N_CTX, H, device="cuda", generator=g)
    state = torch.randn(N_ROWS, S, device="cuda", generator=g)
    idx = torch.randperm(N_CTX, device="cuda", generator=g)[:N_ROWS].contiguous()
    w = torch.randn(N_ROWS, head_dim, device="cuda", generator=g)
    return ctx2d, state, idx, w


def _reference(net64, head64, ctx2d, state, idx, w):
    c64 = ctx2d.double().requires_grad_(True)
    x64 = torch.cat((c64.index_select(0, idx), state.double()), 1)
    x64.retain_grad()
    out64 = head64(net64(x64))
    (out64 * w.double()).sum().backward()
    return out64.detach(), c64.grad, x64.grad, [p.grad for p in list(net64.parameters()) + list(head64.parameters())]


@pytest.mark.parametrize("head_dim", [6, 1])
@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_mlp_head_matches_float64_autograd(act, head_dim):
    from egopose_amd import gemm as G
    net, head, net64, head64 = _modules(act, head_dim, seed=1)
    ctx2d, state, idx, w = _inputs(head_dim, seed=2)
    out64, _, dx64, dp64 = _reference(net64, head64, ctx2d, state, idx, w)
    x = torch.cat((ctx2d[idx], state), 1).requires_grad_(True)
    assert G.mlp_head_available(x, net.affine_layers, head, ACTS[act])
    out = G.mlp_head(x, net.affine_layers, head, n_grad_cols=H, activation=ACTS[act])
    (out * w).sum().backward()
    print("  %s head %d: out %.2e  dx %.2e  params %s" % (act, head_dim, _rel(out.detach(), out64), _rel(x.grad[:, :H], dx64[:, :H]),
                                                         " ".join("%.2e" % _rel(p.grad, r) for p, r in zip(list(net.parameters()) + list(head.parameters()), dp64))))
    assert _rel(out.detach(), out64) < 2e-5
    assert float(x.grad[:, H:].abs().max()) == 0.0 and _rel(x.grad[:, :H], dx64[:, :H]) < 5e-5
    for p, r in zip(list(net.parameters()) + list(head.parameters()), dp64):
        assert p.grad.shape == r.shape and _rel(p.grad, r) < 5e-5, (tuple(r.shape), _rel(p.grad, r))


@pytest.mark.parametrize("head_dim", [6, 1])
@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_gather_mlp_head_matches_float64_autograd(act, head_dim, monkeypatch):
    from egopose_amd import gemm as G
    monkeypatch.setenv("EGP_GEMM_WS", "1")
    assert G.fused_gather_available(H, HIDDEN[0], S)
    net, head, net64, head64 = _modules(act, head_dim, seed=3)
    ctx2d, state, idx, w = _inputs(head_dim, seed=4)
    out64, dctx64, _, dp64 = _reference(net64, head64, ctx2d, state, idx, w)
    c = ctx2d.clone().requires_grad_(True)
    out = G.gather_mlp_head(G.GatheredInput(c, idx, state), net.affine_layers, head, ACTS[act])
    (out * w).sum().backward()
    print("  %s head %d: out %.2e  dctx %.2e  params %s" % (act, head_dim, _rel(out.detach(), out64), _rel(c.grad, dctx64),
                                                           " ".join("%.2e" % _rel(p.grad, r) for p, r in zip(list(net.parameters()) + list(head.parameters()), dp64))))
    assert _rel(out.detach(), out64) < 2e-5
    unused = torch.ones(N_CTX, dtype=torch.bool, device="cuda")
    unused[idx] = False
    assert float(c.grad[unused].abs().max()) == 0.0 and _rel(c.grad, dctx64) < 5e-5
    for p, r in zip(list(net.parameters()) + list(head.parameters()), dp64):
        assert p.grad.shape == r.shape and _rel(p.grad, r) < 5e-5, (tuple(r.shape), _rel(p.grad, r))
    # the two-node form (GatherConcat + MlpHead) is the same products in the same order
    c2 = ctx2d.clone().requires_grad_(True)
    for p in list(net.parameters()) + list(head.parameters()):
        p.grad = None
    out2 = G.mlp_head(G.GatherConcat.apply(c2, idx, state), net.affine_layers, head, H, ACTS[act])
    (out2 * w).sum().backward()
    assert torch.equal(out2, out) and torch.equal(c2.grad, c.grad)


def test_every_activation_of_the_config_takes_the_hip_path():
    from egopose_amd import gemm as G
    from egopose_amd.nets import MLP
    x = torch.zeros(4, H + S, device="cuda")
    for act in (torch.relu, torch.tanh, torch.sigmoid):
        net = MLP(H + S, list(HIDDEN), {torch.relu: "relu", torch.tanh: "tanh", torch.sigmoid: "sigmoid"}[act]).cuda()
        head = torch.nn.Linear(HIDDEN[-1], 6).cuda()
        assert net.activation is act and G.mlp_head_available(x, net.affine_layers, head, act)
    assert not G.mlp_head_available(x, net.affine_layers, head, torch.nn.functional.gelu)
    assert not G.mlp_head_available(x, net.affine_layers, head, None)


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_heads_run_without_nn_linear(act, monkeypatch):
    """PolicyGaussian.mean_std, Value.forward and Discriminator.logits on a tanh / sigmoid net, for a GatheredInput and for a
    plain tensor, forward and backward, with nn.Linear.forward patched to raise."""
    from egopose_amd import gemm as G
    from egopose_amd.nets import MLP, Discriminator, PolicyGaussian, Value
    monkeypatch.setenv("EGP_GEMM_WS", "1")
    torch.manual_seed(5)
    mods = [PolicyGaussian(MLP(H + S, list(HIDDEN), act), 6).cuda(), Value(MLP(H + S, list(HIDDEN), act)).cuda(),
            Discriminator(MLP(H + S, list(HIDDEN), act)).cuda()]
    calls = [lambda x: mods[0].mean_std(x)[0], lambda x: mods[1](x), lambda x: mods[2].logits(x)]
    ctx2d, state, idx, _ = _inputs(1, seed=6)
    want = []
    for fn in calls:                                     # the library path of the same modules, for comparison
        want.append(fn_torch(fn, mods, ctx2d, state, idx, monkeypatch))

    def refuse(self, x):
        raise AssertionError("nn.Linear.forward entered: the %s MLP left the HIP path" % act)
    monkeypatch.setattr(torch.nn.Linear, "forward", refuse)
    for fn, ref in zip(calls, want):
        c = ctx2d.clone().requires_grad_(True)
        out = fn(G.GatheredInput(c, idx, state))
        out.sum().backward()
        assert _rel(out.detach(), ref) < 2e-5 and bool(torch.isfinite(c.grad).all()) and float(c.grad.abs().sum()) > 0
        x = torch.cat((ctx2d[idx], state), 1).requires_grad_(True)
        out = fn(x)
        out.sum().backward()
        assert _rel(out.detach(), ref) < 2e-5 and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().sum()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for m in mods for k, p in m.named_parameters() if k != "action_log_std")


def fn_torch(fn, mods, ctx2d, state, idx, monkeypatch):
    """fn on the materialised input with every product on the library path (EGP_GEMM=torch), in float64 modules' stead: float32."""
    with monkeypatch.context() as mp:
        mp.setenv("EGP_GEMM", "torch")
        with torch.no_grad():
            return fn(torch.cat((ctx2d[idx], state), 1)).double()
