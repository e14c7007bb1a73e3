"""The tanh / sigmoid epilogues of `egp_gemm_f32` (`egp_gemm_desc.act_kind` / `mask_kind`, csrc/egp_gemm.hip) against float64,
in each of the four kernels that have an epilogue, in the manner of tests/test_gemm_reference_gpu.py: operands rounded to
float32, product and epilogue in float64 on the device; nothing of the reference goes through egopose_amd.gemm.

  forward     C = act(A B + bias)                 act_kind 1 tanh, 2 sigmoid
  derivative  C = (A B + bias) * f(m)             mask_kind 1: f = 1 - m^2, 2: f = m (1 - m), m = mask[r][c] (a layer's saved
                                                  OUTPUT). The reference multiplies the float64 product by f computed in
                                                  float64 from the same float32 m -- not from a pre-activation.

Cases (M, N, K) and the kernel each reaches by the launcher's dispatch (terms = 6, EGP_GEMM_WS = 1; confirmed with
torch.profiler in test_profiler_sees_the_expected_kernels). The row tile is 128 rows, column tiles are 64 (N <= 64) or 128 wide:
  k_gemm_ws     needs K >= 32 and N % 4 == 0 (16-byte rows), so its edge tiles are N = 36 and N = 132, not a multiple of
                the column tile:      (5, 36, 64)   (131, 36, 64)   (517, 132, 243)
  k_gemm_bf16x  N % 4 != 0, or K < 32:  (5, 33, 6)   (131, 6, 64)   (131, 36, 6)   (517, 130, 243)
  k_gemv_rows   N = 1, A as (M, K):     (5, 1, 243)   (131, 1, 64)   (517, 1, 6)
  k_rank1       K = 1:                  (5, 130, 1)   (131, 6, 1)   (517, 33, 1)
Every case runs both activations and both derivative kinds, without and with bias; M = 5 / 131 / 517 are below one row tile,
one tile and a ragged second one, four tiles and a ragged fifth one.

Tolerance (derived; E_DIRECT = 8e-7 and E_THIN = 3e-7 are the elementwise bounds tests/test_gemm_reference_gpu.py holds the
pre-activation products to, relative to mag = |A| @ |B| + |bias|):
  forward     |got - ref| <= L * E * mag + E_ACT      L = 1 (tanh is 1-Lipschitz), 1/4 (sigmoid is 1/4-Lipschitz)
  derivative  |got - ref| <= E * mag * |f| + 3 * 2^-24 * |ref|      (one fmaf and one multiply on top of the product)
E_ACT, the activation's own float32 error: measured on the MI355X as max |act_f32(v) - act_f64(v)| over the float32-rounded
pre-activations v of every case of this file (test_activation_error_is_within_e_act, which evaluates the device functions
alone through an exact K = 1 product, 330 334 values in [-6.23, 9.66]): tanh 7.94e-8, sigmoid 8.63e-8, the same through
k_gemv_rows and k_rank1; the larger one doubled (1.73e-7) and rounded up -> E_ACT = 2e-7 for both.

Saturation: pre-activations of +-20 and +-100 give finite outputs, tanh exactly +-1, sigmoid exactly 1 at +20 / +100 and
exactly 0 at -100; with those outputs as the mask the derivative is exactly 0. sigmoid(-20) = 2.06e-9 is a normal float32
number, so there the output is held to 4 ulp of the float64 value instead of to 0, and its derivative to the derivative bound.

Self-check (test_tolerance_tells_a_wrong_answer, float64 on the CPU, no kernel): a wrong answer misses the tolerance by at
least SELF_MARGIN = 3: (a) the gate m > 0 in place of 1 - m^2, (b) 1 - m in place of 1 - m^2, (c) the activation applied
before the bias, (d) sigmoid's factor for a tanh layer.
"""
import ctypes

import pytest
import torch

from test_gemm_reference_gpu import E_DIRECT, E_THIN, SENTINEL, _gen, _kernels_of

gpu = pytest.mark.gpu

E_ACT = 2e-7
SELF_MARGIN = 3.0
LIPSCHITZ = {"tanh": 1.0, "sigmoid": 0.25}
CASES = [("k_gemm_ws", 5, 36, 64), ("k_gemm_ws", 131, 36, 64), ("k_gemm_ws", 517, 132, 243),
         ("k_gemm_bf16x", 5, 33, 6), ("k_gemm_bf16x", 131, 6, 64), ("k_gemm_bf16x", 131, 36, 6), ("k_gemm_bf16x", 517, 130, 243),
         ("k_gemv_rows", 5, 1, 243), ("k_gemv_rows", 131, 1, 64), ("k_gemv_rows", 517, 1, 6),
         ("k_rank1", 5, 130, 1), ("k_rank1", 131, 6, 1), ("k_rank1", 517, 33, 1)]
IDS = ["%s-%dx%dx%d" % c for c in CASES]


@pytest.fixture(autouse=True)
def persistent_kernel_on(monkeypatch):
    monkeypatch.setenv("EGP_GEMM_WS", "1")
    monkeypatch.setenv("EGP_GEMM", "hip")


def _e_product(kernel):
    return E_THIN if kernel in ("k_gemv_rows", "k_rank1") else E_DIRECT


def _act64(z, act):
    return torch.tanh(z) if act == "tanh" else torch.sigmoid(z)


def _factor64(m, kind):
    m = m.double()
    return 1.0 - m * m if kind == "tanh" else m * (1.0 - m)


def _case(M, N, K, seed, device="cuda"):
    """float32 operands of a forward product (A (M, K), W (N, K)) and of a data-gradient product (A (M, K), Wt (K, N)), a bias,
    and a mask of layer outputs in (-1, 1); float64 pre-activations z = A W^T and their magnitudes."""
    g = _gen(seed, device)
    A = torch.randn(M, K, device=device, generator=g)
    W = torch.randn(N, K, device=device, generator=g) / max(K, 1) ** 0.5       # pre-activations of order 1, as a layer's
    bias = torch.randn(N, device=device, generator=g)
    pre = torch.randn(M, N, device=device, generator=g)
    z = A.double() @ W.double().t()
    mag = A.double().abs() @ W.double().abs().t()
    return A, W, bias, pre, z, mag


def _report(what, got, ref, tol):
    d = (got.double() - ref).abs()
    worst = float((d / tol).max())
    print("  %-64s max |diff| %.2e  worst diff / tol %.3f" % (what, float(d.max()), worst))
    return bool(torch.isfinite(got).all()) and worst <= 1.0


@gpu
@pytest.mark.parametrize("kernel,M,N,K", CASES, ids=IDS)
def test_forward_activation_matches_float64(kernel, M, N, K):
    """C = act(A W^T + bias) into a column slice of a wider tensor whose other columns keep their sentinel."""
    from egopose_amd.gemm import gemm
    A, W, bias, _, z, mag = _case(M, N, K, seed=M + N + K)
    E = _e_product(kernel)
    for act in ("tanh", "sigmoid"):
        for use_bias in (False, True):
            b = bias if use_bias else None
            zb, mg = (z + bias.double(), mag + bias.double().abs()) if use_bias else (z, mag)
            ref = _act64(zb, act)
            tol = LIPSCHITZ[act] * E * mg + E_ACT
            wide, lo = torch.full((M, N + 11), SENTINEL, device="cuda"), 3      # (rows need 4-byte alignment only)
            gemm(A, W, True, True, bias=b, act=act, terms=6, out=wide[:, lo:lo + N])
            assert bool((wide[:, :lo] == SENTINEL).all()) and bool((wide[:, lo + N:] == SENTINEL).all()), "guard columns were written"
            assert _report("%s %dx%dx%d %s bias=%d" % (kernel, M, N, K, act, use_bias), wide[:, lo:lo + N], ref, tol), (kernel, act, use_bias)


@gpu
@pytest.mark.parametrize("kernel,M,N,K", CASES, ids=IDS)
def test_derivative_factor_matches_float64(kernel, M, N, K):
    """C = (A Wt + bias) * f(m): the data-gradient form (B given as (K, N)), m = float32 outputs of the activation."""
    from egopose_amd.gemm import gemm
    A, W, bias, pre, z, mag = _case(M, N, K, seed=2 * (M + N + K) + 1)
    Wt = W.t().contiguous()
    E = _e_product(kernel)
    for kind in ("tanh", "sigmoid"):
        m = _act64(pre.double(), kind).float()                                  # what the forward pass saved
        wide_m = torch.full((M, N + 5), 0.5, device="cuda")
        wide_m[:, 2:2 + N] = m
        f = _factor64(m, kind)
        for use_bias in (False, True):
            b = bias if use_bias else None
            zb, mg = (z + bias.double(), mag + bias.double().abs()) if use_bias else (z, mag)
            ref = zb * f
            tol = E * mg * f.abs() + 3 * 2.0 ** -24 * ref.abs() + 1e-300
            got = gemm(A, Wt, True, False, bias=b, mask=wide_m[:, 2:2 + N], mask_kind=kind, terms=6)
            assert _report("%s %dx%dx%d d%s bias=%d" % (kernel, M, N, K, kind, use_bias), got, ref, tol), (kernel, kind, use_bias)


@gpu
def test_linear_helpers_map_an_activation_to_the_kinds():
    """linear_fwd(act=) / linear_dgrad(mask=, act=) are the same launches; relu through `act` is the relu field and the gate."""
    from egopose_amd.gemm import gemm, linear_dgrad, linear_fwd
    A, W, bias, pre, _, _ = _case(131, 36, 64, seed=5)
    for act, fn in (("tanh", torch.tanh), ("sigmoid", torch.sigmoid), ("relu", torch.relu)):
        assert torch.equal(linear_fwd(A, W, bias, act=fn), gemm(A, W, bias=bias, act=act, relu=(act == "relu")))
        dy = torch.randn(131, 36, device="cuda", generator=_gen(6))
        Wn = torch.randn(36, 64, device="cuda", generator=_gen(7))
        m = fn(torch.randn(131, 64, device="cuda", generator=_gen(8)))         # the (M, N) output of the layer below
        assert torch.equal(linear_dgrad(dy, Wn, mask=m, act=act), gemm(dy, Wn, True, False, mask=m, mask_kind=act))
    assert torch.equal(linear_fwd(A, W, bias, act="relu"), linear_fwd(A, W, bias, relu=True))
    assert torch.equal(linear_dgrad(dy, Wn, mask=m), linear_dgrad(dy, Wn, mask=m, act="relu"))
    with pytest.raises(ValueError):
        gemm(A, W, bias=bias, relu=True, act="tanh")
    with pytest.raises(ValueError):
        gemm(A, W, mask_kind="tanh")
    with pytest.raises(ValueError):
        gemm(A, W, act="gelu")


def _pre_activations():
    """The float32-rounded pre-activations of every forward case of this file, with and without bias, in one vector."""
    vs = []
    for kernel, M, N, K in CASES:
        _, _, bias, _, z, _ = _case(M, N, K, seed=M + N + K)
        vs += [z.float().flatten(), (z + bias.double()).float().flatten()]
    return torch.cat(vs)


@gpu
def test_activation_error_is_within_e_act():
    """The device functions alone: a K = 1 product v * 1 is exact, so the result is act_f32(v). Twice the measured error must
    stay within E_ACT (the figure in this file's docstring is what this printed on the MI355X)."""
    from egopose_amd.gemm import gemm
    v = _pre_activations().unsqueeze(1).contiguous()
    one = torch.ones(1, 1, device="cuda")
    for act in ("tanh", "sigmoid"):
        for kernel, got in (("k_gemv_rows", gemm(v, one, True, True, act=act, terms=6)),
                            ("k_rank1", gemm(v.t().contiguous(), one, False, True, act=act, terms=6))):
            err = float((got.double() - _act64(v.double(), act)).abs().max())
            print("  %s through %s over %d pre-activations in [%.2f, %.2f]: max |f32 - f64| %.3e" % (act, kernel, v.numel(), float(v.min()), float(v.max()), err))
            assert 2 * err <= E_ACT, (act, kernel, err)


@gpu
@pytest.mark.parametrize("kernel,N,K", [("k_gemm_ws", 36, 64), ("k_gemm_bf16x", 6, 64), ("k_gemv_rows", 1, 64), ("k_rank1", 6, 1)])
def test_saturated_pre_activations(kernel, N, K):
    """Pre-activations of exactly +-20 and +-100 (one non-zero product per output) in every kernel."""
    from egopose_amd.gemm import gemm
    v = torch.tensor([20.0, -20.0, 100.0, -100.0, 20.0, -100.0, 100.0, -20.0], device="cuda")
    M = v.numel()
    A = torch.zeros(M, K, device="cuda")
    A[:, K // 2] = v
    W = torch.zeros(N, K, device="cuda")
    W[:, K // 2] = 1.0
    assert _kernels_of(lambda: gemm(A, W, act="tanh", terms=6)) == {kernel}
    t = gemm(A, W, act="tanh", terms=6)
    s = gemm(A, W, act="sigmoid", terms=6)
    assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(s).all())
    assert torch.equal(t, torch.sign(v).unsqueeze(1).expand(M, N)), t
    col = v.unsqueeze(1).expand(M, N)
    assert bool((s[col >= 20] == 1.0).all()) and bool((s[col == -100] == 0.0).all()), s
    low, want = s[col == -20].double(), torch.sigmoid(torch.tensor(-20.0, dtype=torch.float64))
    assert bool(((low - want).abs() <= 4 * 2.0 ** -24 * want).all()), low
    # the derivative from those outputs: exactly 0 wherever the activation saturated
    dy = torch.randn(M, K, device="cuda", generator=_gen(3)) * 50
    Wt = torch.randn(K, N, device="cuda", generator=_gen(4))
    z = dy.double() @ Wt.double()
    dt = gemm(dy, Wt, True, False, mask=t, mask_kind="tanh", terms=6)
    ds = gemm(dy, Wt, True, False, mask=s, mask_kind="sigmoid", terms=6)
    assert bool((dt == 0).all()) and bool(torch.isfinite(ds).all())
    assert bool((ds[col != -20] == 0).all())
    f = _factor64(s, "sigmoid")
    tol = _e_product(kernel) * (dy.double().abs() @ Wt.double().abs()) * f + 3 * 2.0 ** -24 * (z * f).abs()
    assert bool(((ds.double() - z * f).abs() <= tol)[col == -20].all())


@gpu
def test_profiler_sees_the_expected_kernels():
    """Every case under torch.profiler, forward and derivative: the kernel the case names runs and no other."""
    from egopose_amd.gemm import gemm
    for kernel, M, N, K in CASES:
        A, W, bias, pre, _, _ = _case(M, N, K, seed=1)
        Wt, m = W.t().contiguous(), torch.tanh(pre)
        assert _kernels_of(lambda: gemm(A, W, bias=bias, act="sigmoid", terms=6)) == {kernel}, (kernel, M, N, K)
        assert _kernels_of(lambda: gemm(A, Wt, True, False, mask=m, mask_kind="tanh", terms=6)) == {kernel}, (kernel, M, N, K)


def _desc(L, a_t, b_t, out, **kw):
    d = L.GemmDesc()
    d.M, d.N, d.K = out.shape[0], out.shape[1], a_t.shape[1]
    d.A, d.lda, d.a_kcontig = a_t.data_ptr(), a_t.shape[1], 1
    d.B, d.ldb, d.b_kcontig = b_t.data_ptr(), b_t.shape[1], 1
    d.C, d.ldc = out.data_ptr(), out.shape[1]
    d.terms, d.splits = 6, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@gpu
def test_refusals_write_nothing():
    """relu together with act_kind, a kind outside 0..2, mask_kind without mask, either kind on a split-K or bias-gradient
    launch: EGP_E_INVALID with a worded message, `out` untouched. A zero-filled tail is today's product."""
    from egopose_amd import _lib as L
    g = _gen(8)
    A, B = torch.randn(200, 64, device="cuda", generator=g), torch.randn(128, 64, device="cuda", generator=g)
    Bt = B.t().contiguous()                                   # (K, N) for the launches with a bias-gradient column
    mask = torch.rand(200, 128, device="cuda", generator=g)
    out = torch.full((200, 128), SENTINEL, device="cuda")
    ws = torch.zeros(4 * 200 * 132, device="cuda")
    bg = torch.full((200,), SENTINEL, device="cuda")
    lib = L.load()
    mk = dict(mask=mask.data_ptr(), ldmask=128)
    split = dict(splits=2, workspace=ws.data_ptr())
    ones = dict(b_kcontig=0, B=Bt.data_ptr(), ldb=128, bias_grad=bg.data_ptr(), workspace=ws.data_ptr())
    refused = [(dict(relu=1, act_kind=1), b"relu"), (dict(relu=1, act_kind=2), b"relu"),
               (dict(act_kind=3), b"act_kind"), (dict(act_kind=-1), b"act_kind"),
               (dict(mask_kind=3, **mk), b"mask_kind"), (dict(mask_kind=-1, **mk), b"mask_kind"),
               (dict(mask_kind=1), b"mask_kind needs a mask"), (dict(mask_kind=2), b"mask_kind needs a mask"),
               (dict(act_kind=1, **split), b"no epilogue on split-K"), (dict(mask_kind=2, **mk, **split), b"no epilogue on split-K"),
               (dict(act_kind=2, **ones), b"no epilogue on split-K"), (dict(mask_kind=1, **mk, **ones), b"no epilogue on split-K")]
    for kw, word in refused:
        rc = lib.egp_gemm_f32(ctypes.byref(_desc(L, A, B, out, **kw)), L.current_stream())
        assert rc == -1, kw                                    # EGP_E_INVALID
        assert word in lib.egp_last_error(), (kw, lib.egp_last_error())
        with pytest.raises(ValueError):
            L.check(rc, "egp_gemm_f32")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((bg == SENTINEL).all())
    L.check(lib.egp_gemm_f32(ctypes.byref(_desc(L, A, B, out)), L.current_stream()), "egp_gemm_f32")       # the tail zero-filled
    ref = A.double() @ B.double().t()
    assert float((out.double() - ref).norm() / ref.norm()) < 1e-6
    L.check(lib.egp_gemm_f32(ctypes.byref(_desc(L, A, B, out, act_kind=1, mask_kind=2, **mk)), L.current_stream()), "egp_gemm_f32")
    want = torch.tanh(ref) * _factor64(mask, "sigmoid")
    assert float((out.double() - want).abs().max()) < 1e-5


def test_tolerance_tells_a_wrong_answer():
    """float64 on the CPU, no kernel: each modelled fault misses this file's tolerance by at least SELF_MARGIN."""
    M, N, K = 131, 36, 64
    A, W, bias, pre, z, mag = _case(M, N, K, seed=11, device="cpu")
    zb, mg = z + bias.double(), mag + bias.double().abs()
    margins = {}
    for E, name in ((E_DIRECT, "tile"), (E_THIN, "thin")):
        m = torch.tanh(pre.double()).float()
        f = _factor64(m, "tanh")
        ref = zb * f
        tol = E * mg * f.abs() + 3 * 2.0 ** -24 * ref.abs()
        miss = lambda wrong: float(((wrong - ref).abs() / tol).max())
        margins["a gate for 1 - m^2, " + name] = miss(zb * (m > 0))
        margins["b 1 - m for 1 - m^2, " + name] = miss(zb * (1.0 - m.double()))
        margins["d sigmoid's factor for tanh, " + name] = miss(zb * _factor64(m, "sigmoid"))
        for act in ("tanh", "sigmoid"):
            ref = _act64(zb, act)
            tol = LIPSCHITZ[act] * E * mg + E_ACT
            margins["c %s before the bias, %s" % (act, name)] = float(((_act64(z, act) + bias.double() - ref).abs() / tol).max())
    print("\n  self-check margins: " + ", ".join("%s %.0fx" % kv for kv in sorted(margins.items())))
    low = {k: v for k, v in margins.items() if not v >= SELF_MARGIN}
    assert not low, low
