"""`egp_policy_step_f32` and `egp_mlp_pack_f32` (csrc/egp_policy.hip) against an independent float64 statement of one
launch, at the forms, widths and row tiles that the drivers' tests (all at 128 + 115 -> 300 -> 200 -> 52 or 13 -> 10 -> 6
-> 4) do not reach.

Reference (`policy_ref`): the launch as include/egopose_hip.h (`egp_policy_desc`) states it -- gather
ctx_rows[r*stride + t_idx[r]*ctx_dim ...], concatenate float(state), `W x + b` per layer with the activation on all but
the last, mean and action = mean + exp(log_std) * noise; with a cell one LSTMCell step (gates i, f, g, o) in front and
[ctx | h'] into the layers; with `vlayers` the second chain to the value. float64 on the CPU from float32 operands drawn
from seeded host generators; nothing of egopose_amd.policy_step or egopose_amd.nets is used, and every launch goes
through a `_lib.PolicyDesc` / `_lib.MlpLayer` filled in here. The same function in float32 is the yardstick of part 2.

Part 0, the packed form: `egp_mlp_pack_f32` == packed[((g*ceil(in/4)+kq)*64+c)*4+kk] = W[64g+c][4kq+kk], zero outside,
for (in, out) = (1, 1), (6, 52), (243, 300), (13, 65), dense and as a column slice (ldw > in_dim), into a destination
prefilled with a sentinel.

Part 1, exact (ReLU; context, state and noise integers in [-3, 3], weights in {-1, 0, 1} with a quarter non-zero, integer
biases in [-2, 2], log_std = 0): every product and partial sum is an exactly representable float32 (each case asserts
|W| |x| + |b| < 2^24 on the reference), so mean_out and action must equal float64 bit for bit, with noise and without
(action == mean), with mean_out and with mean_out = NULL; rows >= n of outputs three rows longer keep their canary.
Which case reaches which path of the kernel (PLAIN below, 4 rows per workgroup, 4 waves, passes of 5 x 64 columns):
  own-column staging (padded input <= 256)  in128+115 (a wave straddling context and state), in64+192 (256 exactly),
                                            in3+1 (one input quad: three waves with an empty k share), in5+8 (state starts
                                            at an unaligned column), in0+7 (no context), in100+0 (no state)
  strided staging, state branch (> 256)     in130+127 (257), in192+115 (307, T = 3, padded row stride)
  small-operand tail loop (> 1024 floats)   small-tail: 5 + 8 -> 512 -> 400 -> 52 with noise, 964 + 52 + 208 = 1224 floats
  dynamic LDS above 64 KiB                  lds-1344 (70500 bytes), lds-2048 (95844 bytes); see "LDS" below
  last layer of two column groups           out65 (and out1, out4, out64: one group, ragged and full)
  hidden width against the 320-column pass  h64 (one-group pass), h65 (pad quad zeroed for the next layer), h192, h256 (3, 4
                                            groups), h320 (5 groups, one pass), h321 (second pass of one column), h641 (three)
  depth 1, depth 8                          depth1 (output layer only), depth8 (seven 64-wide hidden layers)
  n = 1, 4, 5, 33                           n1 (ragged tile), n4 (full), n5-T3 (second tile ragged), n33 (nine workgroups: the
                                            L2 warm-up's second slice)
  T = 3, ctx_row_stride = T*ctx_dim + 8     n5-T3 and in192+115: t_idx hits 0 and T - 1, the pad columns hold NaN
  warm_lines = 0                            separate: every layer's packed weights in an allocation of its own, not adjacent
  actor + critic (`vlayers`)                v-head-only (critic depth 1, vactivation != activation, n = 1), v-deep (critic depth
                                            4 ReLU beside a tanh actor of depth 2: value exact, actor in part 2's tolerance),
                                            v-noctx (vctx_dim = 0), v-wide (vctx_dim = 320 beside ctx_dim = 5: the critic's
                                            carve-up is the larger one, and its workgroups stage strided while the actor's
                                            own columns), n = 1 and 6; the actor's outputs == the plain step's bits
  forecast (`cell`)                         Hs 1 / S 1 / no context with NULL ctx_rows and t_idx / n 1; Hs 7 / S 5 / ctx 5 / n 9;
                                            Hs 80 (gates end on a pass), 81 (one unit past it), 512 (maximum) at n = 5; Hs 128 /
                                            S 115 / ctx 128 / n 9; hc_row_stride = Hs + 3 with sentinel columns. h', c' against the
                                            float64 cell in part 2's tolerance; then mean_out and action == the plain step's bits
                                            on (ctx, state = the kernel's own h').

LDS: the policy kernels never raise hipFuncAttributeMaxDynamicSharedMemorySize. On the MI355X the launches with 70500 and
95844 bytes of dynamic LDS (lds-1344, lds-2048) were observed to be ACCEPTED as they stand and to compute the exact result,
so the launch code is left as it is; a refusal would come back from these two cases as EGP_E_HIP, not as a fault.

Part 2, rounding (normal operands, weights scaled by 1/sqrt(in); ReLU, tanh, sigmoid), n = 9. Two figures per output, as
tests/test_gemm_reference_gpu.py and tests/test_tcn_reference_gpu.py:
  rel  = |got - ref| / |ref| (Frobenius)    against  max(C_POL x rel of the yardstick, FLOOR), FLOOR = 2e-7
  elem = max |got - ref| / mag              against  E_POL
mag = the last layer's |W| |a| + |b| on the reference's activations (mean, action, value), 1 for h and c.
The yardstick is `policy_ref` in float32 on the same operands. Measured on the MI355X (rel of the kernel, of the yardstick,
their ratio; elem; ratios of comparisons under FLOOR are in brackets: there the floor decides):
  shipped 243 -> 300 -> 200 -> 52, ReLU    mean   2.17e-7  2.92e-7  0.74   1.07e-7    action 1.81e-7  2.44e-7  (0.74)  1.03e-7
  307 -> 330 -> 6 -> 4, tanh               mean   1.39e-7  2.10e-7  (0.66) 2.45e-7    action 1.32e-7  2.12e-7  (0.63)  2.31e-7
  forecast 115 / 128 / 128                 h      1.35e-7  1.57e-7  (0.86) 2.11e-7    c      1.17e-7  1.28e-7  (0.92)  4.13e-7
                                           mean   1.53e-7  2.03e-7  (0.75) 8.31e-8    action 1.18e-7  1.50e-7  (0.79)  8.54e-8
  critic at the shipped widths, sigmoid    value  7.72e-8  2.44e-7  (0.32) 1.41e-8    (mean, action: the shipped row's bits)
  part 1, held to the same tolerance       v-deep mean (1.23) 9.67e-8, action (1.21) 1.01e-7; forecast h', c' worst at Hs 512:
                                           h (1.14) 4.07e-7, c (1.10) 7.37e-7 (|c| reaches 4 while its magnitude is taken as 1);
                                           Hs 128: c 5.12e-7; Hs 1 .. 81: ratios 0.88 .. 1.10, elem <= 2.7e-7
    -> C_POL = 3 (2 x 1.23, rounded up), E_POL = 1.5e-6 (2 x 7.37e-7, rounded up); every rel but one is under FLOOR = 2e-7, the
       float32 unit, where the yardstick itself is and the floor decides.

Self-check (test_tolerance_tells_a_wrong_answer, float64 on the CPU, no kernel, n = 9, T = 3): a wrong answer must miss the
tolerance by SELF_MARGIN = 3 in rel or elem of mean or action. At the shipped shape: (a) one input quad of one 64-column group
missing in layer 1, (b) wave 1's quarter of layer 1's k range missing for rows 4 .. 7, (d) a row's noise taken from the next
row, (e) the context row taken at t_idx + 1. (c) the biases behind a width that is no multiple of 4 read at the unrounded offset:
at 307 -> 330 -> 6 -> 4, since the shipped widths are all multiples of 4 and the fault changes nothing there.
Margins: (a) 3.0e4, (b) 1.7e5, (c) 1.4e6, (d) 9.9e5, (e) 5.5e5.
"""
import ctypes
import math

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
C_POL, E_POL = 3.0, 1.5e-6          # measured, see above
FLOOR = 2e-7
SELF_MARGIN = 3.0
CANARY = -777.25
NAN = float("nan")
MIN_NONZERO = 0.25
ACTS = {0: torch.tanh, 1: lambda v: v.clamp_min(0), 2: torch.sigmoid}
SHIPPED = (300, 200, 52)


# ------------------------------------------------------------------------------------------------------ the reference

def _gather(slab, stride, dim, t_idx, n, dtype):
    """x[r] = ctx_rows[r*stride + t_idx[r]*dim ... + dim) of the flat slab."""
    if dim == 0:
        return torch.zeros(n, 0, dtype=dtype)
    idx = (torch.arange(n) * stride + t_idx * dim)[:, None] + torch.arange(dim)[None, :]
    return slab.reshape(-1)[idx].to(dtype)


def _chain(x, layers, act, dtype):
    """-> (last layer's output, its |W| |a| + |b|, the largest |W| |x| + |b| of any layer)."""
    peak = 0.0
    for l, (W, b) in enumerate(layers):
        W, b = W.to(dtype), b.to(dtype)
        mag = x.abs() @ W.abs().t() + b.abs()
        peak = max(peak, float(mag.max()))
        x = x @ W.t() + b
        if l < len(layers) - 1:
            x = ACTS[act](x)
    return x, mag, peak


def policy_ref(slab, stride, ctx_dim, t_idx, state, layers, act=1, log_std=None, noise=None, cell=None, h=None, c=None,
               vslab=None, vstride=0, vctx_dim=0, vlayers=None, vact=1, dtype=torch.float64):
    """One launch in `dtype` -> dict(mean, action, mag, peak [, h, c] [, value, vmag]). cell = (W_ih, W_hh, b) with
    b = b_ih + b_hh, rows in torch's gate order i, f, g, o."""
    n = state.shape[0]
    s = state.float().to(dtype)                               # the kernel casts the state to float32
    out = {}
    tail = s
    if cell is not None:
        w_ih, w_hh, b = (t.to(dtype) for t in cell)
        pre = s @ w_ih.t() + h.to(dtype) @ w_hh.t() + b
        gi, gf, gg, go = pre.chunk(4, dim=1)
        c1 = torch.sigmoid(gf) * c.to(dtype) + torch.sigmoid(gi) * torch.tanh(gg)
        h1 = torch.sigmoid(go) * torch.tanh(c1)
        out["h"], out["c"] = h1, c1
        tail = h1
    x = torch.cat((_gather(slab, stride, ctx_dim, t_idx, n, dtype), tail), 1)
    mean, mag, peak = _chain(x, layers, act, dtype)
    out["mean"], out["mag"] = mean, mag
    out["action"] = mean if noise is None else mean + torch.exp(log_std.to(dtype)) * noise.to(dtype)
    if vlayers is not None:
        xv = torch.cat((_gather(vslab, vstride, vctx_dim, t_idx, n, dtype), s), 1)
        value, vmag, vpeak = _chain(xv, vlayers, vact, dtype)
        out["value"], out["vmag"] = value[:, 0], vmag[:, 0]
        peak = max(peak, vpeak)
    out["peak"] = peak
    return out


def pack_ref(W):
    """The header's packed form of W[out][in]: [g][kq][c][kk] = W[64 g + c][4 kq + kk], zero outside."""
    out_dim, in_dim = W.shape
    G, nkq = (out_dim + 63) // 64, (in_dim + 3) // 4
    full = torch.zeros(G * 64, nkq * 4, dtype=W.dtype)
    full[:out_dim, :in_dim] = W
    return full.view(G, 64, nkq, 4).permute(0, 2, 1, 3).contiguous().reshape(-1)


def lds_bytes(in0, widths):
    """Dynamic LDS of a plain launch as csrc/egp_policy.hip documents its carve-up (4 rows, 4 waves): cur | nxt | the waves'
    partial sums | biases | exp(log_std) | noise | one pad float."""
    xs = ((max((in0,) + tuple(widths)) + 31) & ~31) + 4
    out4 = (widths[-1] + 3) & ~3
    return 4 * (2 * 4 * xs + 4 * 4 * (5 * 64 + 4) + sum((w + 3) & ~3 for w in widths) + out4 + 4 * out4 + 1)


# ----------------------------------------------------------------------------------------------------------- operands

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def make_net(kind, in_dim, widths, g):
    """[(W, b)] of the layers in_dim -> widths[0] -> ... -> widths[-1]."""
    layers, prev = [], in_dim
    for w in widths:
        if kind == "int":
            W = _ints(g, -1, 1, w, prev) * (torch.rand(w, prev, generator=g) < 0.375).float()      # 2/3 x 3/8: a quarter non-zero
            b = _ints(g, -2, 2, w)
        else:
            W = torch.randn(w, prev, generator=g) / math.sqrt(prev)
            b = torch.randn(w, generator=g) * 0.3
        layers.append((W, b))
        prev = w
    return layers


def make_ctx(kind, n, T, dim, pad, g):
    """(slab, row stride): n rows of T context vectors and `pad` NaN columns; without context one unused float."""
    if dim == 0:
        return torch.zeros(1), 0
    slab = torch.full((n, T * dim + pad), NAN)
    slab[:, :T * dim] = _ints(g, -3, 3, n, T * dim) if kind == "int" else torch.randn(n, T * dim, generator=g)
    return slab, T * dim + pad


def make_ops(kind, n, ctx_dim, state_dim, widths, T=1, pad=0, seed=0):
    """Host operands of a plain step."""
    g = _gen(seed)
    o = dict(kind=kind, n=n, T=T, ctx_dim=ctx_dim, state_dim=state_dim, widths=tuple(widths))
    o["slab"], o["stride"] = make_ctx(kind, n, T, ctx_dim, pad, g)
    o["t_idx"] = (torch.arange(n) * 2) % T                    # T = 3: 0, 2, 1, 0, ...
    if kind == "int":
        o["state"] = _ints(g, -3, 3, n, state_dim).double()
        o["noise"] = _ints(g, -3, 3, n, widths[-1])
        o["log_std"] = torch.zeros(widths[-1])
    else:
        o["state"] = torch.randn(n, state_dim, generator=g, dtype=torch.float64) * 2        # not float32 numbers: the cast takes part
        o["noise"] = torch.randn(n, widths[-1], generator=g)
        o["log_std"] = torch.randn(widths[-1], generator=g) * 0.3 - 0.7
    o["layers"] = make_net(kind, ctx_dim + state_dim, widths, g)
    return o


def ref_of(o, noise=True, dtype=torch.float64, **kw):
    return policy_ref(o["slab"], o["stride"], o["ctx_dim"], o["t_idx"], o["state"], o["layers"], o.get("act", 1),
                      o["log_std"] if noise else None, o["noise"] if noise else None, dtype=dtype, **kw)


def _nonzero(t):
    return float((t != 0).double().mean())


# ------------------------------------------------------------------------------------------------------- the launches

def _lib():
    from egopose_amd import _lib as L
    return L, L.load()


def dev_layers(layers, separate=False):
    """The layers packed on the device -> (MlpLayer array, tensors to keep alive). Back to back in one allocation, as the
    kernel's L2 warm-up wants them, or `separate`: an allocation each, 256 floats longer than the packed form, so that no
    layer starts where the one before it ends (asserted). The destinations are prefilled with NaN."""
    L, lib = _lib()
    sizes = [int(lib.egp_mlp_pack_floats(W.shape[1], W.shape[0])) for W, _ in layers]
    if separate:
        dsts = [torch.full((s + 256,), NAN, device=DEV) for s in sizes]
    else:
        flat = torch.full((sum(sizes),), NAN, device=DEV)
        offs = [sum(sizes[:l]) for l in range(len(sizes))]
        dsts = [flat[a:a + s] for a, s in zip(offs, sizes)]
    arr = (L.MlpLayer * len(layers))()
    keep = [dsts]
    for l, (W, b) in enumerate(layers):
        Wd, bd = W.to(DEV).contiguous(), b.to(DEV).contiguous()
        L.check(lib.egp_mlp_pack_f32(Wd.data_ptr(), W.shape[1], W.shape[1], W.shape[0], dsts[l].data_ptr(), L.current_stream()), "egp_mlp_pack_f32")
        arr[l].wt, arr[l].bias, arr[l].in_dim, arr[l].out_dim = dsts[l].data_ptr(), bd.data_ptr(), W.shape[1], W.shape[0]
        assert dsts[l].data_ptr() % 16 == 0
        keep += [Wd, bd]
    follows = [arr[l + 1].wt == arr[l].wt + 4 * sizes[l] for l in range(len(layers) - 1)]
    assert not any(follows) if separate else all(follows)
    torch.cuda.synchronize()
    return arr, keep


def _canary(rows, *cols, dtype=torch.float32):
    return torch.full((rows,) + cols, CANARY, dtype=dtype, device=DEV)


def launch(o, noise=True, mean=True, separate=False, critic=None, cell=None, expect_ok=True):
    """One `egp_policy_step_f32` on the operands `o` through a descriptor filled in here. Outputs are three rows longer than
    n and canary-filled; rows >= n must come back untouched. critic = dict(slab, stride, ctx_dim, layers, act);
    cell = dict(W [4 Hs][S + Hs] in the header's row order, b, h, c, hs, stride, null_ctx). -> dict of CPU tensors (rows < n)."""
    L, lib = _lib()
    n, nu = o["n"], o["widths"][-1]
    key = ("dev", separate)
    if key not in o:
        o[key] = dev_layers(o["layers"], separate)
    arr, _ = o[key]
    t = lambda x: x.to(DEV).contiguous()
    slab, t_idx, state, log_std, nz = t(o["slab"]), t(o["t_idx"]), t(o["state"]), t(o["log_std"]), t(o["noise"])
    if o["state_dim"] == 0:
        state = torch.zeros(1, dtype=torch.float64, device=DEV)          # the pointer is required, nothing is read
    action, mean_out = _canary(n + 3, nu, dtype=torch.float64), _canary(n + 3, nu)
    d = L.PolicyDesc()
    d.n = n
    null_ctx = bool(cell and cell.get("null_ctx"))
    if not null_ctx:
        d.ctx_rows, d.t_idx = slab.data_ptr(), t_idx.data_ptr()
    d.ctx_row_stride, d.ctx_dim = o["stride"], o["ctx_dim"]
    d.state, d.state_dim = state.data_ptr(), o["state_dim"]
    d.layers, d.n_layers, d.activation = arr, len(o["layers"]), o.get("act", 1)
    if noise:
        d.log_std, d.noise = log_std.data_ptr(), nz.data_ptr()
    d.action = action.data_ptr()
    if mean:
        d.mean_out = mean_out.data_ptr()
    keep = []
    if critic:
        if "dev" not in critic:
            critic["dev"] = dev_layers(critic["layers"])
        vslab, value = t(critic["slab"]), _canary(n + 3)
        d.vctx_rows, d.vctx_row_stride, d.vctx_dim = vslab.data_ptr(), critic["stride"], critic["ctx_dim"]
        d.vlayers, d.n_vlayers, d.vactivation = critic["dev"][0], len(critic["layers"]), critic["act"]
        d.value_out = value.data_ptr()
    if cell:
        hs, hst = cell["hs"], cell["stride"]
        if "dev" not in cell:
            cell["dev"] = dev_layers([(cell["W"], cell["b"])])
        hb, cb = _canary(n + 3, hst), _canary(n + 3, hst)
        hb[:n, :hs], cb[:n, :hs] = t(cell["h"]), t(cell["c"])
        d.cell, d.h, d.c, d.hc_row_stride = cell["dev"][0], hb.data_ptr(), cb.data_ptr(), hst
    torch.cuda.synchronize()
    rc = lib.egp_policy_step_f32(ctypes.byref(d), L.current_stream())
    if not expect_ok:
        return rc
    L.check(rc, "egp_policy_step_f32")
    torch.cuda.synchronize()
    got = {"action": action[:n].cpu()}
    assert bool((action[n:] == CANARY).all()), "action: rows >= n were written"
    assert bool((mean_out[n:] == CANARY).all()) and (mean or bool((mean_out == CANARY).all())), "mean_out: rows >= n (or a NULL mean_out) were written"
    if mean:
        got["mean"] = mean_out[:n].cpu()
    if critic:
        assert bool((value[n:] == CANARY).all()), "value_out: rows >= n were written"
        got["value"] = value[:n].cpu()
    if cell:
        for name, buf in (("h", hb), ("c", cb)):
            assert bool((buf[n:] == CANARY).all()) and bool((buf[:, hs:] == CANARY).all()), name + ": written outside rows < n, columns < Hs"
            got[name] = buf[:n, :hs].cpu()
    return got


def assert_exact(what, o, separate=False, null_mean=False):
    """Both launches of a part-1 case equal the float64 reference bit for bit: with noise and mean_out; without noise
    (action == mean), there with mean_out = NULL when `null_mean`."""
    ref, plain = ref_of(o), ref_of(o, noise=False)
    print("  %-28s peak %.3g  nonzero %.2f  lds %d" % (what, ref["peak"], _nonzero(ref["mean"]), lds_bytes(o["ctx_dim"] + o["state_dim"], o["widths"])))
    assert ref["peak"] < 2.0 ** 24 and _nonzero(ref["mean"]) >= MIN_NONZERO
    assert torch.equal(plain["action"], ref["mean"])
    got = launch(o, separate=separate)
    assert torch.equal(got["mean"].double(), ref["mean"]), (what, "mean", int((got["mean"].double() != ref["mean"]).sum()))
    assert torch.equal(got["action"], ref["action"]), (what, "action", int((got["action"] != ref["action"]).sum()))
    assert o["widths"][-1] * o["n"] < 8 or not torch.equal(ref["action"], ref["mean"])          # (the noise took part)
    quiet = launch(o, noise=False, mean=not null_mean, separate=separate)
    assert torch.equal(quiet["action"], ref["mean"]), (what, "action without noise")
    assert null_mean or torch.equal(quiet["mean"].double(), ref["mean"])
    return got


# ------------------------------------------------------------------------------------------- part 0: the packed form

PACK_SHAPES = [(1, 1), (6, 52), (243, 300), (13, 65)]


def test_pack_ref_is_the_headers_formula():
    """`pack_ref`'s reshape against the formula written out index by index, on a shape with ragged quads and groups."""
    W = torch.arange(1, 13 * 65 + 1, dtype=torch.float32).view(65, 13)
    p = pack_ref(W)
    nkq = 4
    assert p.numel() == 2 * nkq * 256
    for g, kq, c, kk in ((0, 0, 0, 0), (0, 3, 63, 0), (0, 3, 5, 1), (1, 0, 0, 3), (1, 2, 0, 1), (1, 0, 1, 0), (0, 1, 17, 2)):
        o, i = 64 * g + c, 4 * kq + kk
        want = float(W[o, i]) if o < 65 and i < 13 else 0.0
        assert float(p[((g * nkq + kq) * 64 + c) * 4 + kk]) == want, (g, kq, c, kk)


@gpu
@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "column-slice"])
@pytest.mark.parametrize("in_dim,out_dim", PACK_SHAPES, ids=["%dto%d" % s for s in PACK_SHAPES])
def test_pack_equals_the_headers_formula(in_dim, out_dim, sliced):
    """No zero operand: a zero in the result is padding. The destination starts as a sentinel and is 64 floats longer than the
    packed form; those stay."""
    L, lib = _lib()
    g = _gen(10 + in_dim)
    W = torch.randn(out_dim, in_dim, generator=g) + 3.0 * torch.sign(torch.randn(out_dim, in_dim, generator=g))
    assert bool((W != 0).all())
    if sliced:
        wide = torch.full((out_dim, in_dim + 7), NAN)
        wide[:, 3:3 + in_dim] = W
        wd = wide.to(DEV)[:, 3:3 + in_dim]
        ldw = in_dim + 7
    else:
        wd, ldw = W.to(DEV), in_dim
    total = int(lib.egp_mlp_pack_floats(in_dim, out_dim))
    assert total == ((out_dim + 63) // 64) * ((in_dim + 3) // 4) * 256
    dst = torch.full((total + 64,), CANARY, device=DEV)
    L.check(lib.egp_mlp_pack_f32(wd.data_ptr(), ldw, in_dim, out_dim, dst.data_ptr(), L.current_stream()), "egp_mlp_pack_f32")
    torch.cuda.synchronize()
    assert torch.equal(dst[:total].cpu(), pack_ref(W)) and bool((dst[total:] == CANARY).all())


# ------------------------------------------------------------------------------------------ part 1: the plain step

# name -> (n, ctx_dim, state_dim, widths, T, pad, options)
PLAIN = {
    "n1": (1, 128, 115, SHIPPED, 1, 0, ""),
    "n4": (4, 128, 115, SHIPPED, 1, 0, "null_mean"),
    "n5-T3": (5, 128, 115, SHIPPED, 3, 8, ""),
    "n33": (33, 128, 115, SHIPPED, 1, 0, ""),
    "separate": (5, 128, 115, SHIPPED, 1, 0, "separate"),
    "in64+192-h64": (5, 64, 192, (64, 52), 1, 0, ""),
    "in130+127-h65": (5, 130, 127, (65, 52), 1, 0, "null_mean"),
    "in192+115-h192": (5, 192, 115, (192, 52), 3, 8, ""),
    "in3+1-h256": (5, 3, 1, (256, 52), 1, 0, ""),
    "in5+8-h320": (5, 5, 8, (320, 52), 3, 8, ""),
    "in0+7-h321": (5, 0, 7, (321, 52), 1, 0, ""),
    "in100+0-h641": (5, 100, 0, (641, 52), 1, 0, ""),
    "out1": (5, 5, 8, (64, 1), 1, 0, ""),
    "out4": (5, 5, 8, (64, 4), 1, 0, ""),
    "out64": (5, 5, 8, (64, 64), 1, 0, ""),
    "out65": (5, 5, 8, (64, 65), 1, 0, "null_mean"),
    "depth1": (5, 5, 8, (52,), 1, 0, ""),
    "depth1-in257-out65": (5, 130, 127, (65,), 1, 0, ""),
    "depth8": (5, 5, 8, (64,) * 7 + (52,), 1, 0, ""),
    "small-tail": (5, 5, 8, (512, 400, 52), 1, 0, ""),
    "lds-1344": (5, 5, 8, (1344, 52), 1, 0, ""),
    "lds-2048": (5, 5, 8, (2048, 52), 1, 0, "null_mean"),
}


def plain_ops(name):
    n, ctx_dim, state_dim, widths, T, pad, _ = PLAIN[name]
    return make_ops("int", n, ctx_dim, state_dim, widths, T, pad, seed=1000 + sorted(PLAIN).index(name))


def test_plain_cases_reach_what_they_are_listed_for():
    """The preconditions of the list above, and the exactness part 1 rests on, without a kernel: on the integer operands a plain
    float32 evaluation equals float64 bit for bit, every |W| |x| + |b| is far below 2^24 and the reference is not mostly zeros."""
    cases = {k: v[:6] for k, v in PLAIN.items()}
    assert {v[0] for v in cases.values()} == {1, 4, 5, 33}
    assert {(v[1], v[2]) for v in cases.values()} >= {(128, 115), (64, 192), (130, 127), (192, 115), (3, 1), (5, 8), (0, 7), (100, 0)}
    assert {v[3][0] for v in cases.values() if len(v[3]) == 2} >= {64, 65, 192, 256, 320, 321, 641}
    assert {v[3][-1] for v in cases.values()} >= {1, 4, 64, 65} and {len(v[3]) for v in cases.values()} >= {1, 8}
    small = lambda w: sum((x + 3) & ~3 for x in w) + ((w[-1] + 3) & ~3) + 4 * w[-1]
    assert small(cases["small-tail"][3]) > 1024 and small(SHIPPED) == 812
    assert lds_bytes(13, (1344, 52)) > 64 * 1024 and lds_bytes(13, (1280, 52)) > 64 * 1024 > lds_bytes(243, SHIPPED)
    assert lds_bytes(13, (1344, 52)) == 70500 and lds_bytes(13, (2048, 52)) == 95844 <= 150 * 1024
    worst = 0.0
    for name in PLAIN:
        o = plain_ops(name)
        if o["T"] == 3:
            assert {0, 2} <= set(o["t_idx"].tolist()) and bool(torch.isnan(o["slab"][:, -8:]).all())
        ref, f32 = ref_of(o), ref_of(o, dtype=torch.float32)
        assert torch.equal(f32["mean"].double(), ref["mean"]) and torch.equal(f32["action"].double(), ref["action"]), name
        assert ref["peak"] < 2.0 ** 21 and _nonzero(ref["mean"]) >= MIN_NONZERO, (name, ref["peak"])
        worst = max(worst, ref["peak"])
    print("\n  largest |W| |x| + |b| of part 1: %.3g" % worst)


@gpu
@pytest.mark.parametrize("name", list(PLAIN))
def test_plain_step_equals_float64(name):
    opts = PLAIN[name][6].split()
    assert_exact(name, plain_ops(name), separate="separate" in opts, null_mean="null_mean" in opts)


# ------------------------------------------------------------------------------------------ part 1: actor + critic

# name -> (n, (ctx_dim, actor widths, activation, kind), (vctx_dim, critic widths, vactivation), state_dim)
CRITIC = {
    "v-head-only": (1, (5, (10, 6, 4), 1, "int"), (7, (1,), 0), 8),
    "v-deep": (6, (5, (64, 4), 0, "real"), (5, (64, 65, 6, 1), 1), 8),
    "v-noctx": (6, (5, (64, 4), 1, "int"), (0, (16, 1), 1), 8),
    "v-wide": (6, (5, (64, 4), 1, "int"), (320, (300, 1), 1), 8),
}


def critic_ops(name, kind_v="int"):
    n, (ctx_dim, widths, act, kind), (vctx_dim, vwidths, vact), S = CRITIC[name]
    o = make_ops(kind, n, ctx_dim, S, widths, T=3, pad=8, seed=2000 + sorted(CRITIC).index(name))
    o["act"] = act
    g = _gen(2100 + sorted(CRITIC).index(name))
    o["state"] = _ints(g, -3, 3, n, S).double()               # shared by both nets: integers, so that the critic stays exact
    vslab, vstride = make_ctx(kind_v, n, 3, vctx_dim, 4, g)
    v = dict(slab=vslab, stride=vstride, ctx_dim=vctx_dim, layers=make_net(kind_v, vctx_dim + S, vwidths, g), act=vact)
    return o, v


def _ref_with_critic(o, v, dtype=torch.float64):
    return ref_of(o, dtype=dtype, vslab=v["slab"], vstride=v["stride"], vctx_dim=v["ctx_dim"], vlayers=v["layers"], vact=v["act"])


def test_critic_cases_reach_what_they_are_listed_for():
    for name, (n, (ctx_dim, widths, act, kind), (vctx_dim, vwidths, vact), S) in CRITIC.items():
        o, v = critic_ops(name)
        ref, f32 = _ref_with_critic(o, v), _ref_with_critic(o, v, torch.float32)
        assert torch.equal(f32["value"].double(), ref["value"]) and ref["peak"] < 2.0 ** 21, name
        assert n < 4 or _nonzero(ref["value"]) >= MIN_NONZERO, name
        if kind == "int":
            assert torch.equal(f32["mean"].double(), ref["mean"]), name
    assert lds_bytes(328, (300, 1)) > lds_bytes(13, (64, 4)) and 328 > 256 >= 13
    assert CRITIC["v-head-only"][2][2] != CRITIC["v-head-only"][1][2] and CRITIC["v-deep"][2][2] != CRITIC["v-deep"][1][2]


@gpu
@pytest.mark.parametrize("name", list(CRITIC))
def test_actor_critic_step_equals_float64_and_the_plain_step(name):
    """value_out == float64; the actor's outputs == the plain step's bits on the same operands, and == float64 where the actor is
    exact (the tanh actor of v-deep: within part 2's tolerance)."""
    o, v = critic_ops(name)
    ref, yard = _ref_with_critic(o, v), _ref_with_critic(o, v, torch.float32)
    assert ref["peak"] < 2.0 ** 24
    both, plain = launch(o, critic=v), launch(o)
    assert torch.equal(both["value"].double(), ref["value"]), (name, both["value"], ref["value"])
    assert torch.equal(both["mean"], plain["mean"]) and torch.equal(both["action"], plain["action"])
    if o["kind"] == "int":
        assert torch.equal(both["mean"].double(), ref["mean"]) and torch.equal(both["action"], ref["action"])
    else:
        _check("critic " + name, "mean", both["mean"], ref["mean"], yard["mean"], ref["mag"])
        _check("critic " + name, "action", both["action"], ref["action"], yard["action"], ref["mag"])
    quiet = launch(o, noise=False, mean=False, critic=v)
    assert torch.equal(quiet["value"], both["value"]) and torch.equal(quiet["action"], both["mean"].double())


# ------------------------------------------------------------------------------------------------ part 1: forecast

# name -> (Hs, state_dim, ctx_dim, n, hc_row_stride - Hs, MLP widths, T)
FORECAST = {
    "Hs1": (1, 1, 0, 1, 0, (64, 4), 1),
    "Hs7": (7, 5, 5, 9, 3, (330, 6, 4), 3),
    "Hs80": (80, 5, 5, 5, 0, (64, 4), 1),
    "Hs81": (81, 5, 128, 5, 3, (64, 4), 3),
    "Hs128": (128, 115, 128, 9, 0, SHIPPED, 1),
    "Hs512": (512, 115, 5, 5, 3, (64, 52), 1),
}


def forecast_ops(name, seed=3000):
    """Real operands: (operands of the MLP behind the cell with `state` = the cell's input, the cell)."""
    Hs, S, ctx_dim, n, extra, widths, T = FORECAST[name]
    seed += sorted(FORECAST).index(name)
    o = make_ops("real", n, ctx_dim, Hs, widths, T=T, pad=8 if T > 1 else 0, seed=seed)
    g = _gen(seed + 500)
    o["cell_state"] = torch.randn(n, S, generator=g, dtype=torch.float64) * 2
    w_ih, w_hh = torch.randn(4 * Hs, S, generator=g) / math.sqrt(S + Hs), torch.randn(4 * Hs, Hs, generator=g) / math.sqrt(S + Hs)
    b = torch.randn(4 * Hs, generator=g) * 0.3
    # the header's row order: row 4 u + gate = [W_ih[gate Hs + u] | W_hh[gate Hs + u]]
    order = (torch.arange(4)[None, :] * Hs + torch.arange(Hs)[:, None]).reshape(-1)
    cell = dict(W=torch.cat((w_ih, w_hh), 1)[order].contiguous(), b=b[order].contiguous(), hs=Hs, stride=Hs + extra,
                h=torch.tanh(torch.randn(n, Hs, generator=g)), c=torch.randn(n, Hs, generator=g), null_ctx=ctx_dim == 0,
                ref=(w_ih, w_hh, b))
    return o, cell


def forecast_ref(o, cell, dtype=torch.float64):
    return policy_ref(o["slab"], o["stride"], o["ctx_dim"], o["t_idx"], o["cell_state"], o["layers"], 1, o["log_std"], o["noise"],
                      cell=cell["ref"], h=cell["h"], c=cell["c"], dtype=dtype)


def run_forecast(o, cell):
    """The forecast launch on (o, cell): the cell's input is o["cell_state"], the MLP's widths are o's."""
    S = o["cell_state"].shape[1]
    fo = dict(o, state=o["cell_state"], state_dim=S)
    got = launch(fo, cell=cell)
    o[("dev", False)] = fo[("dev", False)]
    return got


def test_forecast_cases_cover_the_lists():
    v = list(FORECAST.values())
    assert {c[0] for c in v} == {1, 7, 80, 81, 128, 512} and {c[1] for c in v} == {1, 5, 115} and {c[2] for c in v} == {0, 5, 128}
    assert {c[3] for c in v} == {1, 5, 9} and all(FORECAST[k][3] == 5 for k in ("Hs80", "Hs81", "Hs512")) and {c[4] for c in v} == {0, 3}
    assert 4 * 80 == 5 * 64 and 4 * 81 == 5 * 64 + 4
    o, cell = forecast_ops("Hs7")
    ref = forecast_ref(o, cell)
    lstm = torch.nn.LSTMCell(5, 7).double()                     # the reference's cell step is torch's, gate order included
    with torch.no_grad():
        lstm.weight_ih.copy_(cell["ref"][0]); lstm.weight_hh.copy_(cell["ref"][1]); lstm.bias_ih.copy_(cell["ref"][2]); lstm.bias_hh.zero_()
        h1, c1 = lstm(o["cell_state"].float().double(), (cell["h"].double(), cell["c"].double()))
    assert torch.allclose(h1, ref["h"], rtol=0, atol=1e-14) and torch.allclose(c1, ref["c"], rtol=0, atol=1e-14)


@gpu
@pytest.mark.parametrize("name", list(FORECAST))
def test_forecast_step_by_transitivity(name):
    """h', c' against the float64 cell in part 2's tolerance (magnitude 1); then the kernel's own h' as the plain step's state:
    mean_out and action of the forecast step == the plain step's bits (float32 -> float64 -> float32 is exact)."""
    o, cell = forecast_ops(name)
    ref, yard = forecast_ref(o, cell), forecast_ref(o, cell, torch.float32)
    got = run_forecast(o, cell)
    one = torch.ones(())
    _check("forecast " + name, "h", got["h"], ref["h"], yard["h"], one)
    _check("forecast " + name, "c", got["c"], ref["c"], yard["c"], one)
    assert not torch.equal(got["h"], cell["h"])
    plain = launch(dict(o, state=got["h"].double()))
    assert torch.equal(got["mean"], plain["mean"]) and torch.equal(got["action"], plain["action"])
    assert not torch.equal(got["action"], got["mean"].double()) and bool(torch.isfinite(got["action"]).all())


# -------------------------------------------------------------------------------------------------- part 2: rounding

_WORST = {}


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def _figures(got, ref, yard, mag):
    d = (got.double() - ref).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf"), _rel(yard, ref), float("inf")
    return _rel(got, ref), _rel(yard, ref), float((d / mag.clamp_min(1e-300)).max())


def _check(group, what, got, ref, yard, mag):
    """One comparison: prints its figures, records the group's worst ones, asserts the tolerance."""
    e, y, el = _figures(got, ref, yard, mag)
    w = _WORST.setdefault(group, [0.0, 0.0])
    if e > FLOOR:
        w[0] = max(w[0], e / max(y, 1e-300))
    w[1] = max(w[1], el)
    print("  [%s] %-8s hip %.2e  f32 %.2e  ratio %5.2f  elem %.2e" % (group, what, e, y, e / max(y, 1e-300), el))
    assert e < max(C_POL * y, FLOOR) and el <= E_POL, (group, what, e, y, el)


def _margin(wrong, ref, yard, mag):
    """How many times a known-wrong float64 result misses the tolerance (in rel or in elem, whichever misses more)."""
    e, y, el = _figures(wrong, ref, yard, mag)
    return max(e / max(C_POL * y, FLOOR), el / E_POL)


def shipped_ops(n=9, T=3):
    return make_ops("real", n, 128, 115, SHIPPED, T=T, pad=8, seed=4000)


def narrow_ops(n=9):
    o = make_ops("real", n, 192, 115, (330, 6, 4), T=3, pad=8, seed=4001)
    o["act"] = 0
    return o


@gpu
@pytest.mark.parametrize("name", ["shipped-relu", "307to330to6to4-tanh"])
def test_rounding_of_the_plain_step(name):
    o = shipped_ops() if name == "shipped-relu" else narrow_ops()
    ref, yard = ref_of(o), ref_of(o, dtype=torch.float32)
    got = launch(o)
    for what in ("mean", "action"):
        _check(name, what, got[what], ref[what], yard[what], ref["mag"])


@gpu
def test_rounding_of_the_forecast_step():
    o, cell = forecast_ops("Hs128", seed=4100)
    ref, yard = forecast_ref(o, cell), forecast_ref(o, cell, torch.float32)
    got = run_forecast(o, cell)
    one = torch.ones(())
    for what, mag in (("h", one), ("c", one), ("mean", ref["mag"]), ("action", ref["mag"])):
        _check("forecast-115-128-128", what, got[what], ref[what], yard[what], mag)


@gpu
def test_rounding_of_the_actor_critic_step():
    """The shipped widths for both nets, the critic with sigmoid."""
    o = shipped_ops()
    g = _gen(4200)
    vslab, vstride = make_ctx("real", 9, 3, 128, 8, g)
    v = dict(slab=vslab, stride=vstride, ctx_dim=128, layers=make_net("real", 243, (300, 200, 1), g), act=2)
    ref, yard = _ref_with_critic(o, v), _ref_with_critic(o, v, torch.float32)
    got = launch(o, critic=v)
    for what, mag in (("mean", ref["mag"]), ("action", ref["mag"]), ("value", ref["vmag"])):
        _check("critic-shipped-sigmoid", what, got[what], ref[what], yard[what], mag)


# ------------------------------------------------------------------- self-check of the tolerances (CPU, float64 only)

def _margin_of(wrong, ref, yard):
    return max(_margin(wrong[k], ref[k], yard[k], ref["mag"]) for k in ("mean", "action"))


def test_tolerance_tells_a_wrong_answer():
    """With the float64 reference and the float32 yardstick alone (CPU), n = 9, T = 3: each modelled fault of the kernel misses
    the tolerance by at least SELF_MARGIN in mean or action. (a), (b), (d), (e) at the shipped shape; (c) at 307 -> 330 -> 6 -> 4,
    the part-2 shape with a width that is no multiple of 4 (the shipped widths all are: there the fault changes nothing)."""
    o = shipped_ops()
    ref, yard = ref_of(o), ref_of(o, dtype=torch.float32)
    assert _margin_of(yard, ref, yard) < 1.0                    # float32 itself passes
    n = o["n"]
    x = torch.cat((_gather(o["slab"], o["stride"], 128, o["t_idx"], n, torch.float64), o["state"].float().double()), 1)
    layers = [(W.double(), b.double()) for W, b in o["layers"]]
    sd, nz = torch.exp(o["log_std"].double()), o["noise"].double()

    def rest(pre1, noise=nz, tail=layers[1:], act=1):
        a = ACTS[act](pre1)
        for l, (W, b) in enumerate(tail):
            a = a @ W.t() + b
            if l < len(tail) - 1:
                a = ACTS[act](a)
        return {"mean": a, "action": a + sd * noise}

    W1, b1 = layers[0]
    pre1 = x @ W1.t() + b1
    same = rest(pre1)
    assert torch.allclose(same["mean"], ref["mean"], rtol=0, atol=1e-12) and torch.allclose(same["action"], ref["action"], rtol=0, atol=1e-12)
    margins = {}
    wrong = pre1.clone()                                       # (a) quad 7 of column group 2 missing in layer 1
    wrong[:, 128:192] -= x[:, 28:32] @ W1[128:192, 28:32].t()
    margins["a"] = _margin_of(rest(wrong), ref, yard)
    nkq = (243 + 3) // 4                                       # (b) wave 1's share of the quads, rows 4 .. 7
    k0, k1 = 4 * (1 * nkq // 4), 4 * (2 * nkq // 4)
    assert (k0, k1) == (60, 120)
    wrong = pre1.clone()
    wrong[4:8] -= x[4:8, k0:k1] @ W1[:, k0:k1].t()
    margins["b"] = _margin_of(rest(wrong), ref, yard)
    margins["d"] = _margin_of(rest(pre1, noise=torch.roll(nz, -1, 0)), ref, yard)          # (d) the next row's noise
    xe = torch.cat((_gather(o["slab"], o["stride"], 128, (o["t_idx"] + 1) % 3, n, torch.float64), x[:, 128:]), 1)     # (e) t_idx + 1
    margins["e"] = _margin_of(rest(xe @ W1.t() + b1), ref, yard)
    # (c) the LDS copy of the biases is [b1 (330) | 2 pad | b2 (6) | 2 pad | b3 (4)]; offsets that advance by the unrounded
    # widths read layer 2's at 330 and layer 3's at 336 (the never-written pad floats taken as zero)
    o = narrow_ops()
    ref, yard = ref_of(o), ref_of(o, dtype=torch.float32)
    assert _margin_of(yard, ref, yard) < 1.0
    layers = [(W.double(), b.double()) for W, b in o["layers"]]
    sd, nz = torch.exp(o["log_std"].double()), o["noise"].double()
    x = torch.cat((_gather(o["slab"], o["stride"], 192, o["t_idx"], n, torch.float64), o["state"].float().double()), 1)
    pre1 = x @ layers[0][0].t() + layers[0][1]
    same = rest(pre1, noise=nz, tail=layers[1:], act=0)
    assert torch.allclose(same["mean"], ref["mean"], rtol=0, atol=1e-12) and torch.allclose(same["action"], ref["action"], rtol=0, atol=1e-12)
    lds = torch.zeros(344, dtype=torch.float64)
    lds[0:330], lds[332:338], lds[340:344] = layers[0][1], layers[1][1], layers[2][1]
    shifted = [(layers[1][0], lds[330:336]), (layers[2][0], lds[336:340])]
    margins["c"] = _margin_of(rest(pre1, noise=nz, tail=shifted, act=0), ref, yard)
    print("\n  self-check margins: " + ", ".join("(%s) %.3g" % kv for kv in sorted(margins.items())))
    low = {k: v for k, v in margins.items() if not v >= SELF_MARGIN}
    assert not low, low
