"""The persistent LSTM sweeps (csrc/egp_lstm.hip) against an independent float64 statement of the cell, at the shapes the
update runs and at every kernel instantiation.

The reference (`_sweeps`) is the reference's nn.LSTMCell loop (models/rnn.py:45-61) written with plain torch ops: gate
order i, f, g, o, zero initial state, one loop per problem over t ascending (descending for a reversed problem). It runs
on the GPU in float64 so that the update's shapes stay fast, and its gradients come from float64 autograd over the same
loop. It goes through none of nets.RNN, lstm.* or the egp_* calls.

Tolerances follow a yardstick, as test_gemm_gpu.py does: the same loop evaluated by torch in float32 has an error against
float64 too, and the HIP result may be at most C times that error, or below FLOOR. Both are applied to the norm ratio
|got - ref| / |ref| and to max|got - ref| / max|ref|, per quantity (outputs, d_x, dW_ih, dW_hh, both biases).
Calibrated on the MI355X over every case of this file (worst HIP / yardstick ratio): outputs 1.8x, d_x 2.7x, bias
gradients 2.4x (4.9x in max-abs for the atomic [P][4H] form, under the floor), hence C_YARD = 4. The largest errors that
the floors (1e-6, 1e-5) admit are the bias gradients of lstm_direction, 5.3e-7 in norm; outputs stay under 3.3e-7 in norm
and 1e-6 in max-abs outside the saturated case. The weight gradients come out of split-K products (gemm.linear_wgrad: 32
chains of up to 35 k rows each at B = 5120, T = 220, each summed serially in float32): dW_hh up to 4.7x, dW_ih up to 9.2x
(1.1e-5 in norm, B = 5120 without row lists), hence C_WGRAD = 12.
Each case also shows that the tolerance tells a wrong answer: with the float64 reference alone, W_hh rounded to bf16 (a
lost split term) and the outputs of one sequence shifted by one time step must each miss it by at least SELF_MARGIN.
Measured: at least 16x (bf16 W_hh; d_x of the saturated case) and 25 000x (shift).
"""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C_YARD = 4.0                 # HIP error <= C_YARD x float32 yardstick error ...
C_WGRAD = 12.0               # ... (C_WGRAD for dW_ih and dW_hh) ...
FLOOR = (1e-6, 1e-5)         # ... or below this floor (norm ratio, max-abs over max|ref|)
SELF_MARGIN = 3.0            # a wrong answer misses the tolerance at least this many times
QUANTITIES = ("out", "d_x", "W_ih", "W_hh", "b_ih", "b_hh")


# ---------------------------------------------------------------------------------------------------------- reference

def _sweeps(x, params, reverses):
    """x (T, B, D); params [(w_ih (4H, D), w_hh (4H, H), b_ih, b_hh)] * P -> [(T, B, H)] * P. Problem p walks t = 0 .. T-1
    (T-1 .. 0 when reverses[p]) from h = c = 0: gates = x_t W_ih^T + b_ih + h W_hh^T + b_hh, split i, f, g, o;
    c = sigmoid(f) c + sigmoid(i) tanh(g); h = sigmoid(o) tanh(c). The P problems advance together (one bmm per step)."""
    T, B, _ = x.shape
    w_ih = torch.stack([p[0] for p in params]).transpose(1, 2)             # (P, D, 4H)
    w_hh = torch.stack([p[1] for p in params]).transpose(1, 2)             # (P, H, 4H)
    bias = torch.stack([p[2] + p[3] for p in params]).unsqueeze(1)         # (P, 1, 4H)
    P, H = len(params), w_hh.shape[1]
    xs = x.unbind(0)
    h = c = x.new_zeros(P, B, H)
    outs = []
    for s in range(T):
        xt = torch.stack([xs[T - 1 - s] if r else xs[s] for r in reverses])
        i, f, g, o = (torch.baddbmm(bias, xt, w_ih) + torch.bmm(h, w_hh)).chunk(4, 2)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs.append(h)
    hs = torch.stack(outs)                                                 # (steps, P, B, H)
    return [hs[:, p].flip(0) if r else hs[:, p] for p, r in enumerate(reverses)]


def _evaluate(x, params, reverses, dys, dtype, w_hh_bf16=False):
    """The loop in `dtype`: outputs, and per entry of `dys` (a list of P (T, B, H) output gradients) the gradients
    [d_x, then per problem dW_ih, dW_hh, db_ih, db_hh]. w_hh_bf16: W_hh rounded to bf16 first (a self-check)."""
    xr = x.detach().to(dtype).requires_grad_(True)
    pr = []
    for p in params:
        p = [t.detach() for t in p]
        if w_hh_bf16:
            p[1] = p[1].to(torch.bfloat16)
        pr.append([t.to(dtype).requires_grad_(True) for t in p])
    with torch.enable_grad():
        outs = _sweeps(xr, pr, reverses)
        leaves = [xr] + [t for p in pr for t in p]
        grads = [list(torch.autograd.grad(outs, leaves, [d.to(dtype) for d in dy], retain_graph=k + 1 < len(dys)))
                 for k, dy in enumerate(dys)]
    return [o.detach() for o in outs], grads


class _Ref:
    """float64 reference, float32 yardstick and the bf16-W_hh self-check of one case, evaluated once."""

    def __init__(self, x, cells, reverses, dys):
        params = [(c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh) for c in cells]
        self.out, self.grads = _evaluate(x, params, reverses, dys, torch.float64)
        self.y_out, self.y_grads = _evaluate(x, params, reverses, dys, torch.float32)
        self.w_out, w_grads = _evaluate(x, params, reverses, dys[-1:], torch.float64, w_hh_bf16=True)
        self.w_grads = w_grads[0]
        self.P = len(cells)

    def outputs(self, which, pairs):
        """[(T, B, H)] * P, or the pairs' [(T, B, 2H)] * P/2, of the reference / yardstick / bf16 self-check."""
        o = {"ref": self.out, "yard": self.y_out, "bf16": self.w_out}[which]
        return [torch.cat(o[i:i + 2], 2) for i in range(0, len(o), 2)] if pairs else o


# -------------------------------------------------------------------------------------------------------- comparisons

def _errs(got, ref, mask=None):
    """(|got - ref| / |ref|, max|got - ref| / max|ref|), over the rows where `mask` holds; inf if got is not finite there."""
    got, ref = got.double(), ref.double()
    if mask is not None:
        got, ref = torch.where(mask, got, 0.0), torch.where(mask, ref, 0.0)
    d = got - ref
    if not bool(torch.isfinite(d).all()):
        return float("inf"), float("inf")
    return float(d.norm() / ref.norm()), float(d.abs().max() / ref.abs().max())


class _Case:
    """Collects every comparison of one case and asserts at the end, so that a failing case still reports them all."""

    def __init__(self, name):
        self.name, self.tols, self.lines, self.misses = name, {}, [], []

    def tolerance(self, key, ref, yard, mask=None, c=C_YARD):
        y = _errs(yard, ref, mask)
        self.tols[key] = (y, (max(c * y[0], FLOOR[0]), max(c * y[1], FLOOR[1])))

    def check(self, what, key, got, ref, mask=None):
        e = _errs(got, ref, mask)
        y, tol = self.tols[key]
        ok = e[0] <= tol[0] and e[1] <= tol[1]
        self.lines.append("%-34s hip %.1e / %.1e   f32 %.1e / %.1e   tol %.1e / %.1e%s"
                          % (what, e[0], e[1], y[0], y[1], tol[0], tol[1], "" if ok else "   MISS"))
        if not ok:
            self.misses.append(what)

    def must_miss(self, what, key, wrong, ref, mask=None):
        """A known-wrong result must miss the tolerance of `key` by SELF_MARGIN (in norm or in max-abs)."""
        e = _errs(wrong, ref, mask)
        tol = self.tols[key][1]
        margin = max(e[0] / tol[0], e[1] / tol[1])
        self.lines.append("%-34s self-check misses by %.0fx" % (what, margin))
        if not margin >= SELF_MARGIN:
            self.misses.append(what + " (self-check)")

    def finish(self):
        print("\n[%s]\n  " % self.name + "\n  ".join(self.lines))
        assert not self.misses, "%s: %s" % (self.name, ", ".join(self.misses))


def _set_tolerances(case, ref, pairs, mask=None, tag=""):
    """Tolerances of every quantity from the yardstick: outputs (where `mask` holds), and per gradient set k the gradients."""
    for i, (a, b) in enumerate(zip(ref.outputs("ref", pairs), ref.outputs("yard", pairs))):
        case.tolerance("%sout[%d]" % (tag, i), a, b, mask)
    for k in range(len(ref.grads)):
        for j, (a, b) in enumerate(zip(ref.grads[k], ref.y_grads[k])):
            case.tolerance("%s%d/%s" % (tag, k, _qname(j)), a, b, c=C_WGRAD if _qname(j)[0] == "W" else C_YARD)


def _qname(j):
    return "d_x" if j == 0 else "%s[%d]" % (QUANTITIES[2 + (j - 1) % 4], (j - 1) // 4)


def _check_run(case, what, ref, outs, grads, pairs, k, mask=None, tag=""):
    """HIP outputs (and gradients of set k, when given: [d_x or None, per problem 4]) against the reference."""
    for i, (o, r) in enumerate(zip(outs, ref.outputs("ref", pairs))):
        case.check("%s out[%d]" % (what, i), "%sout[%d]" % (tag, i), o, r, mask)
    if grads is not None:
        for j, (g, r) in enumerate(zip(grads, ref.grads[k])):
            if g is not None:
                case.check("%s %s" % (what, _qname(j)), "%s%d/%s" % (tag, k, _qname(j)), g, r)


def _self_checks(case, ref, pairs, k, seq, mask=None, tag=""):
    """The bf16-W_hh reference and a one-step shift of sequence `seq` against the tolerances of gradient set k."""
    for i, (w, r) in enumerate(zip(ref.outputs("bf16", pairs), ref.outputs("ref", pairs))):
        case.must_miss("W_hh in bf16: out[%d]" % i, "%sout[%d]" % (tag, i), w, r, mask)
        shifted = r.clone()
        shifted[1:, seq] = r[:-1, seq]
        shifted[0, seq] = 0.0
        case.must_miss("shifted by one step: out[%d]" % i, "%sout[%d]" % (tag, i), shifted, r, mask)
    for j, (w, r) in enumerate(zip(ref.w_grads, ref.grads[k])):
        case.must_miss("W_hh in bf16: %s" % _qname(j), "%s%d/%s" % (tag, k, _qname(j)), w, r)


# ------------------------------------------------------------------------------------------------------------ helpers

def _poison(*numels):
    """Hand the caching allocator blocks full of NaN of these sizes (float32 elements): a buffer that the sweeps leave
    unwritten and a later product reads then shows up as NaN instead of as stale plausible numbers."""
    torch.cuda.empty_cache()
    junk = [torch.full((int(n),), float("nan"), device="cuda") for n in numels]
    del junk


def _cells(P, D, H, seed, scale=None):
    torch.manual_seed(seed)
    cells = [torch.nn.LSTMCell(D, H) for _ in range(P)]
    if scale is not None:
        with torch.no_grad():
            for c in cells:
                for name, s in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), scale):
                    getattr(c, name).mul_(s)
    return [c.cuda() for c in cells]


def _hip_grads(cells, x):
    out = [x.grad.clone() if x.grad is not None else None]
    for c in cells:
        out += [c.weight_ih.grad.clone(), c.weight_hh.grad.clone(), c.bias_ih.grad.clone(), c.bias_hh.grad.clone()]
        c.zero_grad(set_to_none=True)
    return out


def _instantiation(H, B):
    nq = 2 if H == 64 and B >= 4096 else 1
    return "NQ=%d LH=%d FULL=%s" % (nq, H, "true" if B % (4 * nq) == 0 else "false")


def _steps(rng, B, T):
    """Step counts shaped like the update's (episode length + margin, T = longest + 2 margins): many full episodes,
    a spread of early ends, some empty padding windows; 0, T and T-1, T-2, T-3 present (every residue mod 4)."""
    m = 10
    steps = rng.randint(m + 1, T - m + 1, size=B)
    steps[rng.rand(B) < 0.3] = T - m
    steps[rng.rand(B) < 0.04] = 0
    steps[:5] = [T, 0, T - 1, T - 2, T - 3]
    return steps


def _workgroup_maxima(steps, rows):
    s = np.sort(steps)[::-1]
    return s[np.arange(0, len(s), rows)]


# -------------------------------------------------------------------------------------------------------------- tests

@pytest.mark.parametrize("H,B", [(64, 4095), (64, 4096), (64, 4097), (64, 4100), (64, 5120), (128, 44), (128, 45)])
def test_every_instantiation_matches_float64(H, B):
    """k_lstm_{fwd,bwd}_mfma<NQ, LH, FULL[, TRAIN]>: 8-row workgroups (NQ = 2) from B = 4096 on at hidden 64, full and
    ragged (4097: one live row in the last workgroup; 4100: one live and one dead quad), 4-row ones below and at hidden
    128. lstm_group (a forward and a reversed problem in one launch) and lstm_direction, in training and under
    torch.no_grad(): outputs, d_x and every parameter gradient against float64. T varies with the case, so that the
    unrolled loops end in each of their remainder iterations."""
    from egopose_amd import lstm as hl
    T = 60 + (B % 4 if H == 64 else B % 2)
    D = 128 if H == 64 else 96
    g = torch.Generator(device="cuda").manual_seed(B + H)
    cells = _cells(2, D, H, seed=B + H)
    revs = [False, True]
    x = torch.randn(T, B, D, device="cuda", generator=g)
    dys = [torch.randn(T, B, H, device="cuda", generator=g) for _ in range(2)]
    assert hl.group_available(x, cells)
    ref = _Ref(x, cells, revs, [dys])
    case = _Case("H=%d B=%d T=%d: %s" % (H, B, T, _instantiation(H, B)))
    _set_tolerances(case, ref, False)
    bufs = (T * B * 2 * 4 * H, 2 * (T + 2) * B * H, 2 * T * B * H, T * B * 4 * H, (T + 1) * B * H, T * B * H)

    _poison(*bufs)
    xx = x.clone().requires_grad_(True)
    outs = hl.lstm_group(xx, cells, revs)
    torch.autograd.backward(outs, dys)
    _check_run(case, "lstm_group", ref, [o.detach() for o in outs], _hip_grads(cells, xx), False, 0)

    _poison(*bufs)
    xx = x.clone().requires_grad_(True)
    outs = [hl.lstm_direction(c, xx, r) for c, r in zip(cells, revs)]
    torch.autograd.backward(outs, dys)
    _check_run(case, "lstm_direction", ref, [o.detach() for o in outs], _hip_grads(cells, xx), False, 0)

    with torch.no_grad():
        _poison(*bufs)
        _check_run(case, "lstm_group no_grad", ref, hl.lstm_group(x, cells, revs), None, False, 0)
        _check_run(case, "lstm_direction no_grad", ref, [hl.lstm_direction(c, x, r) for c, r in zip(cells, revs)], None, False, 0)
    _self_checks(case, ref, False, 0, seq=B - 1)
    case.finish()


@pytest.mark.parametrize("B", [1280, 5120])
def test_update_shape_grouped_sweeps_match_float64(B):
    """The update's grouped sweeps (lstm.LstmGroup as nets.grouped_video_context calls it): T = 220, H = 64, the two
    bi-LSTMs of the critic and the actor as P = 4 problems with reverse mask 0b1010 and paired outputs, D = 128 (the
    context's feature width). B = 1280 is the 1 024-slot update (4-row workgroups), B = 5120 the 4 096-slot one (8-row).
    Runs: full sweeps; ragged step counts (lstm.ragged_order) without and with row lists, d_x included; the update's own
    form (ragged, row lists, leave_skipped, frame table whose last window ends on the table's last row); and its
    torch.no_grad() form. Ragged runs are compared, and differentiated, only inside each sequence's own steps."""
    from egopose_amd import gemm as G
    from egopose_amd import lstm as hl
    T, H, D, P, F = 220, 64, 128, 4, 3000
    rng = np.random.RandomState(B)
    g = torch.Generator(device="cuda").manual_seed(B)
    cells = _cells(P, D, H, seed=B)
    revs = [False, True, False, True]
    table = torch.randn(F, D, device="cuda", generator=g)
    base = rng.randint(0, F - T + 1, size=B)
    base[0], base[B - 1] = F - T, 0                     # the first sequence (T steps) reads the table's last row
    base_t = torch.as_tensor(base.astype(np.int32), device="cuda")
    x = table[base_t.long().unsqueeze(0) + torch.arange(T, device="cuda").unsqueeze(1)]          # (T, B, D)
    steps = _steps(rng, B, T)
    for rows in (4, 8):                                 # every remainder of the unrolled loops is some workgroup's last iteration
        assert set(_workgroup_maxima(steps, rows) % 4) == {0, 1, 2, 3}
    rows_ = hl.ragged_order(steps, torch.device("cuda"), T=T)
    assert rows_.rows is not None and G.fused_rows_available(), "the update's row-list path must be the one under test"
    flat = hl.ragged_order(steps, torch.device("cuda"))
    inside = (torch.arange(T).unsqueeze(1) < torch.as_tensor(steps).unsqueeze(0)).unsqueeze(2).cuda()      # (T, B, 1)
    dys = [torch.randn(T, B, H, device="cuda", generator=g) for _ in range(P)]
    dys_in = [d * inside for d in dys]
    pair = lambda ds: [torch.cat(ds[i:i + 2], 2) for i in range(0, P, 2)]

    ref = _Ref(x, cells, revs, [dys, dys_in])
    case = _Case("update shape B=%d: %s, P=4 paired" % (B, _instantiation(H, B)))
    _set_tolerances(case, ref, True, tag="full ")
    _set_tolerances(case, ref, True, inside)
    bufs = (T * B * P * 4 * H, T * B * P * 4 * H, 2 * (T + 2) * B * 2 * H, P * T * B * H, P * B * 4 * H, F * P * 4 * H)

    def run(ragged, frames, with_dx, ds):
        _poison(*bufs)
        xx = x.clone().requires_grad_(with_dx)
        outs = hl.lstm_group(xx, cells, revs, pairs=True, ragged=ragged, frames=frames)
        torch.autograd.backward(outs, pair(ds))
        return [o.detach() for o in outs], _hip_grads(cells, xx)

    outs, grads = run(None, None, True, dys)
    _check_run(case, "full", ref, outs, grads, True, 0, tag="full ")
    outs, grads = run(flat, None, True, dys_in)
    _check_run(case, "ragged", ref, outs, grads, True, 1, mask=inside)
    outs, grads = run(rows_, None, True, dys_in)
    _check_run(case, "ragged, row lists", ref, outs, grads, True, 1, mask=inside)
    outs, grads = run(rows_, (table, base_t), False, dys_in)
    _check_run(case, "ragged, row lists, frames", ref, outs, grads, True, 1, mask=inside)
    with torch.no_grad():
        _poison(*bufs)
        outs = hl.lstm_group(x, cells, revs, pairs=True, ragged=rows_, frames=(table, base_t))
        _check_run(case, "no_grad, ragged, frames", ref, outs, None, True, 1, mask=inside)
    _self_checks(case, ref, True, 1, seq=0, mask=inside)
    case.finish()


def test_saturated_gates_over_a_long_sequence_match_float64():
    """Weights and biases scaled until gate pre-activations reach +-60 and beyond (the kernels' sigmoid / tanh are
    rcp(1 + exp(..)) forms whose exp overflows to inf there) and the cell state grows past the range of tanh, over
    T = 400 steps: outputs and gradients finite and at float64 within the yardstick's tolerance."""
    from egopose_amd import lstm as hl
    T, B, D, H = 400, 301, 128, 64
    g = torch.Generator(device="cuda").manual_seed(400)
    cells = _cells(2, D, H, seed=400, scale=(40.0, 2.0, 40.0, 40.0))
    revs = [False, True]
    x = torch.randn(T, B, D, device="cuda", generator=g)
    dys = [torch.randn(T, B, H, device="cuda", generator=g) for _ in range(2)]
    pre = torch.cat([x[0] @ c.weight_ih.t() + c.bias_ih + c.bias_hh for c in cells], 1)
    assert float(pre.abs().max()) > 60.0 and float((pre.abs() > 20.0).float().mean()) > 0.3
    ref = _Ref(x, cells, revs, [dys])
    case = _Case("saturated gates, T=400 B=301: %s" % _instantiation(H, B))
    _set_tolerances(case, ref, True)
    xx = x.clone().requires_grad_(True)
    _poison(T * B * 2 * 4 * H, T * B * 2 * 4 * H, (T + 2) * B * 2 * H, 2 * T * B * H)
    outs = hl.lstm_group(xx, cells, revs, pairs=True)
    torch.autograd.backward(outs, [torch.cat(dys, 2)])
    grads = _hip_grads(cells, xx)
    assert all(bool(torch.isfinite(t).all()) for t in [o.detach() for o in outs] + grads)
    _check_run(case, "lstm_group", ref, [o.detach() for o in outs], grads, True, 0)
    _self_checks(case, ref, True, 0, seq=7)
    case.finish()


def test_group_bwd_len_bias_gradient_contract():
    """egp_lstm_bwd_f32 with d_bias_rows = 0 (nothing in lstm.py asks for it) through ctypes: its d_bias is [P][4H],
    summed over every (t, b) row with float atomics into a buffer the caller zeroed. It must equal the float64 sum of its
    own d_pre, the fixed-order sum of the [P][B][4H] rows that d_bias_rows = 1 gives (to tolerance, not bits) and the
    float64 reference's bias gradient; the two forms' d_pre must be bit-identical. B = 4100 with ragged steps:
    8-row workgroups whose last one has a dead quad."""
    from egopose_amd import _lib as L
    T, B, D, H, P = 60, 4100, 64, 64, 4
    kmask = 0b1100                                      # forward-running problems first, as lstm.LstmGroup orders them
    revs = [bool((kmask >> p) & 1) for p in range(P)]
    lib = L.load()
    assert lib.egp_lstm_gate_layout() == 1
    rng = np.random.RandomState(7)
    g = torch.Generator(device="cuda").manual_seed(7)
    cells = _cells(P, D, H, seed=7)
    x = torch.randn(T, B, D, device="cuda", generator=g)
    steps = _steps(rng, B, T)
    inside = (torch.arange(T).unsqueeze(1) < torch.as_tensor(steps).unsqueeze(0)).unsqueeze(2).cuda()
    dys = [torch.randn(T, B, H, device="cuda", generator=g) * inside for _ in range(P)]
    ref = _Ref(x, cells, revs, [dys])
    case = _Case("egp_lstm_bwd_f32 with d_bias [P][4H], B=4100: %s" % _instantiation(H, B))
    _set_tolerances(case, ref, False, inside)

    n = torch.arange(4 * H, device="cuda")
    perm = (n % 4) * H + n // 4                         # kernel column 4u + gate <- torch row gate * H + u
    with torch.no_grad():
        gx = torch.cat([(x.double() @ c.weight_ih.double().t() + (c.bias_ih + c.bias_hh).double())[..., perm] for c in cells],
                       2).float().reshape(T * B, P * 4 * H).contiguous()
        w_hh = torch.stack([c.weight_hh for c in cells]).contiguous()
    order_np = np.argsort(-steps, kind="stable")
    order = torch.as_tensor(order_np.astype(np.int32), device="cuda")
    steps_sorted = torch.as_tensor(steps[order_np].astype(np.int32), device="cuda")
    _poison(P * T * B * H, T * B * P * 4 * H, P * T * B * H, T * B * P * 4 * H, T * B * P * 4 * H)
    h = torch.empty(P, T, B, H, device="cuda")
    gates = torch.empty(T * B, P * 4 * H, device="cuda")
    cells_save = torch.empty(P, T, B, H, device="cuda")
    s = L.current_stream()
    dh = torch.stack(dys).contiguous()
    d_pre = torch.empty(T * B, P * 4 * H, device="cuda")
    d_bias = torch.zeros(P, 4 * H, device="cuda")
    d = L.LstmDesc(T=T, B=B, hidden=H, n_problems=P, reverse_mask=kmask, w_hh=w_hh.data_ptr(), gates_x=gx.data_ptr(), ld_h=H,
                   gates_save=gates.data_ptr(), cells_save=cells_save.data_ptr(), ld_dh=H, d_pre=d_pre.data_ptr(),
                   d_bias=d_bias.data_ptr(), d_bias_rows=0, seq_order=order.data_ptr(), seq_steps=steps_sorted.data_ptr())
    for p in range(P):
        d.h_out[p], d.dh_out[p] = h[p].data_ptr(), dh[p].data_ptr()
    L.check(lib.egp_lstm_fwd_f32(d, s), "fwd")
    L.check(lib.egp_lstm_bwd_f32(d, s), "bwd, d_bias [P][4H]")
    d_pre2 = torch.empty_like(d_pre)
    db_rows = torch.empty(P, B, 4 * H, device="cuda")
    d.d_pre, d.d_bias, d.d_bias_rows = d_pre2.data_ptr(), db_rows.data_ptr(), 1
    L.check(lib.egp_lstm_bwd_f32(d, s), "bwd, d_bias [P][B][4H]")
    torch.cuda.synchronize()
    assert torch.equal(d_pre, d_pre2)
    _check_run(case, "fwd", ref, list(h), None, False, 0, mask=inside)
    # the atomic [P][4H] sum against the float64 sum of the same d_pre and the rows form's fixed-order sum: float32 rounding of
    # the partial sums only, bounded by the sum of the magnitudes
    d64 = d_pre.double().view(T * B, P, 4 * H)
    mag = d64.abs().sum(0)
    for name, other in (("float64 sum of d_pre", d64.sum(0)), ("rows form, summed", db_rows.sum(1).double())):
        bad = ((d_bias.double() - other).abs() > 1e-6 * mag + 1e-30).sum()       # (measured: 1.5e-8)
        case.lines.append("d_bias vs %-24s max %.1e of the magnitude sum" % (name, float(((d_bias.double() - other).abs() / mag.clamp_min(1e-30)).max())))
        if int(bad):
            case.misses.append("d_bias vs " + name)
    db_torch = d_bias[:, torch.argsort(perm)]           # back to torch's gate order
    for p in range(P):
        case.check("d_bias[%d] (atomic)" % p, "0/b_ih[%d]" % p, db_torch[p], ref.grads[0][1 + 4 * p + 2])
    case.must_miss("W_hh in bf16: b_ih[0]", "0/b_ih[0]", ref.w_grads[3], ref.grads[0][3])
    case.finish()


@pytest.mark.parametrize("D", [24, 128])
def test_grouped_backward_at_8_row_workgroups_is_bit_reproducible(D):
    """test_lstm_gpu.py's reproducibility check at B = 5120 (NQ = 2) with ragged steps and row lists: the same grouped sweep
    differentiated three times gives the same bits in every gradient. D = 128 takes the 4 096-slot update's row-list
    products; D = 24 is narrower than one k-tile of them, so lstm.LstmGroup must take the dense projection (it used to hand
    the row lists to a product that refused them)."""
    from egopose_amd import lstm as hl
    T, B, H = 60, 5120, 64
    rng = np.random.RandomState(5)
    g = torch.Generator(device="cuda").manual_seed(5)
    cells = _cells(4, D, H, seed=5)
    x = torch.randn(T, B, D, device="cuda", generator=g)
    steps = _steps(rng, B, T)
    rg = hl.ragged_order(steps, torch.device("cuda"), T=T)
    assert rg.rows is not None
    inside = (torch.arange(T).unsqueeze(1) < torch.as_tensor(steps).unsqueeze(0)).unsqueeze(2).cuda()
    ws = [torch.randn(T, B, H, device="cuda", generator=g) * inside for _ in range(4)]

    def grads():
        hs = hl.lstm_group(x, cells, [False, True, False, True], ragged=rg)
        torch.autograd.backward(hs, ws)
        return _hip_grads(cells, x)[1:]

    first = grads()
    assert all(bool(torch.isfinite(t).all()) for t in first)
    for _ in range(2):
        for a, b in zip(first, grads()):
            assert torch.equal(a, b)


def test_8_row_and_4_row_workgroups_agree():
    """The first 4095 sequences of a B = 4096 run (8-row workgroups) against a B = 4095 run (4-row workgroups, last one
    ragged): outputs in training and inference within 4, d_x within 8 units of 2^-23 x the scale. Measured: outputs 0 and
    2.1 units in two sessions, d_x 2.1."""
    from egopose_amd import lstm as hl
    T, D, H = 62, 128, 64
    g = torch.Generator(device="cuda").manual_seed(4096)
    cells = _cells(2, D, H, seed=4096)
    x = torch.randn(T, 4096, D, device="cuda", generator=g)
    dys = [torch.randn(T, 4096, H, device="cuda", generator=g) for _ in range(2)]
    res = []
    for B in (4096, 4095):
        xx = x[:, :B].clone().requires_grad_(True)
        outs = hl.lstm_group(xx, cells, [False, True])
        torch.autograd.backward(outs, [d[:, :B] for d in dys])
        with torch.no_grad():
            inf = hl.lstm_group(x[:, :B].contiguous(), cells, [False, True])
        res.append(([o.detach()[:, :4095] for o in outs], [o[:, :4095] for o in inf], xx.grad[:, :4095]))
        for c in cells:
            c.zero_grad(set_to_none=True)
    (o8, i8, dx8), (o4, i4, dx4) = res
    ulp = 2.0 ** -23
    diffs = [float((a - b).abs().max()) / (ulp * float(b.abs().max())) for a, b in zip(o8 + i8 + [dx8], o4 + i4 + [dx4])]
    print("\n8-row against 4-row workgroups, max difference in units of 2^-23 x the scale (out, no_grad out, d_x):", diffs)
    assert max(diffs[:-1]) <= 4.0 and diffs[-1] <= 8.0


def test_profiler_sees_every_instantiation():
    """Every k_lstm_fwd_mfma<NQ, LH, FULL, TRAIN> and k_lstm_bwd_mfma<NQ, LH, FULL> is launched by the shapes of this file's
    cases (B = 7 / 8, 4100 / 4096 at hidden 64, 45 / 44 at hidden 128; training and inference), as the torch profiler
    records them."""
    from torch.profiler import ProfilerActivity, profile
    from egopose_amd import lstm as hl
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for H, B in [(64, 7), (64, 8), (64, 4100), (64, 4096), (128, 45), (128, 44)]:
            cells = _cells(2, 16, H, seed=B)
            x = torch.randn(5, B, 16, device="cuda")
            torch.autograd.backward(hl.lstm_group(x, cells, [False, True]), [torch.ones(5, B, H, device="cuda")] * 2)
            with torch.no_grad():
                hl.lstm_group(x, cells, [False, True])
        torch.cuda.synchronize()
    b = lambda v: v in ("true", "1")
    seen = set()
    for e in prof.key_averages():
        m = re.search(r"k_lstm_(fwd|bwd)_mfma<(\d+), ?(\d+), ?(true|false|1|0)(?:, ?(true|false|1|0))?>", e.key)
        if m:
            seen.add((m.group(1), int(m.group(2)), int(m.group(3)), b(m.group(4))) + ((b(m.group(5)),) if m.group(5) else ()))
    want = {("fwd", nq, lh, full, train) for nq, lh in ((1, 64), (2, 64), (1, 128)) for full in (True, False) for train in (True, False)}
    want |= {("bwd", nq, lh, full) for nq, lh in ((1, 64), (2, 64), (1, 128)) for full in (True, False)}
    assert want <= seen, sorted(want - seen)
