"""Temporal convolutional video net (models/tcn.py:15-70 of the reference) on time-major (T, B, C) batches.

One residual block per entry of `num_channels`, dilation 2**i: two weight-normalised dilated convolutions, each followed by
ReLU (and dropout), a plain 1x1 `downsample` on the residual when the width changes, ReLU(out + res) at the end. Parameter
names and their order are the reference's (`network.i.conv1.{bias,weight_g,weight_v}`, the `network.i.net.N` aliases of the
same modules, `network.i.downsample`), so its checkpoints load with strict=True and ours load there.

In the (T*B, C) matrix of a time-major batch a tap of the convolution is the same matrix shifted by s*B whole rows:

    out[r, :] = b + sum_j X[r + s_j*B, :] W[:, :, j]^T        s_j = j*d - pad, rows whose time step leaves [0, T) are zero

Two ways to run a block:
  HIP    csrc/egp_tcn.hip (`egp_tcn_conv_f32`, exact-float32 MFMA): float32 on the device, channel counts multiples of 16 up
         to 512, odd kernel_size <= 7. Forward is two launches per block (conv1; conv2 with the residual product, the add and
         the last ReLU in its epilogue), the data gradient two more (the same kernel with the weights transposed and the
         shifts negated); the weight gradients are one `gemm.linear_wgrad` per tap over contiguous row slices.
  torch  K `addmm` calls on row slices, plain autograd: every other dtype / device / shape (an empty batch among them), and
         `EGP_TCN=torch`.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch
import torch.nn as nn

from . import _lib as L
from . import gemm as G

_IMPL = os.environ.get("EGP_TCN", "hip")        # "torch" forces the plain-ops path (A/B runs), as EGP_LSTM does for the LSTM
MAX_TAPS = 7
MAX_CHANNELS = 512
HIP_CALLS = 0                                   # launches of egp_tcn_conv_f32 so far (tests assert which path ran)


def tap_shifts(kernel_size, dilation, causal):
    """Time shift s_j of every tap: out[t] reads x[t + s_j]."""
    pad = (kernel_size - 1) * dilation // (1 if causal else 2)
    return [j * dilation - pad for j in range(kernel_size)]


def _channels_ok(c):
    return c % 16 == 0 and 16 <= c <= MAX_CHANNELS


def hip_available(x, c_in, c_out, kernel_size, params):
    return (_IMPL != "torch" and x.is_cuda and x.dtype == torch.float32 and _channels_ok(c_in) and _channels_ok(c_out)
            and kernel_size % 2 == 1 and kernel_size <= MAX_TAPS and all(p is None or p.dtype == torch.float32 for p in params))


def _rows(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1)):
        raise ValueError("%s must be a 2-D float32 HIP tensor with contiguous rows, got %s %s" % (name, tuple(t.shape), t.dtype))
    return t


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _vec(t):
    """`t` where the kernel can read it 16 bytes at a time, else a copy that is (a parameter that lives in a flat optimizer
    buffer starts at any 4-byte offset)."""
    if t is None or (t.data_ptr() % 16 == 0 and (t.dim() < 2 or t.shape[0] == 1 or t.stride(0) % 4 == 0)):
        return t
    return t.clone(memory_format=torch.contiguous_format)


def conv_rows(x, T, B, w, shift0, dshift, bias=None, relu=False, mask=None, gate=None, x2=None, w2=None, b2=None,
              x2_after_act=False, out=None, out2=None):
    """One launch of `egp_tcn_conv_f32` (include/egopose_hip.h). x: (T*B, C_in) rows, w: (taps, C_out, C_in) contiguous.
        v = sum_j x[r + (shift0 + j*dshift)*B] w[j]^T  (+ x2 w2^T, or + x2 when w2 is None, unless x2_after_act)
        v = v + bias;  relu;  * mask;  * (gate > 0)                  -> out2 (when given)
        x2_after_act:  v = relu(v + x2 w2^T + b2)                    -> out
    `out` / `out2`: (T*B, C_out) row views to write into (allocated when `out` is None). Returns out."""
    global HIP_CALLS
    if w.dim() != 3 or not w.is_contiguous() or w.dtype != torch.float32:
        raise ValueError("w must be contiguous float32 (taps, C_out, C_in), got %s %s" % (tuple(w.shape), w.dtype))
    if w2 is not None and (w2.dim() != 2 or not w2.is_contiguous() or w2.dtype != torch.float32):
        raise ValueError("w2 must be contiguous float32 (C_out, C2), got %s %s" % (tuple(w2.shape), w2.dtype))
    if b2 is not None and (x2 is None or w2 is None):
        raise ValueError("b2 goes with the second product only: it needs x2 and w2")
    taps, c_out, c_in = w.shape
    M = T * B
    # an identity x2 is read element by element, at any offset and leading dimension
    x, w, x2, w2 = _vec(_rows(x, "x")), _vec(w), (_vec(x2) if w2 is not None else x2), _vec(w2)
    if x.shape != (M, c_in):
        raise ValueError("x must be (T*B, C_in) = (%d, %d), got %s" % (M, c_in, tuple(x.shape)))
    if out is None:
        out = torch.empty(M, c_out, dtype=torch.float32, device=x.device)
    d = L.TcnDesc()
    d.T, d.B, d.C_in, d.C_out, d.taps, d.shift0, d.dshift = T, B, c_in, c_out, taps, shift0, dshift
    d.X, d.ldx, d.W = x.data_ptr(), _ld(x), w.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.relu = 1 if relu else 0
    for name, t in (("mask", mask), ("gate", gate), ("out", out), ("out2", out2)):
        if t is not None and _rows(t, name).shape != (M, c_out):
            raise ValueError("%s must be (%d, %d), got %s" % (name, M, c_out, tuple(t.shape)))
    if mask is not None:
        d.mask, d.ldmask = mask.data_ptr(), _ld(mask)
    if gate is not None:
        d.gate, d.ldgate = gate.data_ptr(), _ld(gate)
    if x2 is not None:
        if _rows(x2, "x2").shape[0] != M:
            raise ValueError("x2 must have %d rows, got %d" % (M, x2.shape[0]))
        d.X2, d.ldx2, d.C2 = x2.data_ptr(), _ld(x2), x2.shape[1]
        if w2 is not None:
            if w2.shape != (c_out, x2.shape[1]) or not w2.is_contiguous() or w2.dtype != torch.float32:
                raise ValueError("w2 must be contiguous float32 (C_out, C2)")
            d.W2 = w2.data_ptr()
            d.b2 = b2.data_ptr() if b2 is not None else None
        d.x2_after_act = 1 if x2_after_act else 0
    d.out, d.ldout = out.data_ptr(), _ld(out)
    if out2 is not None:
        d.out2, d.ldout2 = out2.data_ptr(), _ld(out2)
    if M == 0:          # no row to compute; empty tensors have no address the launcher would accept
        if not (_channels_ok(c_in) and _channels_ok(c_out) and 1 <= taps <= MAX_TAPS):
            raise ValueError("C_in and C_out must be multiples of 16 in [16, %d], 1 to %d taps" % (MAX_CHANNELS, MAX_TAPS))
        return out
    L.check(L.load().egp_tcn_conv_f32(C.byref(d), L.current_stream()), "egp_tcn_conv_f32")
    HIP_CALLS += 1
    return out


def _pack(w, transpose):
    """(C_out, C_in, K) conv weight -> the kernel's (K, C_out, C_in); transposed (K, C_in, C_out) for the data gradient."""
    return (w.permute(2, 1, 0) if transpose else w.permute(2, 0, 1)).contiguous()


def _tap_rows(T, B, s):
    """Row ranges (of the output, of the input) on which tap shift s stays inside [0, T), or None."""
    t0, t1 = max(0, -s), min(T, T - s)
    if t1 <= t0:
        return None
    return slice(t0 * B, t1 * B), slice((t0 + s) * B, (t1 + s) * B)


def _conv_wgrad(dpre, x, T, B, shifts, want_bias):
    """dW (C_out, C_in, K) = per tap dpre[valid rows]^T x[valid rows + s_j*B]; db from the tap with s_j = 0 (all rows)."""
    c_out, c_in = dpre.shape[1], x.shape[1]
    dw = dpre.new_zeros(len(shifts), c_out, c_in)
    db = None
    for j, s in enumerate(shifts):
        rows = _tap_rows(T, B, s)
        if rows is None:
            continue
        dy, xs = dpre[rows[0]], x[rows[1]]
        bias_here = want_bias and s == 0
        if G.enabled():
            res = G.linear_wgrad(dy, xs, want_bias=bias_here)
            dw[j], db = (res[0], res[1]) if bias_here else (res, db)
        else:
            dw[j] = dy.t().mm(xs)
            if bias_here:
                db = dy.sum(0)
    return dw.permute(1, 2, 0), db


class TcnBlock(torch.autograd.Function):
    """One residual block on the HIP kernel. Saved for backward: the block input, both post-ReLU(-dropout) activations and the
    block output (their signs are the ReLU gates), the weights, and the dropout masks when there are any."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, wd, bd, m1, m2, dilation, causal, train):
        T, B, c_in = x.shape
        c_out, _, K = w1.shape
        M = T * B
        x2 = x.reshape(M, c_in)
        s = tap_shifts(K, dilation, causal)
        mm1 = m1.reshape(M, c_out) if m1 is not None else None
        mm2 = m2.reshape(M, c_out) if m2 is not None else None
        a1 = conv_rows(x2, T, B, _pack(w1, False), s[0], dilation, bias=b1, relu=True, mask=mm1)
        a2 = torch.empty_like(a1) if train else None
        o = conv_rows(a1, T, B, _pack(w2, False), s[0], dilation, bias=b2, relu=True, mask=mm2, x2=x2,
                      w2=wd.reshape(c_out, c_in).contiguous() if wd is not None else None, b2=bd, x2_after_act=True, out2=a2)
        if train:
            ctx.save_for_backward(x2, a1, a2, o, w1, w2, wd, mm1, mm2)
            ctx.meta = (T, B, dilation, s)
        return o.view(T, B, c_out)

    @staticmethod
    def backward(ctx, do):
        x2, a1, a2, o, w1, w2, wd, mm1, mm2 = ctx.saved_tensors
        T, B, dilation, s = ctx.meta
        c_out, c_in = a1.shape[1], x2.shape[1]
        zero = o.new_zeros(())
        g = torch.where(o > 0, do.reshape(T * B, c_out), zero)                 # through the last ReLU: both branches see it
        dpre2 = torch.where(a2 > 0, g, zero)
        if mm2 is not None:
            dpre2 = dpre2 * mm2
        need = ctx.needs_input_grad
        dw2, db2 = _conv_wgrad(dpre2, a1, T, B, s, True)
        # data gradient = the same sum of row-shifted products with the weights transposed and the shifts negated; the gate and
        # the dropout mask of conv1's activation are applied by the launch that produces it
        dpre1 = conv_rows(dpre2, T, B, _pack(w2, True), -s[0], -dilation, mask=mm1, gate=a1)
        dw1, db1 = _conv_wgrad(dpre1, x2, T, B, s, True)
        dwd = dbd = None
        if wd is not None:
            if G.enabled():
                dwd, dbd = G.linear_wgrad(g, x2, want_bias=True)
            else:
                dwd, dbd = g.t().mm(x2), g.sum(0)
            dwd = dwd.view(c_out, c_in, 1)
        dx = None
        if need[0]:           # the residual branch's share (g W_d, or g itself) is summed in the same launch
            dx = conv_rows(dpre1, T, B, _pack(w1, True), -s[0], -dilation, x2=g,
                           w2=wd.reshape(c_out, c_in).t().contiguous() if wd is not None else None).view(T, B, c_in)
        return dx, dw1, db1, dw2, db2, dwd, dbd, None, None, None, None, None


def _conv_torch(x2, T, B, w, b, shifts):
    out = b.unsqueeze(0).repeat(T * B, 1)
    for j, s in enumerate(shifts):
        rows = _tap_rows(T, B, s)
        if rows is not None:           # one product per tap over the rows it reaches, zero rows around it
            part = x2[rows[1]].mm(w[:, :, j].t())
            out = out + nn.functional.pad(part, (0, 0, rows[0].start, T * B - rows[0].stop))
    return out


def block_torch(x, w1, b1, w2, b2, wd, bd, m1, m2, dilation, causal):
    """The block in plain torch ops on (T, B, C): the fallback and the float64 yardstick."""
    T, B, c_in = x.shape
    c_out, _, K = w1.shape
    s = tap_shifts(K, dilation, causal)
    x2 = x.reshape(T * B, c_in)
    a1 = torch.relu(_conv_torch(x2, T, B, w1, b1, s))
    if m1 is not None:
        a1 = a1 * m1.reshape(T * B, c_out)
    a2 = torch.relu(_conv_torch(a1, T, B, w2, b2, s))
    if m2 is not None:
        a2 = a2 * m2.reshape(T * B, c_out)
    res = x2 if wd is None else torch.addmm(bd, x2, wd.reshape(c_out, c_in).t())
    return torch.relu(a2 + res).view(T, B, c_out)


def run_block(x, w1, b1, w2, b2, wd, bd, m1, m2, dilation, causal):
    """A block on whichever path serves `x` (the same masks either way)."""
    c_out, c_in, K = w1.shape
    params = (w1, b1, w2, b2, wd, bd)
    # an empty batch has nothing to launch: the plain ops give the empty result and zero (or no) parameter gradients
    if x.shape[0] * x.shape[1] > 0 and hip_available(x, c_in, c_out, K, params + (m1, m2)):
        train = torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params))
        return TcnBlock.apply(x.contiguous(), w1, b1, w2, b2, wd, bd, m1, m2, dilation, causal, train)
    return block_torch(x, w1, b1, w2, b2, wd, bd, m1, m2, dilation, causal)


class WeightNormConv1d(nn.Module):
    """Parameters of a weight-normalised Conv1d under the names and in the order `torch.nn.utils.weight_norm` leaves them
    (bias, weight_g (C_out, 1, 1), weight_v (C_out, C_in, K)); weight = g v / ||v||, the norm over dims (1, 2). Initialised
    as the reference's modules end up: nn.Conv1d's default draw for v and the bias, g = ||v||."""

    def __init__(self, c_in, c_out, kernel_size):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = c_in, c_out, kernel_size
        self.bias = nn.Parameter(torch.empty(c_out))
        v = torch.empty(c_out, c_in, kernel_size)
        nn.init.kaiming_uniform_(v, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(c_in * kernel_size)
        nn.init.uniform_(self.bias, -bound, bound)
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).view(-1, 1, 1))
        self.weight_v = nn.Parameter(v)

    @property
    def weight(self):
        v = self.weight_v
        return v * (self.weight_g / v.flatten(1).norm(dim=1).view(-1, 1, 1))


class Chomp1d(nn.Module):
    """Place holder of the reference's causal trim in `net` (the padding is one-sided here, nothing to trim)."""

    def __init__(self, chomp_size):
        super().__init__()
        self.chomp_size = chomp_size


class TemporalBlock(nn.Module):
    def __init__(self, n_inputs, n_outputs, kernel_size, dilation, dropout, causal):
        super().__init__()
        self.dilation, self.dropout, self.causal = dilation, float(dropout), bool(causal)
        pad = (kernel_size - 1) * dilation // (1 if causal else 2)
        self.conv1 = WeightNormConv1d(n_inputs, n_outputs, kernel_size)
        self.conv2 = WeightNormConv1d(n_outputs, n_outputs, kernel_size)
        # `net` only reproduces the reference's module numbering (state-dict aliases net.0 / net.N of conv1 / conv2)
        mods = []
        for conv in (self.conv1, self.conv2):
            mods.append(conv)
            if causal:
                mods.append(Chomp1d(pad))
            mods.append(nn.ReLU())
            if dropout > 0:
                mods.append(nn.Dropout(dropout))
        self.net = nn.Sequential(*mods)
        self.downsample = nn.Conv1d(n_inputs, n_outputs, 1) if n_inputs != n_outputs else None
        if self.downsample is not None:
            nn.init.normal_(self.downsample.weight, 0.0, 0.01)
        self.relu = nn.ReLU()

    def _mask(self, x, c_out):
        if not (self.training and self.dropout > 0):
            return None
        keep = 1.0 - self.dropout
        return torch.empty(x.shape[0], x.shape[1], c_out, dtype=x.dtype, device=x.device).bernoulli_(keep).div_(keep)

    def forward_tm(self, x, masks=None):
        """x (T, B, C_in) -> (T, B, C_out). `masks` = (m1, m2) dropout mask-scale tensors to use instead of drawing them."""
        c_out = self.conv1.out_channels
        m1, m2 = masks if masks is not None else (self._mask(x, c_out), self._mask(x, c_out))
        ds = self.downsample
        return run_block(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                         ds.weight if ds is not None else None, ds.bias if ds is not None else None, m1, m2, self.dilation, self.causal)

    def forward(self, x):
        return self.forward_tm(x.permute(2, 0, 1)).permute(1, 2, 0)


class TemporalConvNet(nn.Module):
    """`forward` keeps the reference's (B, C, T) -> (B, C_out, T); the video nets call `forward_tm` on (T, B, C)."""

    def __init__(self, num_inputs, num_channels, kernel_size=3, dropout=0.2, causal=False):
        super().__init__()
        if kernel_size % 2 != 1:
            raise ValueError("TemporalConvNet needs an odd kernel_size, got %r" % (kernel_size,))
        self.num_inputs, self.out_dim, self.kernel_size, self.causal = num_inputs, num_channels[-1], kernel_size, bool(causal)
        dims = [num_inputs] + list(num_channels)
        self.network = nn.Sequential(*[TemporalBlock(dims[i], dims[i + 1], kernel_size, 2 ** i, dropout, causal)
                                       for i in range(len(num_channels))])

    def forward_tm(self, x):
        for block in self.network:
            x = block.forward_tm(x)
        return x

    def forward(self, x):
        return self.forward_tm(x.permute(2, 0, 1)).permute(1, 2, 0)


def from_param(input_dim, v_hdim, v_net_param, causal):
    """The net the reference builds from `v_net_param` (models/video_state_net.py:17-24)."""
    p = v_net_param or {}
    size = list(p.get("size", [64, 128]))
    if size[-1] != v_hdim:
        raise ValueError("tcn: the last entry of v_net_param['size'] (%r) must equal v_hdim (%d)" % (size, v_hdim))
    return TemporalConvNet(input_dim, size, kernel_size=p.get("kernel_size", 3), dropout=p.get("dropout", 0.2), causal=causal)
