"""Rollout-time policy step through `egp_policy_step_f32` (csrc/egp_policy.hip): the VideoStateNet concat, the MLP
and the Gaussian head of the reference's `policy_net.select_action` (core/agent.py:38-44, models/policy_gaussian.py:
19-27, models/mlp.py:5-25) for a whole env group in one launch. The module keeps transposed float32 copies of the
weights, packed for the kernel's matrix-core tiles, in persistent buffers (`refresh()` re-reads the live parameters,
addresses stay fixed for hipGraphs). Every class fills one `egp_policy_desc` per call. `FusedForecastPolicy` is the
ego_forecast form (the descriptor's `cell`): one step of VideoForecastNet's state LSTM cell (models/video_forecast_net.py:
88-93, models/rnn.py:29-36) in front of the same MLP, the cell's h / c updated in place; its `with_filter` (the filter
block) puts the observation filter's apply pass in front of it, merged with a tick's tile statistics or frozen.
`FusedActorCritic` is the ego_mimic evaluation's tick (the descriptor's `vlayers`): the frozen filter, the policy step and
the value net of the same rows in one launch."""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib as L

_ACT_CODE = {torch.tanh: 0, torch.relu: 1, torch.sigmoid: 2}


def _addr(t):
    return t.data_ptr() if t is not None else None


def _check_io(ctx_rows, t_idx, state, action_out, noise, mean_out, nu):
    """The tensors every policy step takes: dtypes, layouts and the [n][nu] shapes of the outputs."""
    n, T, H = ctx_rows.shape
    assert ctx_rows.dtype == torch.float32 and ctx_rows.stride(2) == 1 and ctx_rows.stride(1) == H
    assert t_idx.dtype == torch.int64 and t_idx.is_contiguous() and state.dtype == torch.float64 and state.is_contiguous()
    assert action_out.dtype == torch.float64 and action_out.is_contiguous() and action_out.shape == (n, nu)
    if noise is not None:
        assert noise.dtype == torch.float32 and noise.is_contiguous() and noise.shape == (n, nu)
    if mean_out is not None:
        assert mean_out.dtype == torch.float32 and mean_out.is_contiguous() and mean_out.shape == (n, nu)


def supported(policy_net) -> bool:
    """True when `policy_net` is a PolicyGaussian over a plain MLP with an activation the kernel implements."""
    net = getattr(policy_net, "net", None)
    return (getattr(policy_net, "type", None) == "gaussian" and hasattr(net, "affine_layers")
            and getattr(net, "activation", None) in _ACT_CODE and hasattr(policy_net, "action_mean")
            and len(net.affine_layers) + 1 <= 8 and policy_net.action_mean.weight.dtype == torch.float32
            and max(l.out_features for l in net.affine_layers) <= 2048)


def supported_value(value_net) -> bool:
    """True when `value_net` is a Value over a plain float32 MLP with an activation the kernel implements, inside its limits."""
    net, head = getattr(value_net, "net", None), getattr(value_net, "value_head", None)
    return (isinstance(head, nn.Linear) and head.out_features == 1 and hasattr(net, "affine_layers") and len(net.affine_layers) >= 1
            and getattr(net, "activation", None) in _ACT_CODE and len(net.affine_layers) + 1 <= 8
            and head.weight.dtype == torch.float32 and all(l.weight.dtype == torch.float32 for l in net.affine_layers)
            and head.in_features == net.affine_layers[-1].out_features
            and max(max(l.in_features, l.out_features) for l in net.affine_layers) <= 2048)


def supported_forecast(policy_net, vs_net) -> bool:
    """True when `supported(policy_net)` and `vs_net` is a VideoForecastNet whose state net is one float32 nn.LSTMCell
    (with biases, one direction) inside the kernel's limits. (`s_net_type == 'id'` passes the state through unchanged:
    that is FusedGaussianPolicy's input already.)"""
    s_net = getattr(vs_net, "s_net", None)
    cell = getattr(s_net, "rnn_f", None)
    if not (supported(policy_net) and getattr(vs_net, "s_net_type", None) == "lstm" and isinstance(cell, nn.LSTMCell)
            and cell.bias and not getattr(s_net, "bi_dir", False) and cell.weight_ih.dtype == torch.float32):
        return False
    S, Hs = cell.input_size, cell.hidden_size
    return (S >= 1 and Hs >= 1 and 4 * Hs <= 2048 and S + Hs <= 2048 and len(policy_net.net.affine_layers) + 1 <= 7
            and policy_net.net.affine_layers[0].in_features == vs_net.v_hdim + Hs and vs_net.v_hdim + Hs <= 2048)


class FusedGaussianPolicy:

    def __init__(self, policy_net, device, _front=(), _back=()):
        if not supported(policy_net):
            raise ValueError("policy net is not a float32 PolicyGaussian over an MLP")
        self.lib = L.load()
        self.net = policy_net
        self.layers = list(policy_net.net.affine_layers) + [policy_net.action_mean]
        self.act = _ACT_CODE[policy_net.net.activation]
        # the kernel's packed weight form (include/egopose_hip.h: egp_mlp_layer): one 64-column x 4-feature block per wave load
        # (ONE buffer, layer after layer: the kernel's L2 warm-up walks it as a single range)
        # (`_front` / `_back`: (in, out) of packed layers a subclass keeps in front of / behind the MLP's, in the same allocation)
        dims = list(_front) + [(l.in_features, l.out_features) for l in self.layers] + list(_back)
        sizes = [int(self.lib.egp_mlp_pack_floats(i, o)) for i, o in dims]
        self.wt_all = torch.zeros(sum(sizes), dtype=torch.float32, device=device)
        parts = list(torch.split(self.wt_all, sizes))
        self.front_wt, self.wt, self.back_wt = parts[:len(_front)], parts[len(_front):len(parts) - len(_back)], parts[len(parts) - len(_back):]
        self.bias = [torch.empty(l.out_features, dtype=torch.float32, device=device) for l in self.layers]
        self.log_std = torch.empty(self.layers[-1].out_features, dtype=torch.float32, device=device)
        self.desc = (L.MlpLayer * len(self.layers))()
        for i, l in enumerate(self.layers):
            self.desc[i].wt = self.wt[i].data_ptr()
            self.desc[i].bias = self.bias[i].data_ptr()
            self.desc[i].in_dim, self.desc[i].out_dim = l.in_features, l.out_features
        self.in_dim = self.layers[0].in_features
        self.nu = self.layers[-1].out_features
        self.refresh()

    @torch.no_grad()
    def refresh(self):
        """Pack the live parameters into the kernel's buffers (call once per rollout, after the optimiser step)."""
        stream = L.current_stream()
        for l, wt, b in zip(self.layers, self.wt, self.bias):
            w = l.weight if l.weight.stride(1) == 1 else l.weight.contiguous()
            L.check(self.lib.egp_mlp_pack_f32(C.c_void_p(w.data_ptr()), int(w.stride(0)), l.in_features, l.out_features,
                                              C.c_void_p(wt.data_ptr()), stream), "egp_mlp_pack_f32")
            b.copy_(l.bias)
        self.log_std.copy_(self.net.action_log_std.reshape(-1))

    def __call__(self, ctx_rows, t_idx, state, action_out, noise=None, mean_out=None):
        """ctx_rows: float32 [n][T][H] (contiguous slab of per-slot context tables), t_idx: int64 [n],
        state: float64 [n][S], noise: float32 [n][nu] or None (mean action), action_out: float64 [n][nu]."""
        n, T, H = ctx_rows.shape
        S = state.shape[1]
        if H + S != self.in_dim:
            raise ValueError("context dim %d + state dim %d != policy input %d" % (H, S, self.in_dim))
        _check_io(ctx_rows, t_idx, state, action_out, noise, mean_out, self.nu)
        d = self._desc(ctx_rows, t_idx, action_out, noise, mean_out)
        d.state, d.state_dim = _addr(state), S
        return self._step(d, action_out)

    def _desc(self, ctx_rows, t_idx, action_out, noise, mean_out):
        """A PolicyDesc (built per call: the tensors change) with the fields every step shares: rows, context, actor, outputs."""
        d = L.PolicyDesc()
        d.n, _, d.ctx_dim = ctx_rows.shape
        d.ctx_rows, d.ctx_row_stride, d.t_idx = _addr(ctx_rows), ctx_rows.stride(0), _addr(t_idx)
        d.layers, d.n_layers, d.activation, d.log_std = self.desc, len(self.layers), self.act, _addr(self.log_std)
        d.noise, d.action, d.mean_out = _addr(noise), _addr(action_out), _addr(mean_out)
        return d

    def _filter(self, d, ctx, qpos, qvel, phase_t, zf_in, zf_out, clip, y, y2, workspace):
        """The descriptor's filter block."""
        d.ctx, d.qpos, d.qvel, d.phase_t = ctx.handle, _addr(qpos), _addr(qvel), _addr(ctx._phase_t(phase_t, d.n))
        d.zf_in, d.zf_out, d.clip = _addr(zf_in), _addr(zf_out), float(clip or 0.0)
        d.y, d.y2, d.zf_workspace = _addr(y), _addr(y2), _addr(workspace)

    def _step(self, d, action_out):
        L.check(self.lib.egp_policy_step_f32(C.byref(d), L.current_stream()), "egp_policy_step_f32")
        return action_out

    def _zf_scratch(self, zf_in):
        if getattr(self, "_zf_copy", None) is None or self._zf_copy.shape != zf_in.shape or self._zf_copy.device != zf_in.device:
            self._zf_copy = torch.empty_like(zf_in)
        return self._zf_copy

    def with_filter(self, ctx, ctx_rows, t_idx, qpos, qvel, zf_in, zf_out, clip, y, y2, workspace, action_out, noise=None, mean_out=None,
                    phase_t=None):
        """The filter's apply pass + the policy step in one launch (`egp_policy_step_f32` with the filter block): the state columns are the
        observations of (qpos, qvel) normalised with `zf_in` merged with the tile statistics `ctx.obs_zfilter_stats` left in
        `workspace`; y / y2 receive them, `zf_out` the merged statistics. `workspace=None`: `zf_in` as it stands -- the frozen
        filter of an evaluation, `running_state(x, update=False)`; `zf_out` may be None then. `ctx`: the EgpContext of the model."""
        n, T, H = ctx_rows.shape
        if workspace is None and zf_out is None:      # the frozen filter (`zf_in` as it stands): the kernel still writes its copy of the statistics
            zf_out = self._zf_scratch(zf_in)
        d = self._desc(ctx_rows, t_idx, action_out, noise, mean_out)
        self._filter(d, ctx, qpos, qvel, phase_t, zf_in, zf_out, clip, y, y2, workspace)
        return self._step(d, action_out)


class FusedForecastPolicy(FusedGaussianPolicy):
    """The ego_forecast tick in one launch (`egp_policy_step_f32` with `cell`): state LSTM cell step, [context | h'] -> MLP -> Gaussian
    head, h / c written back in place. The cell's packed gate layer sits in front of the MLP's in `wt_all`."""

    def __init__(self, policy_net, vs_net, device):
        if not supported_forecast(policy_net, vs_net):
            raise ValueError("not a float32 PolicyGaussian over an MLP behind a VideoForecastNet with an LSTMCell state net")
        self.cell = vs_net.s_net.rnn_f
        self.S, self.Hs = self.cell.input_size, self.cell.hidden_size
        self.cell_bias = torch.empty(4 * self.Hs, dtype=torch.float32, device=device)
        super().__init__(policy_net, device, _front=[(self.S + self.Hs, 4 * self.Hs)])
        self.cell_desc = (L.MlpLayer * 1)()
        self.cell_desc[0].wt = self.front_wt[0].data_ptr()
        self.cell_desc[0].bias = self.cell_bias.data_ptr()
        self.cell_desc[0].in_dim, self.cell_desc[0].out_dim = self.S + self.Hs, 4 * self.Hs

    @torch.no_grad()
    def refresh(self):
        """Pack the live parameters of the cell and of the MLP into the kernel's buffers."""
        super().refresh()
        c, S, Hs = self.cell, self.S, self.Hs
        # the kernel's gate layer (include/egopose_hip.h): row 4 u + g = [W_ih[g Hs + u] | W_hh[g Hs + u]], bias b_ih + b_hh alike
        w = torch.cat((c.weight_ih, c.weight_hh), 1).view(4, Hs, S + Hs).transpose(0, 1).reshape(4 * Hs, S + Hs).contiguous()
        L.check(self.lib.egp_mlp_pack_f32(C.c_void_p(w.data_ptr()), S + Hs, S + Hs, 4 * Hs, C.c_void_p(self.front_wt[0].data_ptr()),
                                          L.current_stream()), "egp_mlp_pack_f32")
        self.cell_bias.copy_((c.bias_ih + c.bias_hh).view(4, Hs).t().reshape(-1))

    def __call__(self, ctx_rows, t_idx, state, h, c, action_out, noise=None, mean_out=None):
        """ctx_rows: float32 [n][T][H], t_idx: int64 [n], state: float64 [n][S], h / c: float32 [n][Hs] (row slices of the
        per-slot buffers; updated in place), noise: float32 [n][nu] or None (mean action), action_out: float64 [n][nu]."""
        n, T, H = ctx_rows.shape
        if state.shape[1] != self.S or H + self.Hs != self.in_dim:
            raise ValueError("state dim %d / context dim %d do not fit the cell (%d -> %d) and the policy input %d"
                             % (state.shape[1], H, self.S, self.Hs, self.in_dim))
        _check_io(ctx_rows, t_idx, state, action_out, noise, mean_out, self.nu)
        for t in (h, c):
            assert t.dtype == torch.float32 and t.shape == (n, self.Hs) and t.stride(1) == 1 and t.stride(0) == h.stride(0) >= self.Hs
        assert h.data_ptr() != c.data_ptr()
        d = self._desc(ctx_rows, t_idx, action_out, noise, mean_out)
        d.state, d.state_dim = _addr(state), self.S
        return self._step(self._cell(d, h, c), action_out)

    def _cell(self, d, h, c):
        d.cell, d.h, d.c, d.hc_row_stride = self.cell_desc, _addr(h), _addr(c), h.stride(0)
        return d

    def with_filter(self, ctx, ctx_rows, t_idx, qpos, qvel, zf_in, zf_out, clip, y, y2, workspace, h, c, action_out, noise=None, mean_out=None,
                    phase_t=None):
        """The filter's apply pass + the forecast step in one launch (`cell` and the filter block): the cell's state input is
        the observation of (qpos, qvel), normalised with `zf_in` merged with the tile statistics `ctx.obs_zfilter_stats` left in
        `workspace` (`zf_out` receives the merged statistics), or with `workspace=None` with `zf_in` as it stands -- the frozen
        filter of an evaluation, `running_state(x, update=False)`; `zf_out` may be None then. y (and y2, optional): float64
        [n][obs_dim], the normalised rows. `zf_in=None` (a checkpoint without running_state): the raw observations go to y / y2
        and through the unfiltered step. h / c, noise, action_out, mean_out as in `__call__`. `ctx`: the model's EgpContext."""
        n, T, H = ctx_rows.shape
        S = ctx.obs_dim
        if S != self.S or H + self.Hs != self.in_dim:
            raise ValueError("observation dim %d / context dim %d do not fit the cell (%d -> %d) and the policy input %d"
                             % (S, H, self.S, self.Hs, self.in_dim))
        assert qpos.dtype == torch.float64 and qpos.is_contiguous() and qpos.shape == (n, ctx.nq)
        assert qvel.dtype == torch.float64 and qvel.is_contiguous() and qvel.shape == (n, ctx.nv)
        for t in (y, y2):
            assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and t.shape == (n, S))
        assert y is not None
        _check_io(ctx_rows, t_idx, y, action_out, noise, mean_out, self.nu)
        for t in (h, c):
            assert t.dtype == torch.float32 and t.shape == (n, self.Hs) and t.stride(1) == 1 and t.stride(0) == h.stride(0) >= self.Hs
        assert n == 0 or h.data_ptr() != c.data_ptr()
        if zf_in is None:
            assert workspace is None
            ctx.obs_zfilter(qpos, qvel, None, None, clip, y, out2=y2, phase_t=phase_t)
            return self(ctx_rows, t_idx, y, h, c, action_out, noise=noise, mean_out=mean_out)
        for t in (zf_in, zf_out):
            assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and t.shape == (1 + 2 * S,))
        d = self._desc(ctx_rows, t_idx, action_out, noise, mean_out)
        self._filter(d, ctx, qpos, qvel, phase_t, zf_in, zf_out, clip, y, y2, workspace)
        return self._step(self._cell(d, h, c), action_out)


class FusedActorCritic(FusedGaussianPolicy):
    """The ego_mimic evaluation's tick in one launch (`egp_policy_step_f32` with `vlayers`): observation -> frozen filter ->
    [policy context row | state] -> policy MLP -> Gaussian head, and [value context row | state] -> value MLP -> value_head for
    the same rows. The value net's packed layers sit behind the policy's in `wt_all`."""

    def __init__(self, policy_net, value_net, device):
        if not supported_value(value_net):
            raise ValueError("value net is not a float32 Value over an MLP")
        self.value_net = value_net
        self.vlayers = list(value_net.net.affine_layers) + [value_net.value_head]
        self.vact = _ACT_CODE[value_net.net.activation]
        self.vbias = [torch.empty(l.out_features, dtype=torch.float32, device=device) for l in self.vlayers]
        super().__init__(policy_net, device, _back=[(l.in_features, l.out_features) for l in self.vlayers])
        self.vdesc = (L.MlpLayer * len(self.vlayers))()
        for i, l in enumerate(self.vlayers):
            self.vdesc[i].wt = self.back_wt[i].data_ptr()
            self.vdesc[i].bias = self.vbias[i].data_ptr()
            self.vdesc[i].in_dim, self.vdesc[i].out_dim = l.in_features, l.out_features
        self.v_in_dim = self.vlayers[0].in_features

    @torch.no_grad()
    def refresh(self):
        """Pack the live parameters of both nets into the kernel's buffers."""
        super().refresh()
        stream = L.current_stream()
        for l, wt, b in zip(self.vlayers, self.back_wt, self.vbias):
            w = l.weight if l.weight.stride(1) == 1 else l.weight.contiguous()
            L.check(self.lib.egp_mlp_pack_f32(C.c_void_p(w.data_ptr()), int(w.stride(0)), l.in_features, l.out_features,
                                              C.c_void_p(wt.data_ptr()), stream), "egp_mlp_pack_f32")
            b.copy_(l.bias)

    def with_filter(self, ctx, ctx_rows, t_idx, qpos, qvel, zf_in, zf_out, clip, y, y2, workspace, action_out, value_ctx_rows, value_out,
                    noise=None, mean_out=None, phase_t=None):
        """As `FusedGaussianPolicy.with_filter(..., workspace=None)` (the frozen filter -- `workspace` must be None; actions, y, y2
        bit-identical to it) plus the critic: value_ctx_rows float32 [n][T][Hv] (the value net's context tables, indexed by the same
        `t_idx`), value_out float32 [n]. `zf_in=None` (a checkpoint without running_state): the raw observations go to y / y2 and
        into both nets."""
        if workspace is not None:
            raise ValueError("the actor + critic step normalises with frozen statistics only (workspace=None)")
        n, T, H = ctx_rows.shape
        S = ctx.obs_dim
        nv_, Tv, Hv = value_ctx_rows.shape
        if H + S != self.in_dim or Hv + S != self.v_in_dim or nv_ != n:
            raise ValueError("context dims %d / %d + observation dim %d do not fit the policy input %d / the value input %d"
                             % (H, Hv, S, self.in_dim, self.v_in_dim))
        assert qpos.dtype == torch.float64 and qpos.is_contiguous() and qpos.shape == (n, ctx.nq)
        assert qvel.dtype == torch.float64 and qvel.is_contiguous() and qvel.shape == (n, ctx.nv)
        for t in (y, y2):
            assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and t.shape == (n, S))
        assert y is not None
        _check_io(ctx_rows, t_idx, y, action_out, noise, mean_out, self.nu)
        assert value_ctx_rows.dtype == torch.float32 and value_ctx_rows.stride(2) == 1 and value_ctx_rows.stride(1) == Hv
        assert value_out.dtype == torch.float32 and value_out.is_contiguous() and value_out.numel() == n
        if zf_in is None:
            ctx.obs_zfilter(qpos, qvel, None, None, clip, y, out2=y2, phase_t=phase_t)
        else:
            for t in (zf_in, zf_out):
                assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and t.shape == (1 + 2 * S,))
            if zf_out is None:
                zf_out = self._zf_scratch(zf_in)
        d = self._desc(ctx_rows, t_idx, action_out, noise, mean_out)
        if zf_in is None:
            d.state, d.state_dim = _addr(y), S
        else:
            self._filter(d, ctx, qpos, qvel, phase_t, zf_in, zf_out, clip, y, y2, None)
        d.vctx_rows, d.vctx_row_stride, d.vctx_dim = _addr(value_ctx_rows), value_ctx_rows.stride(0), Hv
        d.vlayers, d.n_vlayers, d.vactivation, d.value_out = self.vdesc, len(self.vlayers), self.vact, _addr(value_out)
        return self._step(d, action_out)
