"""Policy / value / video-context networks on PyTorch-ROCm (GEMMs on MFMA via rocBLAS/hipBLASLt/MIOpen).

Parameter names and shapes are those of the reference so checkpoints stay drop-in
(``net.affine_layers.i``, ``action_mean``, ``action_log_std``, ``value_head``, ``v_net.rnn_f/rnn_b``
holding ``nn.LSTMCell`` parameters): models/mlp.py:5-25, models/rnn.py:5-61,
models/video_state_net.py:7-70, core/policy.py:4-23, core/policy_gaussian.py:7-38, core/critic.py:5-18,
core/distributions.py:6-25 of /root/reference.

What differs is how they run: the temporal net consumes whole batches of windows -- (T, B, D) with B =
all envs that reset this tick / all episodes of the PPO batch -- and the bi-LSTM is evaluated with one
input-projection GEMM per direction plus a fused recurrent sweep (MIOpen ``lstm`` when the dtype allows,
otherwise a cell loop over pre-projected gates) instead of 2*T LSTMCell calls at batch 1.
"""
from __future__ import annotations

import collections
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import dist as _dist
from . import gemm as _gemm
from . import gemm_tuning as _tuning
from . import lstm as _hip_lstm
from . import tcn as _tcn
from .tcn import TemporalConvNet  # noqa: F401  (models/tcn.py: part of the nets' public surface)

# Running the train-mode forward LSTM per length bucket was measured SLOWER on the MI355X -- the persistent sweep is bound by
# its per-timestep latency, not by the batch, so several short launches cost more than one long one -- and the ragged sweeps
# (lstm.ragged_order) replaced it. Running the two directions on two HIP streams was also tried: no gain in the update, and
# an intermittent stall next to the resident K1 streams -- removed.
_LSTM_IMPL = os.environ.get("EGP_LSTM", "hip")      # "torch" forces the MIOpen / cell-loop paths (A/B runs)

_ACT = {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid}


def bucket_rows(x):
    """Zero-pad a big (N, D) batch to the next row bucket so its GEMM shapes come from a small tuned set
    (gemm_tuning.py). Returns (x_padded, N) or (x, None)."""
    if _tuning.enabled() and x.is_cuda and x.dim() == 2 and x.shape[0] >= 4 * _tuning.ROW_BUCKET:
        pad = _tuning.pad_to(x.shape[0], _tuning.ROW_BUCKET)
        if pad:
            return nn.functional.pad(x, (0, 0, 0, pad)), x.shape[0]
    return x, None


def _take_lengths(take_offset, n_rows):
    off = np.asarray(take_offset, dtype=np.int64).ravel()
    return np.diff(np.concatenate((off, [int(n_rows)])))


def _check_windows(take_len, expert_ind, start_ind, before, after):
    """Every window [start - before, start + after) inside its take, else ValueError (host-side, numpy indices)."""
    e = np.asarray(expert_ind, dtype=np.int64).ravel()
    s = np.asarray(start_ind, dtype=np.int64).ravel()
    if e.size == 0:
        return
    if e.min() < 0 or e.max() >= len(take_len):
        raise ValueError("take index out of range: [%d, %d] with %d takes" % (e.min(), e.max(), len(take_len)))
    bad = (s - before < 0) | (s + after > take_len[e])
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise ValueError("CNN-feature window [%d, %d) leaves take %d (%d frames): %d of %d windows do"
                         % (s[k] - before, s[k] + after, e[k], take_len[e[k]], int(bad.sum()), e.size))


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dims=(128, 128), activation="tanh"):
        super().__init__()
        self.activation = _ACT[activation]
        dims = [input_dim] + list(hidden_dims)
        self.out_dim = dims[-1]
        self.affine_layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x):
        for layer in self.affine_layers:
            x = self.activation(layer(x))
        return x


def mlp_head(net, head, x):
    """head(net(x)) for an MLP trunk `net` and an nn.Linear `head`. x: a tensor, or a gemm.GatheredInput ([context | state] not formed)."""
    if _gemm.mlp_head_available(x, getattr(net, "affine_layers", ()), head, getattr(net, "activation", None)):
        # the whole head(MLP(x)) as one autograd node on the split-operand bf16 GEMM kernel (gemm.py)
        if isinstance(x, _gemm.GatheredInput):      # the first layer gathers [context | state] itself
            return _gemm.gather_mlp_head(x, net.affine_layers, head, net.activation)
        # `_egp_ctx_cols` (a tag VideoStateNet.forward leaves on the tensor it returns, not a module attribute): only the leading
        # video-context columns of that input carry a gradient -- any other input gets the full gradient
        return _gemm.mlp_head(x, net.affine_layers, head, getattr(x, "_egp_ctx_cols", None), net.activation)
    if isinstance(x, _gemm.GatheredInput):
        x = x.materialize()
    x, n = bucket_rows(x)
    out = head(net(x))
    return out if n is None else out[:n]


class _DiagLogProb(torch.autograd.Function):
    """sum_j log N(value_j; loc_j, exp(log_std_j)) per row (core/distributions.py: normal_log_density + sum(1, keepdim)) in four
    full-size element-wise kernels forward and two backward (torch.distributions.Normal.log_prob takes about eight each way,
    plus a validity check of the sample that synchronises with the host). log_std: one row (1, d), broadcast over the batch."""

    @staticmethod
    def forward(ctx, value, loc, log_std):
        inv_std = torch.exp(-log_std)
        z = (value - loc) * inv_std
        ctx.save_for_backward(z, inv_std)
        const = log_std.sum() + 0.5 * log_std.shape[-1] * math.log(2.0 * math.pi)
        return (z * z).sum(1, keepdim=True).mul_(-0.5).sub_(const)

    @staticmethod
    def backward(ctx, g):
        z, inv_std = ctx.saved_tensors
        d_loc = d_ls = None
        if ctx.needs_input_grad[1]:
            d_loc = (z * inv_std).mul_(g)
        if ctx.needs_input_grad[2]:
            d_ls = ((z * z - 1.0) * g).sum(0, keepdim=True)
        d_val = None
        if ctx.needs_input_grad[0]:
            d_val = -((z * inv_std) * g)
        return d_val, d_loc, d_ls


class DiagGaussian(torch.distributions.Normal):
    """Normal with summed log-prob and the reference's 'KL to a detached copy of itself'. `log_std_row`: the (1, d) log
    standard deviation the scale was expanded from, when the caller has it (PolicyGaussian): log_prob then takes the short
    route (_DiagLogProb)."""

    def __init__(self, loc, scale, log_std_row=None):
        super().__init__(loc, scale, validate_args=False)       # (the argument checks cost a device reduction + host sync per call)
        self._log_std_row = log_std_row

    def kl(self):
        mu0, s0 = self.loc.detach(), self.scale.detach()
        ls1 = self.scale.log()
        out = ls1 - ls1.detach() + (s0.pow(2) + (mu0 - self.loc).pow(2)) / (2.0 * self.scale.pow(2)) - 0.5
        return out.sum(1, keepdim=True)

    def log_prob(self, value):
        if self._log_std_row is not None and value.dim() == 2:
            return _DiagLogProb.apply(value, self.loc, self._log_std_row)
        return super().log_prob(value).sum(1, keepdim=True)

    def mean_sample(self):
        return self.loc


class Policy(nn.Module):
    def select_action(self, x, mean_action=False):
        dist = self.forward(x)
        return dist.mean_sample() if mean_action else dist.sample()

    def get_kl(self, x):
        return self.forward(x).kl()

    def get_log_prob(self, x, action):
        return self.forward(x).log_prob(action)


class PolicyGaussian(Policy):
    def __init__(self, net, action_dim, net_out_dim=None, log_std=0, fix_std=False):
        super().__init__()
        self.type = "gaussian"
        self.net = net
        self.action_mean = nn.Linear(net.out_dim if net_out_dim is None else net_out_dim, action_dim)
        with torch.no_grad():
            self.action_mean.weight.mul_(0.1)
            self.action_mean.bias.zero_()
        self.action_log_std = nn.Parameter(torch.full((1, action_dim), float(log_std)), requires_grad=not fix_std)

    def mean_std(self, x):
        mean = mlp_head(self.net, self.action_mean, x)
        return mean, torch.exp(self.action_log_std).expand_as(mean)         # (a view: no (n, d) tensor of standard deviations)

    def forward(self, x):
        mean, std = self.mean_std(x)
        return DiagGaussian(mean, std, self.action_log_std if self.action_log_std.dim() == 2 and self.action_log_std.shape[0] == 1 else None)

    def get_fim(self, x):
        mean, _ = self.mean_std(x)
        cov_inv = self.action_log_std.exp().pow(-2).squeeze(0).repeat(x.size(0))
        offset, std_id, std_index = 0, 0, 0
        for i, (name, p) in enumerate(self.named_parameters()):
            if name == "action_log_std":
                std_id, std_index = i, offset
            offset += p.numel()
        return cov_inv.detach(), mean, {"std_id": std_id, "std_index": std_index}


class Value(nn.Module):
    def __init__(self, net, net_out_dim=None):
        super().__init__()
        self.net = net
        self.value_head = nn.Linear(net.out_dim if net_out_dim is None else net_out_dim, 1)
        with torch.no_grad():
            self.value_head.weight.mul_(0.1)
            self.value_head.bias.zero_()

    def forward(self, x):
        return mlp_head(self.net, self.value_head, x)


class Discriminator(nn.Module):
    """The discriminator of ego_pose/core/agent_vgail.py:62-67 (the reference ships the agent, not the net): trunk `net`, one
    logit per row from `logic`, shaped like `Value`. `forward` is the probability the reference's nn.BCELoss takes;
    `logits` is what the fused loss (optim.bce_logits) takes."""

    def __init__(self, net, net_out_dim=None):
        super().__init__()
        self.net = net
        self.logic = nn.Linear(net.out_dim if net_out_dim is None else net_out_dim, 1)
        with torch.no_grad():
            self.logic.weight.mul_(0.1)
            self.logic.bias.zero_()

    def logits(self, x):
        return mlp_head(self.net, self.logic, x)

    def forward(self, x):
        return torch.sigmoid(self.logits(x))


# ------------------------------------------------------------------------------------------------ temporal nets
def _lstm_sweep(cell: nn.LSTMCell, x, reverse):
    """(T,B,D) -> (T,B,H) for one direction; zero initial state."""
    T, B, _ = x.shape
    H = cell.hidden_size
    if _LSTM_IMPL != "torch" and _hip_lstm.available(x, cell):
        return _hip_lstm.lstm_direction(cell, x.contiguous(), reverse)      # persistent HIP recurrence
    fused_ok = x.is_cuda and x.dtype in (torch.float32, torch.float16, torch.bfloat16)
    if fused_ok:
        h0 = x.new_zeros(1, B, H)
        xs = x.flip(0) if reverse else x
        out, _, _ = torch._VF.lstm(xs, (h0, h0), [cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh],
                                   True, 1, 0.0, cell.training, False, False)
        return out.flip(0) if reverse else out
    # generic path: one GEMM for every timestep's input projection, then the recurrence
    gates_x = torch.addmm(cell.bias_ih + cell.bias_hh, x.reshape(T * B, -1), cell.weight_ih.t()).view(T, B, 4 * H)
    w_hh_t = cell.weight_hh.t()
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    outs = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = torch.addmm(gates_x[t], h, w_hh_t)
        i, f, gg, o = g.chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs[t] = h
    return torch.stack(outs, 0)


class RNN(nn.Module):
    def __init__(self, input_dim, out_dim, cell_type="lstm", bi_dir=False):
        super().__init__()
        self.input_dim, self.out_dim, self.cell_type, self.bi_dir = input_dim, out_dim, cell_type, bi_dir
        self.mode = "batch"
        make = nn.LSTMCell if cell_type == "lstm" else nn.GRUCell
        hidden = out_dim // 2 if bi_dir else out_dim
        self.rnn_f = make(input_dim, hidden)
        if bi_dir:
            self.rnn_b = make(input_dim, hidden)
        self.hx = self.cx = None
        self.ragged = None       # set by the caller around a batch forward: (order, steps) of lstm.ragged_order

    def set_mode(self, mode):
        self.mode = mode

    def initialize(self, batch_size=1):
        if self.mode == "step":
            p = self.rnn_f.weight_hh
            self.hx = p.new_zeros(batch_size, self.rnn_f.hidden_size)
            self.cx = p.new_zeros(batch_size, self.rnn_f.hidden_size) if self.cell_type == "lstm" else None

    def _sweep(self, cell, x, reverse):
        if self.cell_type == "lstm":
            return _lstm_sweep(cell, x, reverse)
        h = x.new_zeros(x.size(1), cell.hidden_size)
        outs = [None] * x.size(0)
        for t in (range(x.size(0) - 1, -1, -1) if reverse else range(x.size(0))):
            h = cell(x[t], h)
            outs[t] = h
        return torch.stack(outs, 0)

    def forward(self, x):
        if self.mode == "step":
            self.hx = self.hx.to(x.device)
            if self.cell_type == "lstm":
                self.hx, self.cx = self.rnn_f(x, (self.hx, self.cx.to(x.device)))
            else:
                self.hx = self.rnn_f(x, self.hx)
            return self.hx
        if (self.bi_dir and self.cell_type == "lstm" and _LSTM_IMPL != "torch"
                and _hip_lstm.group_available(x, [self.rnn_f, self.rnn_b])):
            # both directions in one grouped launch each way, writing the halves of one (T, B, 2H) buffer (lstm.LstmGroup)
            return _hip_lstm.lstm_group(x, [self.rnn_f, self.rnn_b], [False, True], pairs=True, ragged=self.ragged)[0]
        out = self._sweep(self.rnn_f, x, False)
        if self.bi_dir:
            out = torch.cat((out, self._sweep(self.rnn_b, x, True)), 2)
        return out


def _video_net(input_dim, v_hdim, v_net_type, v_net_param, causal):
    """The temporal net of the video slot: 'lstm' (bi-directional unless causal) or 'tcn' (tcn.from_param)."""
    if v_net_type == "lstm":
        return RNN(input_dim, v_hdim, v_net_type, bi_dir=not causal)
    if v_net_type == "tcn":
        return _tcn.from_param(input_dim, v_hdim, v_net_param, causal)
    raise ValueError("v_net_type must be 'lstm' or 'tcn', got %r" % (v_net_type,))


def _run_video_net(v_net, x):
    """(T, B, D) -> (T, B, v_hdim); the TCN runs time-major as it is (the reference permutes to (B, C, T) and back,
    models/video_state_net.py:72-78)."""
    return v_net.forward_tm(x) if isinstance(v_net, _tcn.TemporalConvNet) else v_net(x)


_Episodes = collections.namedtuple("_Episodes", "ends starts lens max_len covered ep_of indices meta")


def _segment_episodes(masks, v_metas):
    """The flat batch cut into episodes at masks == 0 (models/video_state_net.py:40-51): per episode its last sample, its first
    one and its length; `max_len`; per sample its episode `ep_of` and `indices` = episode * max_len + offset, its cell of an
    (n_ep, max_len) grid -- the samples from `covered` on, behind the last episode end, keep their own number; `meta`, the
    (take, start frame) row of every episode. One device-to-host sync, then one collective: the padded window length is a
    batch-wide quantity in the reference (one process, one batch) and stays global when the batch is sharded over ranks."""
    ends = torch.nonzero(masks == 0).flatten().cpu().numpy()
    starts = np.concatenate(([0], ends[:-1] + 1))
    lens = ends - starts + 1
    max_len = _dist.global_max(int(lens.max()), masks.device)
    ep_of = np.repeat(np.arange(len(ends)), lens)
    covered = int(ends[-1]) + 1
    idx = np.arange(masks.shape[0])
    idx[:covered] = ep_of * max_len + (np.arange(covered) - np.repeat(starts, lens))
    return _Episodes(ends, starts, lens, max_len, covered, ep_of, idx, np.asarray(v_metas)[ends])


class _VideoFrontEnd(nn.Module):
    """The host side that VideoStateNet and VideoForecastNet share: the feature table, the rows of its windows, the train-mode
    batch cut into episodes with their windows gathered, the test-mode input. No parameters, buffers or submodules of its own.
    A subclass states its window through `_extent`."""

    # the part of a train-mode context both nets hold: the same for every net that sees the same batch through the same table
    _SHARED_CONTEXT = ("indices", "gather_indices", "cnn_feat_ctx", "_ctx_key")

    def __init__(self):
        super().__init__()
        self.mode = "test"
        self.v_out = None
        self.t = 0
        for k in self._SHARED_CONTEXT:
            setattr(self, k, None)
        self._cnn_table = None          # optional (device table, take offsets) installed by the env
        self._take_offset_host = self._take_len = None

    def set_mode(self, mode):
        self.mode = mode

    def forward_v_net(self, x):
        return _run_video_net(self.v_net, x)

    def _to_params(self, x):
        p = next(self.parameters())
        return x.to(device=p.device, dtype=p.dtype)

    def attach_feature_table(self, table, take_offset):
        """Device-resident concatenation of all takes' features (+ row offsets) for gather-built contexts."""
        host = np.asarray(take_offset, dtype=np.int64)
        if self._cnn_table is not None and self._cnn_table[0] is table and np.array_equal(self._take_offset_host, host):
            return                     # (same table as last time: no upload -- a copy from pageable memory blocks the host until the stream drains)
        self._cnn_table = (table, torch.as_tensor(host, dtype=torch.long, device=table.device))
        self._take_offset_host = host.copy()
        self._take_len = _take_lengths(take_offset, table.shape[0])

    def _table_on(self, device):
        return self._cnn_table[0] if self._cnn_table is not None and self._cnn_table[0].device == device else None

    def _same_table(self, other):
        return (self._cnn_table is not None and other._cnn_table is not None
                and self._cnn_table[0].data_ptr() == other._cnn_table[0].data_ptr()
                and np.array_equal(self._take_offset_host, other._take_offset_host))

    def _extent(self, length):
        """(before, after): a window of `length` frames from `start` covers the table rows [start - before, start + after)."""
        raise NotImplementedError

    def check_windows(self, expert_ind, start_ind, length):
        """Every window must lie inside its own take: the table is the concatenation of all takes, so a window that leaves
        its take would silently read a neighbour's frames (the reference's numpy slice comes up short and raises on
        assignment, models/video_state_net.py:52-55)."""
        _check_windows(self._take_len, expert_ind, start_ind, *self._extent(length))

    def window_features(self, expert_ind, start_ind, length):
        """Gather the windows of the given takes -> (before + after, B, D) on device."""
        table, off = self._cnn_table
        before, after = self._extent(length)
        base = off[expert_ind.long()] + start_ind.long() - before
        rows = base.unsqueeze(0) + torch.arange(before + after, device=table.device).unsqueeze(1)
        return table[rows]

    def _train_windows(self, ep, cnn_feat, device, dtype, length, rows=None):
        """`cnn_feat_ctx` and `_ctx_key` of the episodes `ep`: their windows of `length` as one (before + after, n_ep, D) block,
        gathered from the feature table when it lives on `device`, else cut from the takes' arrays `cnn_feat` on the host;
        with `rows`, on top of a zero block of that many rows. -> `meta` with the rows of the padding episodes."""
        before, after = self._extent(length)
        meta = ep.meta
        if self._table_on(device) is not None:
            # episode count rounded up to a bucket (gemm_tuning.py): the extra windows repeat episode 0, nothing
            # gathers from them, so their gradient contribution is exactly zero
            pad = _tuning.pad_to(len(meta), _tuning.EPISODE_BUCKET) if _tuning.enabled() and len(meta) >= 4 * _tuning.EPISODE_BUCKET else 0
            if pad:
                meta = np.concatenate((meta, np.repeat(meta[:1], pad, axis=0)), 0)
            self.check_windows(meta[:, 0], meta[:, 1], length)
            ctx = self.window_features(torch.as_tensor(meta[:, 0], device=device), torch.as_tensor(meta[:, 1], device=device), length).to(dtype)
            if rows is not None:
                win, ctx = ctx, ctx.new_zeros(rows, meta.shape[0], self.cnn_feat_dim)
                ctx[:before + after] = win
        else:
            ctx = np.zeros((before + after if rows is None else rows, len(meta), self.cnn_feat_dim))
            for e, (ei, si) in enumerate(meta):
                ctx[:before + after, e, :] = cnn_feat[int(ei)][int(si) - before: int(si) + after]
            ctx = torch.as_tensor(ctx, dtype=dtype, device=device)
        self.cnn_feat_ctx = ctx
        self._ctx_key = (int(ep.max_len), meta.shape[0], hash(meta.tobytes()))       # which windows cnn_feat_ctx holds
        return meta


def _same_windows(n, n0):
    """Train-mode net `n` holds the very windows `n0` holds: same batch, same padding, same block."""
    return (n.mode == "train" and n.cnn_feat_ctx is not None and n._ctx_key == n0._ctx_key
            and n.cnn_feat_ctx.shape == n0.cnn_feat_ctx.shape and n.cnn_feat_ctx.dtype == n0.cnn_feat_ctx.dtype)


class VideoStateNet(_VideoFrontEnd):
    """Temporal net over precomputed CNN features, concatenated in front of the state.

    test mode: ``initialize(window)`` with window (T+2m, D) for ONE episode, or (T+2m, B, D) for a batch of
    episodes (the lockstep rollout), keeps ``v_out`` = net(window)[m:-m]; ``forward(state)`` prepends
    v_out[t] and advances t (single-episode form) -- the batched rollout indexes ``v_out`` itself.
    train mode: ``initialize((masks, cnn_feat, v_metas))`` segments the flat batch into episodes and builds
    the padded context (max_len+2m, n_ep, D) and flat gather indices; ``forward(states)`` runs the net over
    the context and gathers one row per sample.
    """

    def __init__(self, cnn_feat_dim, v_hdim=128, v_margin=10, v_net_type="lstm", v_net_param=None, causal=False):
        super().__init__()
        self.cnn_feat_dim, self.v_hdim, self.v_margin, self.v_net_type = cnn_feat_dim, v_hdim, v_margin, v_net_type
        self.v_net = _video_net(cnn_feat_dim, v_hdim, v_net_type, v_net_param, causal)
        self._gather_tm = None
        self._gather_unique = False
        self._ragged = None      # (order, steps) of the train-mode windows for the grouped HIP sweeps
        self._frames = None      # (table, first row of every window) when the input projection runs per frame of the table
        self._v_ctx = None

    def _extent(self, length):
        return self.v_margin, length + self.v_margin          # rows [start - m, start + length + m)

    def initialize(self, x):
        m = self.v_margin
        if self.mode == "test":
            x = self._to_params(x)
            single = x.dim() == 2
            out = self.forward_v_net(x.unsqueeze(1) if single else x)[m:-m]
            self.v_out = out.squeeze(1) if single else out
            self.t = 0
            return
        masks, cnn_feat, v_metas = x
        device, dtype = masks.device, masks.dtype
        self._frames = None
        ep = _segment_episodes(masks, v_metas)
        self.indices = idx = ep.indices
        max_len = ep.max_len
        meta = self._train_windows(ep, cnn_feat, device, dtype, max_len)
        # The windows are runs of consecutive rows of the feature table: window b starts at row base[b]. When the table is
        # (much) smaller than the windows laid end to end -- the takes' frames are visited by many episodes -- the LSTMs'
        # input projection is computed per frame of the table instead of per window row (lstm.LstmGroup, `frames`).
        table = self._table_on(device)
        n_rows = self.cnn_feat_ctx.shape[0] * self.cnn_feat_ctx.shape[1]
        if table is not None and table.dtype == dtype and table.is_contiguous() and 2 * table.shape[0] <= n_rows:
            base = self._take_offset_host[meta[:, 0].astype(np.int64)] + meta[:, 1].astype(np.int64) - m
            self._frames = (table, torch.as_tensor(base.astype(np.int32), device=device))
        self.gather_indices = torch.as_tensor(idx, dtype=torch.long, device=device)
        # the same rows addressed in the net's own (time, episode) order: forward() gathers straight from the LSTM output
        # instead of slicing off the margins, transposing and copying it first
        tm = ((idx % max_len) + m) * self.cnn_feat_ctx.shape[1] + idx // max_len
        self._gather_tm = torch.as_tensor(tm, dtype=torch.long, device=device)
        # the backward pass's scatter relies on distinct rows. Samples inside episodes have them by construction (episode e,
        # offset < len_e <= max_len -> a distinct (frame, episode) cell); only a batch with samples after its last episode
        # end (idx = the sample's own number there) needs the look
        self._gather_unique = ep.covered == masks.shape[0] or np.unique(tm).size == tm.size
        # Ragged sweeps (lstm.ragged_order): the forward direction's output at frame t depends on frames <= t only and only
        # frames [m, m + len_e) of an episode are ever gathered, so it stops after m + len_e steps (workgroups of sequences
        # sorted by length); the backward direction starts at the end of the padded window and runs it all, as in the
        # reference. Windows added to fill an episode bucket need no step at all.
        steps = np.zeros(self.cnn_feat_ctx.shape[1], np.int64)
        steps[:len(ep.lens)] = ep.lens + m
        lstm_ctx = self.cnn_feat_ctx.is_cuda and isinstance(self.v_net, RNN)         # (a TCN has no sweeps to cut short)
        self._ragged = _hip_lstm.ragged_order(steps, device, T=self.cnn_feat_ctx.shape[0]) if lstm_ctx else None

    @torch.no_grad()
    def online_contexts(self, x):
        """The contexts of the reference's ONLINE evaluation (ego_pose/ego_mimic_eval.py:143-145: the net is re-initialised at
        every tick on the frames seen so far) for one take's features x (T + 2m, D) -> (T, v_hdim): row t is what
        ``initialize(x[:t + 2m + 1]); v_out[t]`` gives, i.e. row t + m of the net over frames [0, t + 2m]. Test mode, no gradients;
        `v_out` and `t` stay as they are.

        bi-LSTM      left half: the forward direction at frame t + m sees frames <= t + m whatever the prefix -- rows [m, m + T)
                     of one sweep. Right half: rnn_b after m + 1 steps from zero over frames t + 2m .. t + m -- T windows of
                     m + 1 frames, one launch of `lstm.window_last` over one per-frame projection (float32 on the device), else
                     a gathered (m + 1, T, D) batch through the module's own reverse sweep.
        causal nets  (uni-directional LSTM, causal TCN): no look-ahead, online == offline.
        TCN          one-sided reach R = (kernel_size - 1) * (2**levels - 1) frames: while R <= m row t + m never reaches the
                     prefix's padded end, online == offline exactly. R > m: by the definition, one net pass per tick -- O(T^2)
                     frames, slow; no shipped config has it."""
        if self.mode != "test":
            raise RuntimeError("online_contexts is a test-mode (evaluation) call")
        m = self.v_margin
        x = self._to_params(x)
        if x.dim() != 2 or x.shape[0] < 2 * m + 1:
            raise ValueError("online_contexts takes one take's features (T + 2m, D) with T >= 1, got %s" % (tuple(x.shape),))
        T, net = x.shape[0] - 2 * m, self.v_net
        offline = lambda: self.forward_v_net(x.unsqueeze(1))[m:m + T, 0]
        if isinstance(net, _tcn.TemporalConvNet):
            reach = (net.kernel_size - 1) * (2 ** len(net.network) - 1)
            if net.causal or reach <= m:
                return offline()
            return torch.stack([self.forward_v_net(x[:t + 2 * m + 1].unsqueeze(1))[t + m, 0] for t in range(T)], 0)
        if not net.bi_dir:
            return offline()
        H = net.rnn_f.hidden_size
        out = x.new_empty(T, 2 * H)
        out[:, :H] = net._sweep(net.rnn_f, x.unsqueeze(1), False)[m:m + T, 0]
        if net.cell_type == "lstm" and _LSTM_IMPL != "torch" and _hip_lstm.window_available(x, net.rnn_b):
            base = torch.arange(m, m + T, dtype=torch.int32, device=x.device)
            _hip_lstm.window_last(net.rnn_b, x.contiguous(), base, m + 1, True, out[:, H:])
        else:
            rows = torch.arange(m + 1, device=x.device).unsqueeze(1) + torch.arange(m, m + T, device=x.device).unsqueeze(0)
            out[:, H:] = net._sweep(net.rnn_b, x[rows], True)[0]
        return out

    _TRAIN_CONTEXT = _VideoFrontEnd._SHARED_CONTEXT + ("_gather_tm", "_gather_unique", "_ragged", "_frames")

    def adopt_train_context(self, other, x):
        """``initialize(x)`` in train mode when ``other`` has just been initialised with the SAME ``x``: the episode
        segmentation, the gather indices, the gathered feature windows and the ragged order depend on ``x``, the margin and
        the feature table only (not on the net's weights), so the policy's and the value function's front ends
        (ego_pose/core/agent_ego.py:34-41 initialises one after the other) share them -- one device sync and one pass of
        index arithmetic over the batch instead of two. Falls back to ``initialize`` when the two nets are not alike."""
        alike = (isinstance(other, VideoStateNet) and self.mode == "train" and other.mode == "train" and other.cnn_feat_ctx is not None
                 and self.v_margin == other.v_margin and self.cnn_feat_dim == other.cnn_feat_dim and self.v_net_type == other.v_net_type
                 and self._same_table(other) and other.cnn_feat_ctx.dtype == x[0].dtype)
        if not alike:
            return self.initialize(x)
        for k in self._TRAIN_CONTEXT:
            setattr(self, k, getattr(other, k))

    def forward(self, x, lazy_width=0):
        """`lazy_width` > 0 (train mode; the width of the consumer's first layer, passed per call by an agent whose heads can
        read the parts themselves): the result may be a gemm.GatheredInput -- [context rows | x] not yet formed -- instead of
        a tensor. The tensors this returns in train mode carry `_egp_ctx_cols` = v_hdim when x needs no gradient: their
        trailing columns are raw states, so a consumer may skip that part of the input gradient."""
        if self.mode == "test":
            out = torch.cat((self.v_out[[self.t], :], x), dim=1)
            self.t += 1
            return out
        def tagged(out):
            if not x.requires_grad:
                out._egp_ctx_cols = self.v_hdim
            return out
        ctx2d = self.context_rows()
        if self._gather_unique and _gemm.gather_concat_available(ctx2d, self._gather_tm, x):
            if lazy_width and _gemm.fused_gather_available(self.v_hdim, lazy_width, x.shape[1]):
                return _gemm.GatheredInput(ctx2d, self._gather_tm, x)            # the consumer's first layer gathers (gemm.GatherMlpHead)
            return tagged(_gemm.GatherConcat.apply(ctx2d, self._gather_tm, x))  # gather + concatenation in one pass
        return tagged(torch.cat((ctx2d.index_select(0, self._gather_tm), x), dim=1))

    def context_rows(self):
        """Train mode: the temporal net over the batch's windows as rows in the net's own (time, episode) order,
        (T * n_ep, v_hdim); `_gather_tm` holds every sample's row. They depend on the CNN features only, not on the states."""
        ctx = None
        if self._v_ctx is not None:          # computed together with another net's (grouped_video_context)
            (ctx, with_grad), self._v_ctx = self._v_ctx, None
            if with_grad != torch.is_grad_enabled():
                ctx = None                   # left over from a pass in the other autograd mode: never reuse it
        if ctx is None and isinstance(self.v_net, RNN):
            self.v_net.ragged = self._ragged
            try:
                ctx = self.forward_v_net(self.cnn_feat_ctx)
            finally:
                self.v_net.ragged = None
        elif ctx is None:
            ctx = self.forward_v_net(self.cnn_feat_ctx)
        return ctx.reshape(-1, self.v_hdim)


class Bf16Shadow:
    """bfloat16 compute copy of a convolutional encoder whose float32 parameters stay the MASTER weights (state_dict,
    optimizer). `torch.autocast` is not the way to bf16 on this stack: it re-casts weights and activations around every
    op (127 ms per 256-frame ResNet-18 step against 37 ms in float32); a module that simply IS bf16 runs MIOpen's
    implicit-GEMM MFMA convolutions end to end (21 ms). Normalisation layers are shared with the master (float32 affine
    parameters and running statistics, mixed-dtype batch norm), convolution / linear weights are bf16 copies:
    `pull()` after an optimizer step or a checkpoint load, `push_grads()` between backward and the optimizer step."""

    def __init__(self, master):
        import copy
        self.master = master
        self.shadow = copy.deepcopy(master)
        for name, m in list(master.named_modules()):
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                parent = self.shadow
                *path, leaf = name.split(".")
                for part in path:
                    parent = getattr(parent, part)
                setattr(parent, leaf, m)
        mp = dict(master.named_parameters())
        self.pairs = []
        for n, p in self.shadow.named_parameters():
            if p is not mp[n]:
                p.data = p.data.to(torch.bfloat16)
                self.pairs.append((mp[n], p))

    @torch.no_grad()
    def pull(self):
        torch._foreach_copy_([s for _, s in self.pairs], [m for m, _ in self.pairs])

    @torch.no_grad()
    def push_grads(self):
        dst, src = [], []
        for m, s in self.pairs:
            if s.grad is None:
                continue
            if m.grad is None:
                m.grad = torch.empty_like(m)
            dst.append(m.grad)
            src.append(s.grad)
        if dst:
            torch._foreach_copy_(dst, src)
        for _, s in self.pairs:
            s.grad = None

    def __call__(self, x):
        return self.shadow(x.to(torch.bfloat16)).float()


class VideoRegNet(nn.Module):          # (ResNet is defined further down; resolved at construction time)
    """State regressor of models/video_reg_net.py:10-59: [ResNet-18 per frame ->] temporal net -> MLP (relu) -> Linear.
    `no_cnn=True` (what the evaluation drivers load, ego_pose/ego_mimic_eval.py:71-80) takes precomputed features
    x: (T, B, cnn_fdim); with the encoder x: (T, B, 3, H, W). Output (T*B, out_dim)."""

    def __init__(self, out_dim, v_hdim, cnn_fdim, no_cnn=True, frame_shape=(3, 224, 224), mlp_dim=(300, 200),
                 cnn_type="resnet", v_net_type="lstm", v_net_param=None, causal=False):
        super().__init__()
        if not no_cnn and cnn_type != "resnet":
            raise NotImplementedError("only the 'resnet' image encoder is implemented (mobile net is out of scope)")
        self.out_dim, self.cnn_fdim, self.v_hdim, self.no_cnn = out_dim, cnn_fdim, v_hdim, no_cnn
        self.frame_shape = tuple(frame_shape)
        self.cnn = None if no_cnn else ResNet(cnn_fdim)
        self.v_net_type = v_net_type
        self.v_net = _video_net(cnn_fdim, v_hdim, v_net_type, v_net_param, causal)
        self.mlp = MLP(v_hdim, mlp_dim, "relu")
        self.linear = nn.Linear(self.mlp.out_dim, out_dim)

    def forward_v_net(self, x):
        return _run_video_net(self.v_net, x)

    def channels_last(self):
        """Keep the encoder's weights and activations NHWC (MIOpen's fp32 kernels run the ResNet-18 step 22 % faster in
        that layout on the MI355X: 46.1 -> 37.7 ms per 256-frame clip; same arithmetic). Returns self."""
        if self.cnn is not None:
            self.cnn.to(memory_format=torch.channels_last)
            self._nhwc = True
        return self

    def bf16_encoder(self, on=True):
        """Run the image encoder in bfloat16 on the matrix cores with its float32 parameters as master weights
        (BASELINE config 4; `Bf16Shadow`). Training loops call `encoder_grads_ready()` after backward and
        `encoder_stepped()` after the optimizer step (or a checkpoint load). Returns self."""
        self.__dict__["_enc16"] = Bf16Shadow(self.cnn) if (on and self.cnn is not None) else None
        return self

    def encoder_grads_ready(self):
        if self.__dict__.get("_enc16") is not None:
            self._enc16.push_grads()

    def encoder_stepped(self):
        if self.__dict__.get("_enc16") is not None:
            self._enc16.pull()

    def _encode(self, frames):
        # The bf16 copy serves OPTIMISATION steps only (train mode with autograd on). Everything whose output is kept --
        # the features gen_cnn_feature stores for the RL nets, test-mode predictions, eval metrics -- goes through the
        # float32 master encoder: ~8 mantissa bits would change stored features with no opt-in.
        enc = self.__dict__.get("_enc16")
        if enc is not None and self.training and torch.is_grad_enabled():
            enc.shadow.train(True)
            return enc(frames)
        return self.cnn(frames)

    def _frames(self, x):
        x = x.reshape((-1,) + self.frame_shape)
        return x.contiguous(memory_format=torch.channels_last) if getattr(self, "_nhwc", False) else x

    def forward(self, x):
        if self.cnn is not None:        # x: (T, B, 3, H, W) optical-flow frames -> per-frame features
            x = self._encode(self._frames(x)).view(-1, x.size(1), self.cnn_fdim)
        x = self.forward_v_net(x).reshape(-1, self.v_hdim)
        return self.linear(self.mlp(x))

    def get_cnn_feature(self, x):
        return self._encode(self._frames(x))


class VideoForecastNet(_VideoFrontEnd):
    """Policy/value front end of ego_forecast (models/video_forecast_net.py:7-111): the video net sees only the
    `v_margin` frames BEFORE the episode (causal LSTM or causal TCN, last output kept for the whole episode), the state goes through
    its own LSTM (`s_net_type='lstm'`, stepped one env-step at a time while sampling) or through unchanged ('id').

    test mode   ``initialize(window)``: window (>= v_margin, D) of ONE episode, or (v_margin, B, D) for a batch of
                episodes (the lockstep rollout); ``forward(state)`` -> cat(v_out, s_net(state)). The batched rollout
                steps the state LSTM itself through ``s_step``.
    train mode  ``initialize((masks, cnn_feat, v_metas))`` segments the flat batch into episodes;
                ``forward(states)`` scatters the states into a padded (max_len, n_ep, state_dim) block, runs both
                nets and gathers one row per sample.
    """

    def __init__(self, cnn_feat_dim, state_dim, v_hdim=128, v_margin=10, v_net_type="lstm", v_net_param=None,
                 s_hdim=None, s_net_type="id", dynamic_v=False):
        super().__init__()
        if s_net_type not in ("id", "lstm"):
            raise ValueError("s_net_type must be 'id' or 'lstm'")
        s_hdim = state_dim if s_hdim is None else s_hdim
        self.cnn_feat_dim, self.state_dim, self.v_hdim, self.v_margin = cnn_feat_dim, state_dim, v_hdim, v_margin
        self.v_net_type, self.s_net_type, self.s_hdim, self.dynamic_v = v_net_type, s_net_type, s_hdim, dynamic_v
        self.out_dim = v_hdim + s_hdim
        self.v_net = _video_net(cnn_feat_dim, v_hdim, v_net_type, v_net_param, True)
        if s_net_type == "lstm":
            self.s_net = RNN(state_dim, s_hdim, s_net_type, bi_dir=False)
        self.num_episode = self.max_episode_len = None
        self._grp = None
        self.set_mode("test")

    def set_mode(self, mode):
        self.mode = mode
        if self.s_net_type == "lstm":
            self.s_net.set_mode("batch" if mode == "train" else "step")

    def _extent(self, length):
        return self.v_margin, length                          # rows [start - v_margin, start + length)

    def check_windows(self, expert_ind, start_ind, length=0):        # (the plain context window needs no `length`)
        super().check_windows(expert_ind, start_ind, length)

    def window_features(self, expert_ind, start_ind, length=0):
        return super().window_features(expert_ind, start_ind, length)

    def context(self, window):
        """(v_margin, B, D) -> the per-episode video context (B, v_hdim): last output of the causal net."""
        return self.forward_v_net(window[:self.v_margin])[-1]

    def s_step(self, state, hc):
        """One step of the state net for a batch of envs: state (B, state_dim), hc = (h, c) or None -> (out, (h, c))."""
        if self.s_net_type != "lstm":
            return state, hc
        h, c = self.s_net.rnn_f(state, hc)
        return h, (h, c)

    def initialize(self, x):
        if self.mode == "test":
            x = self._to_params(x)
            self.v_out = self.context(x.unsqueeze(1) if x.dim() == 2 else x)
            if self.s_net_type == "lstm":
                self.s_net.initialize(self.v_out.shape[0])
            self.t = 0
            return
        masks, cnn_feat, v_metas = x
        ep = _segment_episodes(masks, v_metas)
        self.indices, self.max_episode_len = ep.indices, ep.max_len
        T_ctx = self.v_margin + ep.max_len if self.dynamic_v else self.v_margin
        # (the episode bucket's extra columns count as episodes of the padded blocks; nothing gathers from them)
        self.num_episode = self._train_windows(ep, cnn_feat, masks.device, masks.dtype, 0, rows=T_ctx).shape[0]
        self.gather_indices = torch.as_tensor(ep.indices, dtype=torch.long, device=masks.device)
        self._grp = None

    def state_sequences(self, x):
        """Flat batch of states -> (max_episode_len, num_episode, state_dim), zero where an episode is shorter."""
        s_ctx = x.new_zeros(self.num_episode * self.max_episode_len, self.state_dim)
        s_ctx = s_ctx.index_copy(0, self.gather_indices, x)
        return s_ctx.view(self.num_episode, self.max_episode_len, self.state_dim).transpose(0, 1).contiguous()

    def forward(self, x):
        if self.mode == "test":
            if self.s_net_type == "lstm":
                x = self.s_net(x)
            self.t += 1
            return torch.cat((self.v_out, x), dim=1)
        v_seq = s_seq = None
        if self._grp is not None:            # both sweeps came out of grouped launches (grouped_forecast_context)
            (v_seq, s_seq, x_ref, with_grad), self._grp = self._grp, None
            if x_ref is not x or with_grad != torch.is_grad_enabled():
                v_seq = s_seq = None         # prepared for another batch / autograd mode: never reuse
        if v_seq is None:
            v_seq = self.forward_v_net(self.cnn_feat_ctx)
        v_ctx = v_seq[self.v_margin:] if self.dynamic_v else v_seq[[-1]].expand(self.max_episode_len, -1, -1)
        v_out = v_ctx.transpose(0, 1).reshape(-1, self.v_hdim).index_select(0, self.gather_indices)
        if self.s_net_type == "lstm":
            if s_seq is None:
                s_seq = self.s_net(self.state_sequences(x))
            s_out = s_seq.transpose(0, 1).reshape(-1, self.s_hdim).index_select(0, self.gather_indices)
        else:
            s_out = x
        return torch.cat((v_out, s_out), dim=1)


def grouped_video_context(nets):
    """Train-mode video contexts of several VideoStateNets (the critic's and the actor's) in ONE grouped recurrent
    launch each way (lstm.LstmGroup): their bi-LSTMs read the same windows with different weights, and a single sweep
    leaves most of the chip idle. Each net's next forward() consumes its context. Returns False (nothing done) when the
    nets do not qualify (a TCN video net among them); the nets then compute their contexts one by one as usual."""
    if _LSTM_IMPL == "torch" or len(nets) < 1:
        return False
    n0 = nets[0]
    for n in nets:
        if not (isinstance(n, VideoStateNet) and _same_windows(n, n0) and getattr(n.v_net, "cell_type", None) == "lstm"
                and n.v_net.bi_dir == n0.v_net.bi_dir):
            return False
    cells, revs = [], []
    for n in nets:
        cells.append(n.v_net.rnn_f); revs.append(False)
        if n.v_net.bi_dir:
            cells.append(n.v_net.rnn_b); revs.append(True)
    x = n0.cnn_feat_ctx                      # same episodes, same windows for every net (initialize() of the same batch)
    if not _hip_lstm.group_available(x, cells):
        return False
    hs = _hip_lstm.lstm_group(x, cells, revs, pairs=n0.v_net.bi_dir, ragged=n0._ragged, frames=n0._frames)     # bi-directional: (T, B, 2H) per net, no concatenation
    for i, n in enumerate(nets):
        n._v_ctx = (hs[i], torch.is_grad_enabled())
    return True


def grouped_forecast_context(nets, x):
    """ego_forecast's counterpart of grouped_video_context: the causal video LSTMs of all nets in one grouped launch each
    way, and their state LSTMs over the scattered states `x` in another. Each net's next forward(x) consumes its pair.
    False (nothing done) when a net's video side is a TCN: every net then runs its own two nets."""
    if _LSTM_IMPL == "torch" or len(nets) < 2 or x is None:
        return False
    n0 = nets[0]
    for n in nets:
        if not (isinstance(n, VideoForecastNet) and _same_windows(n, n0) and n.s_net_type == "lstm"
                and n.dynamic_v == n0.dynamic_v and n.state_dim == n0.state_dim
                and isinstance(n.v_net, RNN) and not n.v_net.bi_dir and not n.s_net.bi_dir and n.v_net.cell_type == "lstm" and n.s_net.cell_type == "lstm"):
            return False
    v_cells, s_cells = [n.v_net.rnn_f for n in nets], [n.s_net.rnn_f for n in nets]
    s_in = n0.state_sequences(x)
    if not (_hip_lstm.group_available(n0.cnn_feat_ctx, v_cells) and _hip_lstm.group_available(s_in, s_cells)):
        return False
    fwd = [False] * len(nets)
    hv = _hip_lstm.lstm_group(n0.cnn_feat_ctx, v_cells, fwd)
    hs = _hip_lstm.lstm_group(s_in, s_cells, fwd)
    for n, a, b in zip(nets, hv, hs):
        n._grp = (a, b, x, torch.is_grad_enabled())
    return True


# ---------------------------------------------------------------------- image encoder of the state regressor
class _BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = torch.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return torch.relu(out + idt)


class ResNet18(nn.Module):
    """The published ResNet-18 (He et al. 2016; basic blocks [2, 2, 2, 2], 64-128-256-512 channels) with the module and
    parameter names of torchvision's `resnet18`, so a torchvision state dict loads unchanged; `fc` -> out_dim as
    models/resnet.py:12-17 does. torchvision is not in this image, so no pretrained weights are fetched here."""

    def __init__(self, out_dim):
        super().__init__()
        self.out_dim = out_dim
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        chans, layers, cin = (64, 128, 256, 512), [], 64
        for i, c in enumerate(chans):
            layers.append(nn.Sequential(_BasicBlock(cin, c, 1 if i == 0 else 2), _BasicBlock(c, c, 1)))
            cin = c
        self.layer1, self.layer2, self.layer3, self.layer4 = layers
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512, out_dim)

    def forward(self, x):
        x = self.maxpool(torch.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


class ResNet(nn.Module):
    """models/resnet.py:6-18: `self.resnet` = ResNet-18 whose fc maps to `out_dim`."""

    def __init__(self, out_dim, fix_params=False):
        super().__init__()
        self.out_dim = out_dim
        self.resnet = ResNet18(out_dim)
        if fix_params:
            for name, p in self.resnet.named_parameters():
                p.requires_grad = name.startswith("fc.")

    def forward(self, x):
        return self.resnet(x)
