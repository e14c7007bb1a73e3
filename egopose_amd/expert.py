"""Expert table handling: building the per-frame features the reward reads and keeping them in HBM.

The reference precomputes ``datasets/features/expert_<id>.p`` offline with
/root/reference/ego_pose/data_process/gen_expert.py:28-83 (MuJoCo FK + utils/math.py helpers) and
HumanoidEnv.load_experts unpickles it (ego_pose/envs/humanoid_v1.py:47-54). Here the same per-take dict is
either unpickled unchanged, or derived from a qpos sequence with the K7 feature kernel (GPU) + the physics
backend's forward kinematics; ``ExpertSet`` concatenates the takes, uploads the packed reward rows
(egp_upload_experts) and keeps the CNN features as one device table for gather-built LSTM windows.
"""
from __future__ import annotations

import numpy as np
import torch

HOT_KEYS = ("qpos", "qvel", "rlinv_local", "rangv", "rq_rmh", "ee_pos", "bquat", "bangvel")


def body_positions(physics, qpos_seq):
    """World body positions (L, nbody, 3) of a qpos sequence via the physics backend's FK (env 0)."""
    sk = physics.skel
    out = np.empty((qpos_seq.shape[0], len(sk.body_names), 3))
    zero_v = np.zeros(sk.nv)
    for i, q in enumerate(qpos_seq):
        physics.reset(0, q, zero_v)
        out[i] = physics.drain(0)[4]
    return out


def build_expert_take(ctx, physics, qpos_seq, lb=0, ub=None):
    """gen_expert.get_expert: features of one take from its qpos sequence (float64, reference formats)."""
    sk = ctx.skel
    qpos = np.array(qpos_seq, dtype=np.float64)
    addr = sk.body_qposaddr()
    for hand in ("LeftHand", "RightHand"):                     # "remove noisy hand data" (gen_expert.py:37-39)
        qpos[:, slice(*addr[hand])] = 0.0
    L = qpos.shape[0]
    xpos = body_positions(physics, qpos)
    ee_w = xpos[:, sk.ee_body, :].reshape(L, 15)
    dev = torch.device("cuda", ctx.device)
    cur = torch.as_tensor(qpos, device=dev)
    prev = torch.cat([cur[:1], cur[:-1]], 0).contiguous()
    f = ctx.pose_features(cur, prev, torch.as_tensor(ee_w, device=dev), expert_convention=True)
    f = {k: v.cpu().numpy() for k, v in f.items()}
    for k in ("qvel", "rlinv_local", "rangv", "bangvel"):      # frame 0 repeats frame 1 (gen_expert.py:66-69,75)
        f[k][0] = f[k][1]
    take = dict(f)
    take["rlinv"] = f["qvel"][:, :3].copy()
    take["qpos"] = qpos
    take["ee_wpos"] = ee_w
    take["head_pos"] = xpos[:, sk.body_names.index("Head"), :].copy()
    ub = L if ub is None else ub
    for k in list(take):
        take[k] = np.ascontiguousarray(take[k][lb:ub])
    take["len"] = take["qpos"].shape[0]
    take["height_lb"] = float(take["qpos"][:, 2].min())
    take["head_height_lb"] = float(take["head_pos"][:, 2].min())
    return take


OBS_MODES = ("reference", "fd")


def expert_obs_rows(expert_arr, ctx=None, mode="reference", obs_dim=None):
    """-> [per take: (len, S) float64] the expert's observation rows (what ego_pose/core/agent_vgail.py:83 reads as
    `expert_arr[i]['obs']`).

    mode "reference": each take's `obs` array as the pickle has it when EVERY take has one; otherwise derived as
        data_process/gen_expert.py:40-43 does -- `env.get_obs()` after setting `qpos` only, i.e. K3 on (qpos, zeros): the
        velocity columns of every row are zero (the reference's own quirk, kept as the default).
    mode "fd": always derived, with the take's finite-difference `qvel` -- rows comparable to the learner's.
    `ctx` (hip.EgpContext, the agent's own observation options) serves the derivation; `obs_dim` (default ctx.obs_dim): the
    width the rows must have."""
    if mode not in OBS_MODES:
        raise ValueError("expert_obs must be one of %s, got %r" % (OBS_MODES, mode))
    want = obs_dim if obs_dim is not None else (ctx.obs_dim if ctx is not None else None)
    if mode == "reference" and all("obs" in e for e in expert_arr):
        rows = [np.asarray(e["obs"], dtype=np.float64) for e in expert_arr]
    else:
        if ctx is None:
            raise ValueError("expert observation rows (mode %r) are derived on the device: a kernel context is needed" % mode)
        if getattr(ctx, "obs_phase", False):
            raise NotImplementedError("expert observation rows with obs_phase: the phase column depends on the episode, not on the take's frame")
        dev = torch.device("cuda", ctx.device)
        rows = []
        for e in expert_arr:
            qpos = torch.as_tensor(np.ascontiguousarray(e["qpos"], dtype=np.float64), device=dev)
            if mode == "fd":
                qvel = torch.as_tensor(np.ascontiguousarray(e["qvel"], dtype=np.float64), device=dev)
            else:
                qvel = torch.zeros(qpos.shape[0], ctx.nv, dtype=torch.float64, device=dev)
            rows.append(ctx.obs(qpos, qvel).cpu().numpy())
    for i, r in enumerate(rows):
        if r.ndim != 2 or (want is not None and r.shape[1] != want):
            raise ValueError("expert take %d has observation rows of width %s, the env's obs_dim is %s" % (i, r.shape[-1], want))
    return rows


class ExpertSet:
    """All training takes, concatenated; host copies feed resets, device copies feed K2 and the LSTM."""

    def obs_table(self, ctx, device, dtype, mode="reference", obs_dim=None):
        """-> (table [sum of the takes' lengths][S] on `device`, take_offset): the expert's observation rows of every take
        (`expert_obs_rows`), concatenated; cached per (device, dtype, mode)."""
        if self.expert_arr is None:
            raise ValueError("a features-only set has no expert rows")
        cache = self.__dict__.setdefault("_obs_table", {})
        key = (str(device), dtype, mode)
        if key not in cache:
            rows = expert_obs_rows(self.expert_arr, ctx, mode, obs_dim)
            for r, n in zip(rows, self.lens):
                if r.shape[0] != n:
                    raise ValueError("a take's observation rows (%d) do not match its length (%d)" % (r.shape[0], n))
            cache[key] = torch.as_tensor(np.ascontiguousarray(np.concatenate(rows, 0)), dtype=dtype, device=device)
        return cache[key], self.take_offset

    def __init__(self, expert_arr, cnn_feat):
        if len(expert_arr) != len(cnn_feat) or not expert_arr:
            raise ValueError("need one cnn feature array per expert take")
        self.expert_arr = expert_arr
        self.cnn_feat = cnn_feat
        self.lens = np.array([int(e["len"]) if "len" in e else int(e["qpos"].shape[0]) for e in expert_arr], np.int64)
        self.take_offset = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.qpos = np.ascontiguousarray(np.concatenate([e["qpos"] for e in expert_arr], 0), dtype=np.float64)
        self.qvel = np.ascontiguousarray(np.concatenate([e["qvel"] for e in expert_arr], 0), dtype=np.float64)
        self.head_height_lb = np.array([float(e["head_height_lb"]) for e in expert_arr])
        self.cnn_lens = np.array([c.shape[0] for c in cnn_feat], np.int64)
        self.cnn_offset = np.concatenate([[0], np.cumsum(self.cnn_lens)]).astype(np.int64)
        self._cnn_table = {}

    @classmethod
    def features_only(cls, cnn_feat):
        """The feature side alone (takes without MoCap): `cnn_table` / `cnn_offset` as above, no expert rows, no `head_height_lb`."""
        if not cnn_feat:
            raise ValueError("need at least one cnn feature array")
        self = cls.__new__(cls)
        self.expert_arr, self.cnn_feat = None, list(cnn_feat)
        self.lens = self.take_offset = self.qpos = self.qvel = self.head_height_lb = None
        self.cnn_lens = np.array([c.shape[0] for c in self.cnn_feat], np.int64)
        self.cnn_offset = np.concatenate([[0], np.cumsum(self.cnn_lens)]).astype(np.int64)
        self._cnn_table = {}
        return self

    def upload(self, ctx):
        if self.expert_arr is None:
            raise ValueError("a features-only set has no expert rows to upload")
        ctx.upload_experts(self.expert_arr)

    def cnn_table(self, device, dtype):
        key = (str(device), dtype)
        if key not in self._cnn_table:
            tab = np.ascontiguousarray(np.concatenate(self.cnn_feat, 0))
            self._cnn_table[key] = torch.as_tensor(tab, dtype=dtype, device=device)
        return self._cnn_table[key]
