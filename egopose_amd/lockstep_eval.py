"""The lockstep pass of the evaluation drivers: k <= N takes or windows on the slots of `env.batched(N)`, advanced tick by tick.

`BatchedEvaluator` (evaluate.py, and `BatchedWildEvaluator` through it) and `ForecastEvaluator` (evaluate_forecast.py) run their
takes / windows through one `LockstepPass` per `run()`. The pass owns what does not depend on the policy: the batched env and its
device, the frozen observation filter (`running_state(x, update=False)` as the device state the fused launches read), the
`obs_phase` table, seating and re-seating slots, the `active` mask, the record buffers and their copy-out, and a tick's

    record qpos (/ qvel) -> launch(t, k) -> event -> [behind_event(t)] -> env-step of the active slots -> wait for the host physics

The driver passes `launch` (its fused policy launch, which reads `eng.qpos[:k]` / `eng.qvel[:k]` and writes `states[t, :k]` and
`actions[t, :k]`) and, where it has device work that must NOT hold the env-step back, `behind_event` (queued behind the event the
env-step waits on: the mimic driver's pinned value copy). The host decision after a tick -- fail-safe, re-seats, the `failed` log --
is the driver's.

`Timing` is the drivers' `timing` dict: wall seconds of a run split into the wait for the host physics (`phys_wait`) and the rest,
and the `passes` and `ticks` the pass counts; a driver adds its own counts (`takes`, `windows`, `fs_passes`, ...).
"""
from __future__ import annotations

import time

import numpy as np
import torch


class Timing(dict):
    def __init__(self, **counts):
        super().__init__(phys_wait=0.0, passes=0, ticks=0, **counts)
        self._t0 = time.time()

    def close(self):
        self["total"] = time.time() - self._t0
        self["rest"] = self["total"] - self["phys_wait"]


def check_frozen_filter(running_state, advice=""):
    """The fused launches apply the filter as (x - mean) / std, clipped: a driver's constructor refuses a `running_state` that does
    anything else."""
    if running_state is not None and not (running_state.demean and running_state.destd):
        raise NotImplementedError("running_state without demean / destd" + advice)


class LockstepPass:
    """`n_ticks`: the longest pass of the run (the records' first dimension). `timing`: the run's `Timing`. Records, float64 on the
    device: `traj` [T][N][nq], `qvel` [T][N][nv] (None unless `record_qvel`), `states` [T][N][obs_dim], `actions` [T][N][nu]."""

    def __init__(self, env, num_envs, device_index, n_threads, running_state, n_ticks, timing, record_qvel=True):
        self.N, self.timing = int(num_envs), timing
        self.sim = env.batched(self.N, device_index, n_threads, 1)
        self.ctx, self.eng = self.sim.ctx, self.sim.engine
        self.dev = dev = torch.device("cuda", self.ctx.device)
        self.zf_in, self.clip = None, 0.0
        if running_state is not None:
            self.zf_in, self.clip = running_state.to_device_state(dev), float(running_state.clip or 0.0)
        T, N, ctx = int(n_ticks), self.N, self.ctx
        z = lambda width: torch.zeros(T, N, width, dtype=torch.float64, device=dev)
        self.traj, self.qvel, self.actions, self.states = z(ctx.nq), z(ctx.nv) if record_qvel else None, z(ctx.nu), z(ctx.obs_dim)
        self.phase = torch.arange(T, dtype=torch.int32, device=dev).unsqueeze(1).expand(T, N).contiguous() if ctx.obs_phase else None
        self.k, self.active, self._seated = 0, None, False

    def seat(self, q0, v0):
        """Start a pass with slots 0 .. k-1 on the rows of q0 / v0 -> the `active` mask (the driver clears a slot that is done)."""
        k, N = len(q0), self.N
        ids = np.arange(k)
        if not self._seated and k < N:            # slots nothing ever lands on: a valid state all the same (they are never stepped)
            ids = np.arange(N)
            q0, v0 = np.concatenate((q0, np.repeat(q0[:1], N - k, 0))), np.concatenate((v0, np.repeat(v0[:1], N - k, 0)))
        self._seated = True
        self.eng.reset(ids, q0, v0)
        self.k, self.active = k, np.zeros(N, np.int32)
        self.active[:k] = 1
        return self.active

    def reseat(self, slots, qpos, qvel):
        """Mid-pass: put the slots `slots` on new states (a partial engine reset); the others keep theirs."""
        self.eng.reset(np.asarray(slots), qpos, qvel)

    def phase_t(self, t):
        return None if self.phase is None else self.phase[t, :self.k]

    def tick(self, t, launch, behind_event=None):
        """One tick (module docstring) -> what `behind_event(t)` returned."""
        eng, k, tm = self.eng, self.k, self.timing
        self.traj[t, :k].copy_(eng.qpos[:k])
        if self.qvel is not None:
            self.qvel[t, :k].copy_(eng.qvel[:k])
        launch(t, k)
        ev = torch.cuda.Event()
        ev.record()
        out = behind_event(t) if behind_event is not None else None
        eng.step_async(0, self.actions[t], self.active, ev)
        t0 = time.time()
        eng.wait(0)
        tm["phys_wait"] += time.time() - t0
        tm["ticks"] += 1
        return out

    def copy_out(self, n_ticks, *names):
        """End a pass of `n_ticks` ticks -> the records `names` of its k slots as host arrays [k][n_ticks][..]."""
        torch.cuda.synchronize(self.dev)
        self.timing["passes"] += 1
        return tuple(getattr(self, name)[:n_ticks, :self.k].transpose(0, 1).cpu().numpy() for name in names)
