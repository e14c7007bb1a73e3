#!/usr/bin/env python3
"""Fixtures of the ego_forecast evaluation: tests/golden/forecast_eval.npz.

Imports the reference exactly as tools/gen_golden.py does (same stubs for the absent third-party modules, nothing copied)
and records, in float64:

    sync_*      ego_pose/utils/tools.py:18-32 sync_traj on a synthetic (T = 7) qpos / qvel trajectory and a yawed, translated
                ref_qpos.
    fm_*        ego_pose/eval_forecast.py:29-98 compute_metrics / compute_err_vs_h. That script parses argv and opens result
                files when imported, so the two functions are taken from the file itself at generation time: their FunctionDef
                nodes are extracted with `ast` and executed in a namespace that holds the reference's ego_pose.utils.metrics
                functions, `dt` and a `cfg` stub (nothing is retyped here). Inputs: 2 takes x 3 windows x (m + 20) frames of
                synthetic qpos with unit root quaternions, m = 4; outputs: the three numbers at horizons 10 and 20 and the
                err-vs-horizon vector.

Runs ONLY where the reference is present. Own seeds, arrays only (loads with allow_pickle=False).
"""
import ast
import contextlib
import io
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden as G          # noqa: E402  (stubs + workdir helpers)


def _setup():
    G.install_stubs()
    if G.REF not in sys.path:
        sys.path.insert(0, G.REF)
    G.enter_workdir()
    import utils  # noqa: F401  (reference utils)
    from egopose_amd.skeleton import load_skeleton
    return load_skeleton(os.path.join(G.REF, "assets/mujoco_models/humanoid_1205_v1.xml"))


def _yaw(a):
    return np.array([np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)])


def sync_traj_case(sk, out):
    from ego_pose.utils.tools import sync_traj
    from utils.transformation import quaternion_multiply
    rng = np.random.RandomState(5501)
    T = 7
    qpos = G.synth_qpos(rng, sk, T)
    qvel = rng.normal(size=(T, sk.nv))
    ref = qpos[0].copy()
    ref[:3] += np.array([0.7, -1.3, 0.05])
    ref[3:7] = quaternion_multiply(_yaw(0.9), ref[3:7])
    new_qpos, new_qvel = sync_traj(qpos, qvel, ref)
    out.update(sync_qpos=qpos, sync_qvel=qvel, sync_ref=ref, sync_out_qpos=new_qpos, sync_out_qvel=new_qvel)


def _functions_of(path, names, namespace):
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(d.name for d in defs) == sorted(names)
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), namespace)
    return [namespace[n] for n in names]


def forecast_metrics_case(sk, out):
    from ego_pose.utils import metrics as ref_metrics
    m, n_win, n_fr = 4, 3, 24
    ns = {k: getattr(ref_metrics, k) for k in dir(ref_metrics) if not k.startswith("_")}
    ns.update(np=np, dt=1 / 30.0, cfg=types.SimpleNamespace(fr_margin=m))
    compute_metrics, compute_err_vs_h = _functions_of(os.path.join(G.REF, "ego_pose", "eval_forecast.py"),
                                                      ["compute_metrics", "compute_err_vs_h"], ns)
    rng = np.random.RandomState(5502)
    takes = ["take_a", "take_b"]
    orig = {t: np.stack([G.synth_qpos(rng, sk, n_fr) for _ in range(n_win)]) for t in takes}
    pred = {}
    for t in takes:
        p = orig[t] + 0.05 * rng.normal(size=orig[t].shape)
        p[..., 3:7] /= np.linalg.norm(p[..., 3:7], axis=-1, keepdims=True)
        pred[t] = p
    results = {"traj_pred": pred, "traj_orig": orig}
    with contextlib.redirect_stdout(io.StringIO()):
        for h in (10, 20):
            out["fm_h%d" % h] = np.array(compute_metrics(results, "ego forecast", h, False))
        out["fm_err_vs_h"] = compute_err_vs_h(results, "ego forecast", 24, step=5)
    out.update(fm_margin=m, fm_err_horizon=24, fm_err_step=5, fm_pred=np.stack([pred[t] for t in takes]),
               fm_orig=np.stack([orig[t] for t in takes]))


if __name__ == "__main__":
    sk = _setup()
    out = {}
    sync_traj_case(sk, out)
    forecast_metrics_case(sk, out)
    path = os.path.join(G.OUT, "forecast_eval.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, "%.0f kB" % (os.path.getsize(path) / 1e3), {k: np.asarray(v).shape for k, v in out.items()})
