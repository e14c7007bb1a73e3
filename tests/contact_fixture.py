"""Shared by the plausibility tests (test_contact_cpu.py on the CPU, test_contact_gpu.py on the GPU): pose rows of the joint-position
tests' generator placed at drawn heights over the ground, following rows of four kinds, contact points, and the yardstick -- float64
forward kinematics of oracle/dynamics.py (R and p) plus the definitions written out point by point in plain loops, so that it is
neither the product's host path nor the kernel."""
import numpy as np

import pose3d_fixture as PF

KINDS = ("moved in xy and yawed a little", "an unrelated row", "none", "itself")
LOW, HIGH = -0.03, 0.05              # the lowest contact point of a row sits at a drawn height in this range: penetrating, touching, floating
MARGIN = 1e-9                        # no point of any row lies this close to contact_height: rounding cannot flip a count


def random_contacts(skel, K, seed, bodies=None):
    """K points on drawn bodies (of `bodies`, default all) at drawn offsets within 0.1 m -> body int32 [K], offset [K][3], group int32 [K]."""
    rng = np.random.RandomState(seed)
    pool = np.arange(len(skel.body_names)) if bodies is None else np.asarray(bodies)
    return pool[rng.randint(len(pool), size=K)].astype(np.int32), rng.uniform(-0.1, 0.1, size=(K, 3)), rng.randint(2, size=K).astype(np.int32)


def leaves(skel):
    par = set(int(p) for p in skel.body_parent)
    return [b for b in range(len(skel.body_names)) if b not in par]


def points_of(skel, body, offset, qpos):
    """World contact points [N][K][3] of every row, from the oracle's body frames."""
    from oracle import dynamics as D
    out = np.zeros((len(qpos), len(body), 3))
    for i, q in enumerate(qpos):
        R, p = D.fk(skel, q)[:2]
        for k in range(len(body)):
            out[i, k] = p[body[k]] + R[body[k]] @ offset[k]
    return out


def figures_of_points(P, Pn, ground_z, contact_height):
    """One item's (pen, gap, n_contact, n_skate, skate, skate_max) from its points [K][3] and the following row's (None: none)."""
    z = [pt[2] - ground_z for pt in P]
    pen = max(max(0.0, -v) for v in z)
    gap = max(0.0, min(z))
    n_contact = sum(1 for v in z if v <= contact_height)
    slides = []
    if Pn is not None:
        for k in range(len(P)):
            if z[k] <= contact_height and Pn[k][2] - ground_z <= contact_height:
                slides.append(float(np.sqrt((Pn[k][0] - P[k][0]) ** 2 + (Pn[k][1] - P[k][1]) ** 2)))
    return np.array([pen, gap, n_contact, len(slides), sum(slides) / len(slides) if slides else 0.0, max(slides) if slides else 0.0])


def yardstick(points, row, nxt, ground_z=0.0, contact_height=0.02):
    """points [N][K][3] of all rows (points_of), row [n] (None: item i is row i), nxt [n] -> per_frame [n][6], points [n][K][3]."""
    n = len(nxt)
    row = np.arange(n) if row is None else row
    per_frame = np.stack([figures_of_points(points[row[i]], points[nxt[i]] if nxt[i] >= 0 else None, ground_z, contact_height) for i in range(n)])
    return per_frame, points[row]


def _yaw(q, a):
    return PF._qmul(np.array([np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)]), q)


def case(skel, body, offset, n, seed, gen=PF.poses, ground_z=0.0, contact_height=0.02):
    """n item rows (rows 0..n-1) and the following rows of the items of kind 0 behind them -> dict(qpos [N][nq], nxt [n], points
    [N][K][3] from the oracle, kind [n]). Item i is of kind i % 4 (KINDS). Redrawn (seed + 1000, ...) until every point of every row
    lies more than MARGIN from contact_height, so no item is ever left out of a comparison."""
    for attempt in range(20):
        rng = np.random.RandomState(seed + 1000 * attempt)
        q = gen(skel, n, rng)
        low = points_of(skel, body, offset, q)[:, :, 2].min(1)
        q[:, 2] += ground_z + rng.uniform(LOW, HIGH, size=n) - low
        extra, nxt = [], np.full(n, -1, np.int64)
        for i in range(n):
            kind = i % 4
            if kind == 0:
                f = q[i].copy()
                f[:2] += rng.normal(size=2) * 0.01
                f[3:7] = _yaw(f[3:7], rng.normal() * 0.03)
                nxt[i] = n + len(extra)
                extra.append(f)
            elif kind == 1:
                nxt[i] = (i + 2 + rng.randint(max(n - 3, 1))) % n          # never itself for n > 3, adjacent only by chance
            elif kind == 3:
                nxt[i] = i
        qpos = np.concatenate([q, np.array(extra).reshape(-1, skel.nq)])
        points = points_of(skel, body, offset, qpos)
        if np.abs(points[:, :, 2] - ground_z - contact_height).min() > MARGIN:
            kind = np.arange(n) % 4
            for a in (qpos, nxt, points, kind):
                a.setflags(write=False)
            return dict(qpos=qpos, nxt=nxt, points=points, kind=kind)
    raise AssertionError("no draw with every point more than %g m from contact_height" % MARGIN)


def two_takes(skel, seed=7):
    """pose3d_fixture.two_takes lowered so that the feet are near the ground: the root at 0.87 m +- a slow drift of a few centimetres."""
    res = PF.two_takes(skel, seed)
    rng = np.random.RandomState(seed + 1)
    for key in ("traj_pred", "traj_orig"):
        for take, tr in res[key].items():
            tr[:, 2] = 0.87 + np.cumsum(rng.normal(size=len(tr)) * 0.01)
    return res
