"""update_tail_fixture.py checked on the CPU: its float64 references against independent yardsticks (torch autograd over the update
monitor's form of the log-density plus the closed-form gradients; torch.optim.Adam + clip_grad_norm_), its cases (no row near the
clip boundary, all three regimes populated), and its bounds -- a float32 emulation of the kernels stays inside them, and every
wrong kernel listed below leaves them by at least 5 x at the small shapes. The margins are printed."""
import math

import numpy as np
import pytest
import torch

import update_tail_fixture as F

MARGIN = 5.0
LOSS_OUT = ("v_loss", "s_loss", "d_pred", "d_mean", "d_log_std")
SMALL_FULL = [c for c in F.WIDTH_CASES + F.ROW_CASES if c[1] <= 67]
SMALL_WINDOWS = [(n, A, form) for n, A in F.WINDOW_SHAPES if n <= 33 for form in F.WINDOW_FORMS]


def _yardstick(c, mean, fixed, n_val, n_exp, mask=None):
    """ppo_stats_torch's expression of the log-density (var = exp(2 log_std)) under float64 autograd, and the gradients in closed
    form: g_i = -adv_i ratio_i / n_exp unless the row is clipped, d_mean = g z / std, d_log_std = sum g (z^2 - 1)."""
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    rows, clip = c["rows"], c["clip"]
    pred, mu, ls = (t(a).requires_grad_(True) for a in (c["pred"], mean, c["log_std"]))
    act, adv = t(c["actions"] if rows is None else c["actions"][rows]), t(c["adv"] if rows is None else c["adv"][rows])
    logp = (-(act - mu).pow(2) / (2.0 * torch.exp(ls * 2.0)) - 0.5 * math.log(2.0 * math.pi) - ls).sum(1)
    fx = logp.detach() if fixed is None else t(fixed)
    ratio = torch.exp(logp - fx)
    keep = torch.ones(logp.shape[0], dtype=torch.bool) if mask is None else torch.from_numpy(np.asarray(mask, dtype=bool))
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv)[keep]
    s_loss = -surr.sum() / n_exp
    v_loss = ((pred - t(c["returns"])) ** 2).sum() / n_val
    (s_loss + v_loss).backward()
    r, a = ratio.detach().numpy(), adv.numpy()
    clipped = ((a > 0) & (r > 1.0 + clip)) | ((a < 0) & (r < 1.0 - clip))
    g = np.where(clipped | ~keep.numpy(), 0.0, -a * r / n_exp)
    std = np.exp(np.asarray(c["log_std"], dtype=np.float64))
    z = (act.numpy() - np.asarray(mean, dtype=np.float64)) / std
    zero = lambda x: torch.zeros_like(x)
    auto = {"v_loss": v_loss.item(), "s_loss": s_loss.item(), "d_pred": (pred.grad if pred.grad is not None else zero(pred)).numpy(),
            "d_mean": (mu.grad if mu.grad is not None else zero(mu)).numpy(), "d_log_std": (ls.grad if ls.grad is not None else zero(ls)).numpy()}
    closed = {"d_mean": g.reshape(-1, 1) * z / std, "d_log_std": (g.reshape(-1, 1) * (z * z - 1.0)).sum(0),
              "d_pred": 2.0 * (np.asarray(c["pred"], dtype=np.float64) - c["returns"]) / n_val}
    return auto, closed


@pytest.mark.parametrize("case", F.WIDTH_CASES + F.ROW_CASES + [F.EMPTY_POL_CASE], ids=str)
def test_loss_reference_against_autograd_and_closed_form(case):
    c = F.policy_case(*case)
    for mean, fixed, ref in ((c["mean0"], None, c["ref_write"]), (c["mean"], c["fixed"], c["ref_read"])):
        auto, closed = _yardstick(c, mean, fixed, c["n_val"], c["n_exp"])
        for want in (auto, closed):
            for k, w in want.items():
                np.testing.assert_allclose(ref[k], w, rtol=1e-11, atol=1e-14 * max(1.0, float(np.abs(w).max()) if np.size(w) else 1.0), err_msg=k)


@pytest.mark.parametrize("n,A,form", SMALL_WINDOWS + [(511, 5, "mixed")], ids=str)
def test_window_reference_against_autograd_and_closed_form(n, A, form):
    c, e, ref = F.window_case(n, A, form)
    auto, closed = _yardstick(c, c["mean"], c["fixed"], float(n), float((e != 0).sum()), mask=e != 0)
    for want in (auto, closed):
        for k, w in want.items():
            np.testing.assert_allclose(ref[k], w, rtol=1e-11, atol=1e-14 * max(1.0, float(np.abs(w).max())), err_msg=k)
    assert not ref["d_mean"][e == 0].any()


@pytest.mark.parametrize("case", F.FULL_CASES + [F.STRIDE_CASE] + [(n, n, A, False) for n, A in F.WINDOW_SHAPES], ids=str)
def test_policy_cases_leave_no_row_out_and_fill_the_three_regimes(case):
    c = F.policy_case(*case)
    n_pol, A = c["n_pol"], c["A"]
    assert c["near"] == 0 and not F.near_rows(c["ref_read"], A).any()          # the share of excluded rows is zero by construction
    assert c["redrawn"] <= 4 + n_pol // 250              # (measured on 20 000 rows: 0.085 % of the rows at A = 256, fewer below)
    assert not F.near_rows(c["ref_write"], A).any() and not c["ref_write"]["log_ratio"].any()
    if c["rows"] is not None and n_pol > 2:
        assert len(set(c["rows"].tolist())) == n_pol and (np.diff(c["rows"]) < 0).any()      # a subset, unsorted
    shares = F.regimes(c["ref_read"])
    print("n_pol %d A %d: below %.3f inside %.3f above %.3f, %d rows drawn again" % ((n_pol, A) + shares + (c["redrawn"],)))
    if n_pol >= 200:
        assert min(shares) >= 0.05


def _ties(ref, clip=F.CLIP):
    """rows whose ratio lies inside the clip range: surr1 == surr2 there, torch.min's tie"""
    return (ref["log_ratio"] > math.log(1.0 - clip)) & (ref["log_ratio"] < math.log(1.0 + clip))


def _loss_margins(c, ref, bounds, emu):
    return {k: F.worst(emu[k], ref[k], bounds[k]) for k in LOSS_OUT}


@pytest.mark.parametrize("case", SMALL_FULL, ids=str)
def test_loss_bounds_hold_the_emulation_and_tell_wrong_kernels_apart(case):
    c = F.policy_case(*case)
    n_pol, A = c["n_pol"], c["A"]
    P = F.rows_per_lane(n_pol)
    for name, mean, fixed, ref, write in (("write", c["mean0"], None, c["ref_write"], True), ("read", c["mean"], c["fixed"], c["ref_read"], False)):
        b = F.loss_bounds(ref, A, P, write)
        emu = F.loss_emulation(c, mean, fixed, c["n_val"], c["n_exp"])
        good = _loss_margins(c, ref, b, emu)
        good["logp"] = F.worst(emu["logp"], ref["logp"], b["logp"])
        print("%s pass, emulation / bound: %s" % (name, {k: round(v, 3) for k, v in good.items()}))
        assert max(good.values()) <= 1.0, good
        for mutant in ("drop", "tie"):
            if mutant == "tie" and not _ties(ref).any():
                print("%s pass, mutant tie: NOT exercised (every row of this pass is outside the clip range: nothing ties)" % name)
                continue
            bad = _loss_margins(c, ref, b, F.loss_emulation(c, mean, fixed, c["n_val"], c["n_exp"], mutant=mutant))
            print("%s pass, mutant %s / bound: %.3g" % (name, mutant, max(bad.values())))
            assert max(bad.values()) >= MARGIN, (mutant, bad)


@pytest.mark.parametrize("A", [1, 17, 256])
def test_clamp_ends_excluded_is_told_apart_where_every_row_sits_on_both_ends(A):
    """clip_eps = 0 in the write pass: ratio = lo = hi = 1 in every row, a tie of min at both ends of clamp's range. torch gives the
    whole gradient there (half through each branch, the clamp's sub-gradient 1); with the ends excluded it is half."""
    c = F.policy_case(101, 67, A, True, 0.0)
    ref = c["ref_write"]
    b = F.loss_bounds(ref, A, F.rows_per_lane(67), True)
    auto, closed = _yardstick(c, c["mean0"], None, c["n_val"], c["n_exp"])
    np.testing.assert_allclose(ref["d_mean"], auto["d_mean"], rtol=1e-12, atol=1e-16)
    np.testing.assert_allclose(ref["d_mean"], closed["d_mean"], rtol=1e-12, atol=1e-16)
    good = _loss_margins(c, ref, b, F.loss_emulation(c, c["mean0"], None, c["n_val"], c["n_exp"], clip=0.0))
    bad = _loss_margins(c, ref, b, F.loss_emulation(c, c["mean0"], None, c["n_val"], c["n_exp"], clip=0.0, mutant="ends"))
    print("emulation / bound %.3f, mutant ends / bound %.3g" % (max(good.values()), max(bad["d_mean"], bad["d_log_std"])))
    assert max(good.values()) <= 1.0, good
    assert bad["d_mean"] >= MARGIN and bad["d_log_std"] >= MARGIN, bad


@pytest.mark.parametrize("n,A,form", SMALL_WINDOWS, ids=str)
def test_window_bounds_hold_the_emulation_and_tell_wrong_kernels_apart(n, A, form):
    c, e, ref = F.window_case(n, A, form)
    n_exp = float((e != 0).sum())
    b = F.loss_bounds(ref, A, F.rows_per_lane(n, window=True), False)
    run = lambda mutant: _loss_margins(c, ref, b, F.loss_emulation(c, c["mean"], c["fixed"], float(n), n_exp, mask=e != 0, window=True, mutant=mutant))
    good = run(None)
    print("emulation / bound: %s" % {k: round(v, 3) for k, v in good.items()})
    assert max(good.values()) <= 1.0, good
    for mutant in ("drop", "tie"):
        if mutant == "tie" and not (_ties(ref) & (e != 0)).any():
            print("mutant tie: NOT exercised (no live row inside the clip range in this window: nothing ties)")
            continue
        bad = run(mutant)
        print("mutant %s / bound: %.3g" % (mutant, max(bad.values())))
        assert max(bad.values()) >= MARGIN, (mutant, bad)


# ------------------------------------------------------------------------------------------------ clip + Adam
def test_adam_reference_against_torch_adam_and_clip_grad_norm():
    """Three steps over layout L1 in float64 with weight decay on one segment: every segment a parameter of its own in its own
    param group of torch.optim.Adam(foreach=False), every clip group a clip_grad_norm_ call."""
    total, segs = F.L1_TOTAL, F.L1
    p, m, v = F.adam_state(total, "torch", False)
    params = [torch.nn.Parameter(torch.from_numpy(p[s["begin"]:s["end"]].copy())) for s in segs]
    opt = torch.optim.Adam([{"params": [q], "lr": s["lr"], "betas": (s["beta1"], s["beta2"]), "eps": s["eps"], "weight_decay": s["wd"]}
                            for q, s in zip(params, segs)], foreach=False)
    state = (p, m, v)
    for k, nm in enumerate(({1: 2.5, 3: 0.8}, {1: 0.8, 3: 2.5}, {1: 2.5, 3: 0.8})):
        g = F.adam_gradient(segs, total, ("torch", k), nm)
        ref = F.adam_reference(F.with_step(segs, k + 1), g, state[0], state[1], state[2], np.float64)
        for q, s in zip(params, segs):
            q.grad = torch.from_numpy(g[s["begin"]:s["end"]].copy())
        for grp in (1, 3):
            mine = [q for q, s in zip(params, segs) if s["clip_group"] == grp]
            norm = torch.nn.utils.clip_grad_norm_(mine, [s["max_norm"] for s in segs if s["clip_group"] == grp][0])
            assert abs(float(norm) - ref["norms"][grp]) <= 1e-13 * ref["norms"][grp]
            assert (ref["coef"][grp] < 1.0) == (nm[grp] > 1.0)
        opt.step()
        for q, s in zip(params, segs):
            sl = slice(s["begin"], s["end"])
            if s["end"] == s["begin"]:
                continue
            st = opt.state[q]
            for name, got in (("p", q.detach().numpy()), ("m", st["exp_avg"].numpy()), ("v", st["exp_avg_sq"].numpy())):
                want = ref[name][sl]
                np.testing.assert_allclose(want, got, rtol=1e-13, atol=1e-13 * float(np.abs(got).max()), err_msg="%s step %d" % (name, k + 1))
        out = ~F.covered(segs, total)
        assert np.array_equal(ref["p"][out], p[out]) and not ref["m"][out].any() and not ref["v"][out].any()      # the gaps are untouched
        assert np.isnan(ref["norms"][[0, 2, 4, 5, 6, 7, 8]]).all()
        state = (ref["p"], ref["m"], ref["v"])


def _adam_margins(ref, emu, mask):
    return {k: F.worst(emu[k][mask], ref[k][mask], ref["e_" + k][mask]) for k in ("p", "m", "v")}


@pytest.mark.parametrize("run", sorted(F.ADAM_RUNS))
def test_adam_bounds_hold_the_float32_emulation(run):
    p, m, v, steps = F.adam_run(F.L1, F.L1_TOTAL, run, np.float32, True)
    mask = F.covered(F.L1, F.L1_TOTAL)
    state = {"p": p, "m": m, "v": v}
    for k, (segs, g, ref) in enumerate(steps):
        state = F.adam_emulation_f32(segs, g, state["p"], state["m"], state["v"])
        good = _adam_margins(ref, state, mask)
        print("%s step %d, emulation / bound: %s" % (run, k + 1, {a: round(b, 3) for a, b in good.items()}))
        assert max(good.values()) <= 1.0, good
        assert all(np.array_equal(state[a][~mask], (p, m, v)[i].astype(np.float32)[~mask]) for i, a in enumerate("pmv"))


def test_adam_bounds_tell_wrong_kernels_apart():
    """t = 1 from zero moments, layout L1, float32. `1.f - (float)beta2` is the form k_adam had: every second moment 1.29e-5 too
    small against a bound of 16 u = 9.5e-7 of it."""
    p, m, v, steps = F.adam_run(F.L1, F.L1_TOTAL, "t1", np.float32, True)
    segs, g, ref = steps[0]
    mask = F.covered(F.L1, F.L1_TOTAL)
    for mutant, where in (("eps", "p"), ("wd", "m"), ("beta", "v")):
        bad = _adam_margins(ref, F.adam_emulation_f32(segs, g, p, m, v, mutant=mutant), mask)
        print("mutant %s / bound: %s" % (mutant, {a: float("%.3g" % b) for a, b in bad.items()}))
        assert bad[where] >= MARGIN, (mutant, bad)


@pytest.mark.parametrize("run", sorted(F.ADAM_RUNS))
def test_adam_reference_with_the_kernels_weights_holds_the_kernels_emulation(run):
    """The reference with weights="kernel" is what k_adam<float> computes today: the emulation with the same weights stays inside the
    same bounds, and the other two wrong kernels still leave them (the GPU file's float32 guard on p, m and v rests on this)."""
    p, m, v, steps = F.adam_run(F.L1, F.L1_TOTAL, run, np.float32, True, weights="kernel")
    mask = F.covered(F.L1, F.L1_TOTAL)
    state = {"p": p, "m": m, "v": v}
    for k, (segs, g, ref) in enumerate(steps):
        if k == 0 and run == "t1":
            for mutant, where in (("eps", "p"), ("wd", "m")):
                bad = _adam_margins(ref, F.adam_emulation_f32(segs, g, p, m, v, mutant=mutant), mask)
                print("kernel weights, mutant %s / bound: %s" % (mutant, {a: float("%.3g" % b) for a, b in bad.items()}))
                assert bad[where] >= MARGIN, (mutant, bad)
            torch_form = _adam_margins(ref, F.adam_emulation_f32(segs, g, p, m, v), mask)
            print("kernel weights, torch's weights / bound: %s" % {a: float("%.3g" % b) for a, b in torch_form.items()})
            assert torch_form["v"] >= MARGIN                      # the two forms are told apart in this direction too
        state = F.adam_emulation_f32(segs, g, state["p"], state["m"], state["v"], mutant="kernel")
        good = _adam_margins(ref, state, mask)
        print("%s step %d, kernel weights, emulation / bound: %s" % (run, k + 1, {a: round(b, 3) for a, b in good.items()}))
        assert max(good.values()) <= 1.0, good
