"""egp_lstm_fwd_f32 with last_only (csrc/egp_lstm.hip: B windows of `steps` consecutive frames of one projection table, last hidden state
only) against a float64 nn.LSTMCell loop on the CPU over the gathered windows (models/rnn.py:45-61), against the grouped forward
sweep it shares its step with, its argument checks, and VideoStateNet.online_contexts on the device against its float64 definition
(ego_pose/ego_mimic_eval.py:143-145)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, F = 24, 96                       # input width, frames of the table
STEPS = (1, 2, 3, 4, 5, 11)         # the remainders of both unroll depths (4 for hidden 64, 2 for hidden 128), and m + 1 of the configs
ATOL = {64: 2e-5, 128: 3e-5}        # tests/test_lstm_gpu.py: the forward sweeps against the same kind of reference
CANARY = -7.0

_PROBLEMS = {}


def _problem(H):
    """Per hidden size, once: a cell, a table of frames, its projection in float32 in the kernels' unit-major layout."""
    if H not in _PROBLEMS:
        torch.manual_seed(100 + H)
        cell = torch.nn.LSTMCell(D, H).double()
        x = torch.randn(F, D, dtype=torch.float64)
        with torch.no_grad():
            gx = torch.addmm(cell.bias_ih + cell.bias_hh, x, cell.weight_ih.t())              # (F, 4H), torch order: column g*H + u
        n = torch.arange(4 * H)
        gx_um = gx[:, (n % 4) * H + n // 4].float().contiguous().cuda()                       # column 4*u + g
        _PROBLEMS[H] = dict(cell=cell, x=x, gx=gx_um, w_hh=cell.weight_hh.detach().float().contiguous().cuda())
    return _PROBLEMS[H]


def _reference(pr, base, steps, reverse):
    """float64 LSTMCell loop from zero state over the gathered windows -> (B, H)."""
    cell, x = pr["cell"], pr["x"]
    B = len(base)
    h = c = torch.zeros(B, cell.hidden_size, dtype=torch.float64)
    order = range(steps - 1, -1, -1) if reverse else range(steps)
    with torch.no_grad():
        for k in order:
            h, c = cell(x[torch.as_tensor(base) + k], (h, c))
    return h.numpy()


def _bases(kind, B, rng):
    if kind == "stride1":                       # overlapping, as the evaluation uses them
        return np.arange(B) + 3
    b = rng.randint(0, F - max(STEPS) + 1, size=B)          # shuffled, non-monotonic, repeats allowed
    if B > 2:
        b[0], b[1], b[2] = 40, 2, F - max(STEPS)
    return b


def _window_call(pr, H, base_dev, steps, reverse, B, out_ptr, ld_out, hidden=None, ld_g=None, last_only=1):
    """egp_lstm_fwd_f32 over the windows of the frame table, one problem; last_only: the state after `steps` steps alone."""
    from egopose_amd import _lib as L
    d = L.LstmDesc(T=steps, B=B, hidden=H if hidden is None else hidden, n_problems=1, reverse_mask=1 if reverse else 0,
                   w_hh=pr["w_hh"].data_ptr(), gates_x=pr["gx"].data_ptr(), ld_g=4 * H if ld_g is None else ld_g, ld_h=ld_out,
                   last_only=last_only, seq_base=base_dev.data_ptr())
    d.h_out[0] = out_ptr
    return L.load().egp_lstm_fwd_f32(d, L.current_stream())


def _group_last(pr, H, base_dev, steps, reverse, B):
    """The last state of the full sweep (every step's state stored) over the same windows."""
    from egopose_amd import _lib as L
    h = torch.full((steps, B, H), CANARY, device="cuda")
    L.check(_window_call(pr, H, base_dev, steps, reverse, B, h.data_ptr(), H, last_only=0), "egp_lstm_fwd_f32")
    return h[0 if reverse else steps - 1]


CASES = [(H, B, rev, "stride1") for H in (64, 128) for B in (1, 5, 70) for rev in (0, 1)] + [(64, 70, 1, "shuffled"), (128, 5, 0, "shuffled")]


@pytest.mark.parametrize("H,B,reverse,kind", CASES)
def test_window_last_against_float64_and_the_grouped_sweep(H, B, reverse, kind):
    from egopose_amd import _lib as L
    pr = _problem(H)
    base = _bases(kind, B, np.random.RandomState(7 * B + H))
    assert base.min() >= 0 and base.max() + max(STEPS) <= F
    base_dev = torch.as_tensor(base, dtype=torch.int32, device="cuda")
    ld_out, col0 = H + 8, 3
    for steps in STEPS:
        buf = torch.full((B + 3, ld_out), CANARY, device="cuda")
        out = buf[:B, col0:col0 + H]
        L.check(_window_call(pr, H, base_dev, steps, reverse, B, out.data_ptr(), ld_out), "egp_lstm_fwd_f32")
        got = out.cpu().numpy()
        want = _reference(pr, base, steps, reverse)
        err = np.abs(got - want).max()
        print("H %d B %d reverse %d %s steps %d: max |err| %.3g, max |h| %.3g" % (H, B, reverse, kind, steps, err, np.abs(want).max()))
        np.testing.assert_allclose(got, want, rtol=0, atol=ATOL[H], err_msg="steps %d" % steps)
        assert np.abs(want).max() > 1e-2
        host = buf.cpu().numpy()
        host[:B, col0:col0 + H] = CANARY
        assert (host == CANARY).all(), "steps %d: something outside [B][hidden] was written" % steps
        # the same step body: only the projection's addressing may differ
        np.testing.assert_allclose(got, _group_last(pr, H, base_dev, steps, reverse, B).cpu().numpy(), rtol=0, atol=1e-6, err_msg="steps %d" % steps)


def test_argument_errors_return_without_a_launch():
    from egopose_amd import _lib as L
    H, B = 64, 5
    pr = _problem(H)
    base_dev = torch.arange(B, dtype=torch.int32, device="cuda")
    buf = torch.full((B + 3, H + 8), CANARY, device="cuda")
    ok = dict(steps=3, reverse=1, B=B, out_ptr=buf.data_ptr(), ld_out=H + 8)
    for bad in (dict(hidden=32), dict(hidden=256), dict(steps=0), dict(steps=-2), dict(B=-1), dict(ld_out=H - 1), dict(ld_g=4 * H - 4)):
        rc = _window_call(pr, H, base_dev, **dict(ok, **bad))
        assert rc != 0, bad
        with pytest.raises(ValueError):
            L.check(rc, "egp_lstm_fwd_f32")
    assert _window_call(pr, H, base_dev, **dict(ok, B=0)) == 0                  # no window: a no-op
    assert _window_call(pr, H, base_dev, 3, 1, 0, None, H + 8) == 0
    torch.cuda.synchronize()
    assert (buf == CANARY).all()
    assert _window_call(pr, H, base_dev, **ok) == 0                             # ... and the same arguments, valid, do write
    assert (buf[:B, :H] != CANARY).all() and (buf[B:] == CANARY).all() and (buf[:, H:] == CANARY).all()


def test_python_wrapper_checks_the_windows():
    from egopose_amd import lstm as hl
    torch.manual_seed(1)
    cell = torch.nn.LSTMCell(D, 64).cuda()
    table = torch.randn(20, D, device="cuda")
    out = torch.empty(4, 64, device="cuda")
    n0 = hl.WINDOW_CALLS
    for base in ([0, 1, 2, 18], [-1, 0, 1, 2]):                                 # frames 18 .. 20 / -1 .. 1 of a 20-frame table
        with pytest.raises(ValueError, match="leave the table"):
            hl.window_last(cell, table, torch.tensor(base, dtype=torch.int32, device="cuda"), 3, True, out)
    with pytest.raises(ValueError):
        hl.window_last(cell, table, torch.tensor([0, 1, 2, 3], dtype=torch.int64, device="cuda"), 3, True, out)
    with pytest.raises(ValueError):
        hl.window_last(cell, table.double(), torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda"), 3, True, out)
    assert hl.WINDOW_CALLS == n0
    hl.window_last(cell, table, torch.tensor([0, 1, 2, 17], dtype=torch.int32, device="cuda"), 3, True, out)
    assert hl.WINDOW_CALLS == n0 + 1 and torch.isfinite(out).all()


@pytest.fixture(scope="module")
def policy_vs():
    """The policy's video net of subject_03: 128 features -> 128, bi-LSTM (2 x hidden 64), margin 10."""
    from egopose_amd.nets import VideoStateNet
    torch.manual_seed(21)
    net = VideoStateNet(128, 128, 10, "lstm")
    net.eval()
    net.set_mode("test")
    return net


@pytest.mark.parametrize("n_frames", [21, 45])
def test_online_contexts_on_the_device(policy_vs, n_frames, monkeypatch):
    """21 frames: one tick (T = 1); 45: 25 ticks. Against the float64 definition on the CPU; the window kernel ran once per call."""
    import egopose_amd.nets as nets
    from egopose_amd import lstm as hl
    m = 10
    torch.manual_seed(n_frames)
    x = torch.randn(n_frames, 128)
    net64 = copy.deepcopy(policy_vs).double()
    want = []
    with torch.no_grad():
        for t in range(n_frames - 2 * m):
            net64.initialize(x[:t + 2 * m + 1].double())
            want.append(net64.v_out[t].numpy().copy())
        net64.initialize(x.double())
    want, off = np.stack(want), net64.v_out.numpy()
    net = copy.deepcopy(policy_vs).cuda()
    n0 = hl.WINDOW_CALLS
    got = net.online_contexts(x.cuda())
    assert hl.WINDOW_CALLS == n0 + 1
    assert got.shape == (n_frames - 2 * m, 128) and got.dtype == torch.float32 and got.is_cuda
    err = np.abs(got.cpu().numpy() - want).max()
    print("online_contexts, %d frames: max |err| %.3g" % (n_frames, err))
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=3e-5)
    np.testing.assert_allclose(want[-1], off[-1], rtol=0, atol=1e-12)       # the last tick has seen the whole take
    if n_frames > 2 * m + 1:
        # online is not offline: the comparison above can tell them apart only where the two references differ by well more than
        # its tolerance -- ten times it, on the right half of every earlier row (a fresh 128-wide cell forgets fast: ~1e-3 here)
        assert (np.abs(want[:-1, 64:] - off[:-1, 64:]).max(1) > 10 * 3e-5).all()
    # EGP_LSTM=torch: the gathered windows through the module's own sweep, no window launch
    monkeypatch.setattr(nets, "_LSTM_IMPL", "torch")
    got_t = net.online_contexts(x.cuda())
    assert hl.WINDOW_CALLS == n0 + 1
    np.testing.assert_allclose(got_t.cpu().numpy(), want, rtol=0, atol=3e-5)
