"""Time the persistent LSTM kernels alone (HIP events): python tools/lstm_probe.py [T B H]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from egopose_amd import _lib as L
T, B, H = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (220, 1280, 64)
lib = L.load()
dev = torch.device("cuda", 0)
gx = torch.randn(T, B, 4 * H, device=dev) * 0.5
w = torch.randn(4 * H, H, device=dev) * 0.1
h = torch.empty(T, B, H, device=dev); gates = torch.empty(T, B, 4 * H, device=dev); cells = torch.empty(T, B, H, device=dev)
dh = torch.randn(T, B, H, device=dev); dpre = torch.empty(T, B, 4 * H, device=dev)
s = L.current_stream()
d = L.LstmDesc(T=T, B=B, hidden=H, n_problems=1, w_hh=w.data_ptr(), gates_save=gates.data_ptr(), cells_save=cells.data_ptr(),
               d_pre=dpre.data_ptr())
d.h_out[0], d.dh_out[0] = h.data_ptr(), dh.data_ptr()


def fwd():
    g = gx.clone()                    # (kept alive to the end of the call: the launch is enqueued by then)
    d.gates_x = g.data_ptr()
    L.check(lib.egp_lstm_fwd_f32(d, s), "fwd")


def bench(f, reps=10):
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


cl = lambda: gx.clone()
bwd = lambda: L.check(lib.egp_lstm_bwd_f32(d, s), "bwd")
t_clone = bench(cl)
print("T %d B %d H %d: fwd %.1f us  bwd %.1f us  (per step %.2f / %.2f us)" % (
    T, B, H, bench(fwd) - t_clone, bench(bwd), (bench(fwd) - t_clone) / T, bench(bwd) / T))
