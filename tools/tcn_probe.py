#!/usr/bin/env python3
"""Time the TCN video net on both paths (HIP events): python tools/tcn_probe.py [T B] [--out FILE]

Default shape 220 704 (the update's padded context: max_len + 2 * fr_margin frames, one column per episode), 128 -> [64, 128],
k = 3, non-causal, dropout off, float32. Times the net's forward (no autograd) and forward + backward on the HIP path
(csrc/egp_tcn.hip + gemm.linear_wgrad) and on the torch path (library GEMMs through autograd), alternating the two, each
window after its own warm-up and long enough to dwarf the clock (>= 0.5 s or 20 passes). TFLOP/s counts the products the
algorithm needs -- 2 * rows * C_in * C_out per tap and residual product, forward; three times that with the backward pass --
over the measured time: a whole-pass figure, not a kernel's share of peak. Fails without a device."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                    # noqa: E402
from egopose_amd import tcn                     # noqa: E402

C_IN, SIZE, K = 128, [64, 128], 3


def flops_forward(T, B):
    rows, total, c_in = T * B, 0, C_IN
    for c_out in SIZE:
        total += 2 * rows * K * (c_in * c_out + c_out * c_out)
        if c_in != c_out:
            total += 2 * rows * c_in * c_out
        c_in = c_out
    return total


def timed(f, min_s=0.5, min_reps=20):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    reps, total_ms = 0, 0.0
    while reps < min_reps or total_ms < min_s * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            f()
        e1.record()
        torch.cuda.synchronize()
        total_ms += e0.elapsed_time(e1)
        reps += 5
    return total_ms / reps * 1e3          # us per pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[220, 704])
    ap.add_argument("--out", default=None, help="also write the result as JSON")
    args = ap.parse_args()
    T, B = args.shape
    if not torch.cuda.is_available():
        raise SystemExit("tcn_probe needs an MI355X: no ROCm device visible")
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = tcn.TemporalConvNet(C_IN, SIZE, kernel_size=K, dropout=0.0).to(dev)
    x = torch.randn(T, B, C_IN, device=dev)
    R = torch.randn(T, B, SIZE[-1], device=dev)

    def fwd():
        with torch.no_grad():
            net.forward_tm(x)

    def fwd_bwd():
        for p in net.parameters():
            p.grad = None
        (net.forward_tm(x) * R).sum().backward()

    res = {"T": T, "B": B, "net": "%d -> %s, k = %d" % (C_IN, SIZE, K), "loadavg": os.getloadavg(),
           "gflop_forward": flops_forward(T, B) / 1e9}
    try:
        res["commit"] = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True,
                                       cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except Exception:
        res["commit"] = "unknown (no git checkout)"
    for rnd in range(2):                     # alternate the paths: two rounds show the spread
        for impl in ("hip", "torch"):
            tcn._IMPL = impl
            calls = tcn.HIP_CALLS
            us_f, us_fb = timed(fwd), timed(fwd_bwd)
            assert (tcn.HIP_CALLS > calls) == (impl == "hip")
            res["%s_round%d" % (impl, rnd)] = {"fwd_us": us_f, "fwd_bwd_us": us_fb,
                                               "fwd_tflops": flops_forward(T, B) / us_f / 1e6,
                                               "fwd_bwd_tflops": 3 * flops_forward(T, B) / us_fb / 1e6}
    tcn._IMPL = "hip"
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
