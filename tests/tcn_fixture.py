"""Shared by the TCN tests: tests/golden/tcn.npz (tools/gen_golden_tcn.py) read once, nets rebuilt from its cases."""
import functools

import numpy as np
import torch

from conftest import load_golden

# plain-net cases: C_in, num_channels, kernel_size, causal
CASES = {"a": (16, [16, 32], 3, False), "b": (16, [16, 32], 3, True), "c": (16, [32, 32, 16], 5, False),
         "d": (16, [16, 32], 3, True), "g": (4, [1, 2, 8], 3, False)}
SD_OF = {"d": "b", "f": "e_vs"}          # cases that run another case's net


@functools.lru_cache(maxsize=None)
def golden():
    z = load_golden("tcn.npz")
    return {k: z[k] for k in z.files}


def rel(got, ref):
    """||got - ref|| / ||ref|| (tests/test_gemm_gpu.py:_rel)."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def state_dict(case):
    """The reference's state dict of a case, in its key order; the `net.0` / `net.N` aliases take conv1's / conv2's values."""
    z, tag = golden(), SD_OF.get(case, case)
    out = {}
    for k in z[tag + "__keys"].tolist():
        src = k
        if ".net." in k:
            head, leaf = k[:k.index(".net.")], k.rsplit(".", 1)[1]
            src = head + (".conv1." if ".net.0." in k else ".conv2.") + leaf
        out[k] = torch.from_numpy(z["%s__sd__%s" % (tag, src)])
    return out


def grads(case):
    z, pre = golden(), case + "__grad__"
    return {k[len(pre):]: z[k] for k in z if k.startswith(pre)}


def plain_net(case, dtype=torch.float64, device="cpu"):
    from egopose_amd.tcn import TemporalConvNet
    c_in, size, k, causal = CASES[case]
    net = TemporalConvNet(c_in, size, kernel_size=k, dropout=0.0, causal=causal).double()
    net.load_state_dict(state_dict(case), strict=True)
    return net.to(device=device, dtype=dtype).eval()


def run_plain(case, dtype=torch.float64, device="cpu"):
    """(net, y, dx) of sum(y * R) backpropagated; parameter gradients are left in .grad."""
    z = golden()
    net = plain_net(case, dtype, device)
    x = torch.from_numpy(z[case + "__x"]).to(device=device, dtype=dtype).requires_grad_(True)
    y = net.forward_tm(x)
    (y * torch.from_numpy(z[case + "__R"]).to(device=device, dtype=dtype)).sum().backward()
    return net, y.detach(), x.grad


def video_state_net(dtype=torch.float64, device="cpu"):
    from egopose_amd.nets import VideoStateNet
    net = VideoStateNet(16, 32, 4, "tcn", {"size": [16, 32]}).double()
    net.load_state_dict(state_dict("e_vs"), strict=True)
    return net.to(device=device, dtype=dtype).eval()


def forecast_net(dtype=torch.float64, device="cpu"):
    from egopose_amd.nets import VideoForecastNet
    net = VideoForecastNet(16, 7, 32, 4, "tcn", {"size": [16, 32]}, s_hdim=8, s_net_type="lstm").double()
    net.load_state_dict(state_dict("e_fc"), strict=True)
    return net.to(device=device, dtype=dtype).eval()


def run_case_f(dtype=torch.float64, device="cpu"):
    """VideoStateNet in train mode over the three stored episodes -> (net, y); parameter gradients in .grad."""
    z = golden()
    net = video_state_net(dtype, device)
    net.set_mode("train")
    masks = torch.from_numpy(z["f__masks"]).to(device=device, dtype=dtype)
    net.initialize((masks, [z["f__take0"], z["f__take1"]], z["f__v_metas"].astype(np.int64)))
    y = net(torch.from_numpy(z["f__states"]).to(device=device, dtype=dtype))
    (y * torch.from_numpy(z["f__R"]).to(device=device, dtype=dtype)).sum().backward()
    return net, y.detach()
