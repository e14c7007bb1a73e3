#!/usr/bin/env python3
"""TCN fixtures: the reference's TemporalConvNet (models/tcn.py) and its video nets with v_net_type='tcn', float64 on the CPU.

Imports the reference exactly as tools/gen_golden.py does (same stubs for the absent third-party modules, nothing copied)
and writes tests/golden/tcn.npz. Layout: every net input is stored time-major (T, B, C), as egopose_amd's nets take it; the
reference's TemporalConvNet sees the (B, C, T) permutation of it. Per plain-net case `<c>` in a, b, c, d, g:

    <c>__keys           the state dict's keys in its order, aliases included
    <c>__sd__<key>      its values; an alias `...net.0.*` / `...net.N.*` (the same tensors as conv1 / conv2) is not stored twice
    <c>__x, <c>__y      input and eval-mode output (T, B, C)
    <c>__R              weights of the loss  sum(y * R)
    <c>__dx             its gradient with respect to x
    <c>__grad__<name>   ... and to every parameter (named_parameters)

    a  16 -> [16, 32], k = 3, non-causal, (T, B) = (23, 3)      b  the same, causal
    c  16 -> [32, 32, 16], k = 5, non-causal, (5, 2)            d  b's net (no d__sd__*), (37, 9)
    g  4 -> [1, 2, 8], k = 3, non-causal, (80, 3): the reference's own toy shape

    e_vs__*   VideoStateNet(16, 32, 4, 'tcn', {'size': [16, 32]}) in test mode: window x (28, 16) -> v_out (20, 32)
    e_fc__*   VideoForecastNet(16, 7, 32, 4, 'tcn', {'size': [16, 32]}, s_hdim=8, s_net_type='lstm'): window x (9, 16) -> v_out,
              then one forward(state) -> y
    f__*      the net of e_vs in train mode: episodes of 5, 9 and 7 steps cut from two takes (take0, take1, masks, v_metas,
              states) -> y, R and the parameter gradients of sum(y * R)
    keys_causal<0|1>_drop<0|1>   state-dict key order of TemporalConvNet(16, [16, 32], 3, dropout 0 / 0.2, causal)

Inputs, loss weights and parameters are coarse binary fractions (exact in float32 too); all arrays float64, key lists `<U`.
Size: about 700 kB, not the 300 kB first aimed at. The parameter gradients of these cases are 4 x 6 880 + 23 152 full-precision
float64 values (a, b, d, f and c), about 410 kB that no compression shrinks, and d's output and input gradient add 130 kB more;
what could be saved is (coarse grids, aliases and shared nets stored once). Smaller cases would no longer be the ones listed.
The archive is written with fixed time stamps, so a second run reproduces it byte for byte. Own seeds."""
import io
import os
import sys
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden as G          # noqa: E402  (stubs + workdir helpers)


def _grid(a, steps):
    return np.round(np.asarray(a, np.float64) * steps) / steps


def _write_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp per member: byte-identical from run to run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    G.install_stubs()
    if G.REF not in sys.path:
        sys.path.insert(0, G.REF)
    G.enter_workdir()
    import torch
    torch.set_default_dtype(torch.float64)
    import utils as _ru          # noqa: F401  (reference utils: star exports the models rely on)
    from models.tcn import TemporalConvNet
    from models.video_state_net import VideoStateNet
    from models.video_forecast_net import VideoForecastNet

    rng = np.random.RandomState(4101)
    out = {}

    def shake(net):
        """Parameters away from their initial values (weight_g = ||v|| there, downsample ~ 0.01), on a coarse grid."""
        with torch.no_grad():
            for name, p in net.named_parameters():
                v = p.numpy()
                if name.endswith("weight_g"):
                    v = v * rng.uniform(0.5, 1.5, size=v.shape)
                elif "downsample" in name:
                    v = rng.normal(0.0, 0.3, size=v.shape)
                p.copy_(torch.from_numpy(_grid(v, 1024.0)))
        return net.eval()

    def store_sd(tag, net):
        sd = net.state_dict()
        out[tag + "__keys"] = np.array(list(sd.keys()))
        for k, v in sd.items():
            if ".net." in k:          # alias of conv1 / conv2: same storage, same values
                twin = k.replace(".net.0.", ".conv1.") if ".net.0." in k else k[:k.index(".net.")] + ".conv2." + k.rsplit(".", 1)[1]
                assert sd[twin].data_ptr() == v.data_ptr(), (k, twin)
                continue
            out["%s__sd__%s" % (tag, k)] = v.detach().numpy().astype(np.float64)

    def store_grads(tag, net):
        for k, p in net.named_parameters():
            out["%s__grad__%s" % (tag, k)] = p.grad.numpy().copy()

    for tag, c_in, size, k, causal, (T, B) in (("a", 16, [16, 32], 3, False, (23, 3)), ("b", 16, [16, 32], 3, True, (23, 3)),
                                               ("d", 16, [16, 32], 3, True, (37, 9)), ("c", 16, [32, 32, 16], 5, False, (5, 2)),
                                               ("g", 4, [1, 2, 8], 3, False, (80, 3))):
        if tag != "d":            # (d runs b's net on a longer, wider batch)
            torch.manual_seed(41 + ord(tag))
            net = shake(TemporalConvNet(c_in, size, kernel_size=k, dropout=0.0, causal=causal))
        net.zero_grad()
        x = torch.from_numpy(_grid(rng.normal(size=(T, B, c_in)), 64.0)).requires_grad_(True)
        y = net(x.permute(1, 2, 0).contiguous()).permute(2, 0, 1)
        R = torch.from_numpy(_grid(rng.normal(size=tuple(y.shape)), 8.0))
        (y * R).sum().backward()
        if tag != "d":
            store_sd(tag, net)
        store_grads(tag, net)
        out[tag + "__x"], out[tag + "__y"], out[tag + "__R"], out[tag + "__dx"] = x.detach().numpy(), y.detach().numpy(), R.numpy(), x.grad.numpy()

    for causal in (0, 1):
        for drop in (0, 1):
            keys = list(TemporalConvNet(16, [16, 32], 3, dropout=0.2 * drop, causal=bool(causal)).state_dict().keys())
            out["keys_causal%d_drop%d" % (causal, drop)] = np.array(keys)

    # e: the two video nets in test mode
    torch.manual_seed(51)
    vs = shake(VideoStateNet(16, 32, 4, 'tcn', {'size': [16, 32]}))
    x = torch.from_numpy(_grid(rng.normal(size=(28, 16)), 64.0))
    with torch.no_grad():
        vs.initialize(x)
    store_sd("e_vs", vs)
    out["e_vs__x"], out["e_vs__v_out"] = x.numpy(), vs.v_out.numpy()
    torch.manual_seed(52)
    fc = shake(VideoForecastNet(16, 7, 32, 4, 'tcn', {'size': [16, 32]}, s_hdim=8, s_net_type='lstm'))
    x = torch.from_numpy(_grid(rng.normal(size=(9, 16)), 64.0))
    state = torch.from_numpy(_grid(rng.normal(size=(1, 7)), 64.0))
    with torch.no_grad():
        fc.initialize(x)
        y = fc(state)
    store_sd("e_fc", fc)
    out["e_fc__x"], out["e_fc__v_out"], out["e_fc__state"], out["e_fc__y"] = x.numpy(), fc.v_out.numpy(), state.numpy(), y.numpy()

    # f: VideoStateNet in train mode over three episodes of two takes
    vs.set_mode('train')          # (the net of e_vs)
    takes = [_grid(rng.normal(size=(30, 16)), 64.0), _grid(rng.normal(size=(26, 16)), 64.0)]
    lens, where = [5, 9, 7], [(0, 6), (1, 5), (0, 12)]
    masks = np.ones(sum(lens))
    masks[np.cumsum(lens) - 1] = 0
    v_metas = np.concatenate([np.tile(np.array([w]), (n, 1)) for n, w in zip(lens, where)], 0)
    states = torch.from_numpy(_grid(rng.normal(size=(sum(lens), 5)), 64.0))
    vs.initialize((torch.from_numpy(masks), takes, v_metas))
    y = vs(states)
    R = torch.from_numpy(_grid(rng.normal(size=tuple(y.shape)), 8.0))
    (y * R).sum().backward()
    store_grads("f", vs)
    out["f__take0"], out["f__take1"], out["f__masks"], out["f__v_metas"] = takes[0], takes[1], masks, v_metas.astype(np.float64)
    out["f__states"], out["f__y"], out["f__R"] = states.numpy(), y.detach().numpy(), R.numpy()

    for k, v in out.items():
        assert v.dtype == np.float64 or v.dtype.kind == "U", (k, v.dtype)
    path = os.path.join(G.OUT, "tcn.npz")
    _write_npz(path, out)
    print("wrote", path, "%.0f kB" % (os.path.getsize(path) / 1e3), "%d arrays" % len(out))


if __name__ == "__main__":
    main()
