"""TCN video nets on the torch path, float64, against the reference's recorded runs (tests/golden/tcn.npz)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tcn_fixture as F
from conftest import REPO

TOL = 1e-10          # the project's float64 golden tolerance: the two formulations differ by summation order only


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "g"])
def test_plain_nets_match_the_reference(case):
    z = F.golden()
    net, y, dx = F.run_plain(case)
    figures = {"y": F.rel(y, z[case + "__y"]), "dx": F.rel(dx, z[case + "__dx"])}
    want = F.grads(case)
    have = dict(net.named_parameters())
    assert set(want) == set(have)
    for k, g in want.items():
        figures[k] = F.rel(have[k].grad, g)
    print(case, figures)
    assert max(figures.values()) <= TOL, figures


def test_compat_forward_takes_the_reference_layout():
    z = F.golden()
    net = F.plain_net("a")
    with torch.no_grad():
        y = net(torch.from_numpy(z["a__x"]).permute(1, 2, 0))          # (B, C, T) in, (B, C_out, T) out
    assert tuple(y.shape) == (3, 32, 23)
    assert F.rel(y.permute(2, 0, 1), z["a__y"]) <= TOL


def test_video_nets_in_test_mode_match_the_reference():
    z = F.golden()
    vs = F.video_state_net()
    with torch.no_grad():
        vs.initialize(torch.from_numpy(z["e_vs__x"]))
    assert tuple(vs.v_out.shape) == (20, 32) and F.rel(vs.v_out, z["e_vs__v_out"]) <= TOL
    fc = F.forecast_net()
    with torch.no_grad():
        fc.initialize(torch.from_numpy(z["e_fc__x"]))
        y = fc(torch.from_numpy(z["e_fc__state"]))
    assert F.rel(fc.v_out, z["e_fc__v_out"]) <= TOL and F.rel(y, z["e_fc__y"]) <= TOL


def test_video_state_net_in_train_mode_matches_the_reference():
    z = F.golden()
    net, y = F.run_case_f()
    figures = {"y": F.rel(y, z["f__y"])}
    want, have = F.grads("f"), dict(net.named_parameters())
    assert set(want) == set(have)
    for k, g in want.items():
        figures[k] = F.rel(have[k].grad, g)
    print(figures)
    assert max(figures.values()) <= TOL, figures


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("drop", [0, 1])
def test_state_dict_keys_and_their_order(causal, drop):
    from egopose_amd.tcn import TemporalConvNet
    net = TemporalConvNet(16, [16, 32], 3, dropout=0.2 * drop, causal=bool(causal))
    assert list(net.state_dict().keys()) == F.golden()["keys_causal%d_drop%d" % (causal, drop)].tolist()
    n = 2 + causal + drop
    for block in net.network:
        assert block.net[0] is block.conv1 and block.net[n] is block.conv2
        sd = block.state_dict()
        assert sd["net.%d.weight_v" % n].data_ptr() == sd["conv2.weight_v"].data_ptr() == block.conv2.weight_v.data_ptr()
        assert tuple(block.conv1.weight_g.shape) == (block.conv1.out_channels, 1, 1)


@pytest.mark.parametrize("case", ["a", "b", "c", "g", "e_vs", "e_fc"])
def test_reference_state_dicts_load_strictly_and_round_trip(case):
    sd = F.state_dict(case)
    net = {"e_vs": F.video_state_net, "e_fc": F.forecast_net}[case]() if case in ("e_vs", "e_fc") else F.plain_net(case)
    back = net.state_dict()
    assert list(back.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(back[k], sd[k]), k


def test_refusals():
    from egopose_amd.nets import VideoForecastNet, VideoRegNet, VideoStateNet
    from egopose_amd.tcn import TemporalConvNet
    with pytest.raises(ValueError):
        TemporalConvNet(16, [16, 32], kernel_size=4)
    for make in (lambda: VideoStateNet(16, 64, 4, "tcn", {"size": [16, 32]}),
                 lambda: VideoForecastNet(16, 7, 64, 4, "tcn", {"size": [16, 32]}),
                 lambda: VideoRegNet(9, 64, 16, v_net_type="tcn", v_net_param={"size": [16, 32]}),
                 lambda: VideoStateNet(16, 32, 4, "tcn", {"size": [16, 32], "kernel_size": 2})):
        with pytest.raises(ValueError):
            make()
    assert VideoStateNet(16, 128, 4, "tcn").v_net.network[1].dropout == 0.2          # the reference's defaults: [64, 128], 0.2, k = 3
    assert VideoForecastNet(16, 7, 32, 4, "tcn", {"size": [32]}).v_net.causal
    assert VideoRegNet(9, 32, 16, v_net_type="tcn", v_net_param={"size": [32]}, causal=True).v_net.causal
    y = VideoRegNet(9, 32, 16, v_net_type="tcn", v_net_param={"size": [16, 32]}).eval()(torch.zeros(6, 2, 16))
    assert tuple(y.shape) == (12, 9)


def test_compat_models_export_the_reference_s_names():
    from egopose_amd.compat.models import MLP, RNN, ResNet, TemporalConvNet
    from egopose_amd import nets, tcn
    assert TemporalConvNet is tcn.TemporalConvNet and MLP is nets.MLP and RNN is nets.RNN and ResNet is nets.ResNet
    # the way the compat packages are used: their directory on the path, `models` a top-level package
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.path.join(REPO, "egopose_amd", "compat"), HIP_VISIBLE_DEVICES="")
    code = ("from models import MLP, RNN, TemporalConvNet, ResNet; from models.tcn import TemporalConvNet as T2; import models, torch; "
            "assert T2 is TemporalConvNet; print(models.__file__); "
            "print(tuple(TemporalConvNet(4, [1, 2, 8], kernel_size=3, causal=False)(torch.zeros(3, 4, 80)).shape))")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=REPO)
    assert res.returncode == 0, res.stderr
    origin, shape = res.stdout.strip().splitlines()
    assert origin.startswith(os.path.join(REPO, "egopose_amd", "compat")) and shape == "(3, 8, 80)"


def test_dropout_follows_the_seed_in_training_and_is_off_in_eval():
    from egopose_amd.tcn import TemporalConvNet
    torch.manual_seed(5)
    net = TemporalConvNet(16, [16, 32], 3, dropout=0.2).double()
    x = torch.randn(11, 3, 16, dtype=torch.float64)

    def run(seed):
        torch.manual_seed(seed)
        with torch.no_grad():
            return net.forward_tm(x)
    net.train()
    a, b, c = run(1), run(1), run(2)
    assert torch.equal(a, b) and not torch.equal(a, c)
    net.eval()
    d, e = run(1), run(2)
    assert torch.equal(d, e) and not torch.equal(d, a)
    # explicit masks are what both paths are handed: all-ones masks reproduce eval mode
    blk = net.network[0].train()
    ones = torch.ones(11, 3, 16, dtype=torch.float64)
    with torch.no_grad():
        assert torch.equal(blk.forward_tm(x, masks=(ones, ones)), blk.eval().forward_tm(x))


def test_abi_mirror_of_the_descriptor():
    import ctypes
    from egopose_amd import _lib
    assert _lib.load().egp_abi_sizeof(b"egp_tcn_desc") == ctypes.sizeof(_lib.TcnDesc)
