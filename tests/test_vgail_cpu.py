"""AgentVGAIL on the CPU: the plain `update_discriminator` (the reference's loop in torch ops) against golden runs of the
reference's own (tests/golden/vgail*.npz, tools/gen_golden_vgail.py), float64; the expert rows, the Discriminator module, the
compat import, and a world_size-2 `gloo` run that must reproduce the single-process run."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from conftest import load_golden  # noqa: E402
import vgail_fixture as V  # noqa: E402
from update_fixture import check_final  # noqa: E402


@pytest.fixture(autouse=True)
def _float64_default():
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


@pytest.mark.parametrize("fixture", V.FIXTURES)
def test_get_expert_states_equals_the_reference(fixture):
    g = load_golden(fixture)
    agent, _ = V.build_agent(g)
    _, masks, v_metas = V.inputs(g)
    es = agent.get_expert_states(v_metas, masks)
    assert es.dtype == torch.float64 and es.shape == (g["masks"].shape[0], int(g["dims"][0]))
    np.testing.assert_allclose(es.numpy()[g["expert_states_rows"]], g["expert_states"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("fixture", V.FIXTURES)
def test_plain_update_discriminator_float64_equals_the_reference(fixture):
    g = load_golden(fixture)
    agent, mods = V.build_agent(g)
    e_loss = V.run_update(agent, g)
    assert isinstance(e_loss, float)
    check_final(mods, g, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(e_loss, float(g["e_loss"]), rtol=1e-9)


def test_compat_import():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "egopose_amd", "compat"))
    try:
        from ego_pose.core.agent_vgail import AgentVGAIL
    finally:
        sys.path.pop(0)
    from egopose_amd.agent import AgentEgo, AgentVGAIL as Ours
    assert AgentVGAIL is Ours and issubclass(AgentVGAIL, AgentEgo)


def test_discriminator_module():
    from egopose_amd.nets import MLP, Discriminator
    torch.manual_seed(0)
    d = Discriminator(MLP(20, [24, 12], "relu"))
    assert list(d.state_dict()) == ["net.affine_layers.0.weight", "net.affine_layers.0.bias", "net.affine_layers.1.weight",
                                    "net.affine_layers.1.bias", "logic.weight", "logic.bias"]
    assert d.logic.weight.shape == (1, 12) and float(d.logic.bias.detach().abs().max()) == 0.0
    assert float(d.logic.weight.detach().abs().max()) <= 0.1 / np.sqrt(12) + 1e-12          # nn.Linear's init bound, scaled by 0.1
    x = torch.randn(7, 20)
    z = d.logits(x)
    assert z.shape == (7, 1)
    torch.testing.assert_close(z, d.logic(d.net(x)), rtol=0, atol=0)
    torch.testing.assert_close(d(x), torch.sigmoid(z), rtol=0, atol=0)
    assert Discriminator(MLP(5, [4], "tanh"), net_out_dim=4).logic.in_features == 4


def test_obs_table_reference_returns_the_file_rows():
    from egopose_amd.expert import ExpertSet, expert_obs_rows
    g = load_golden("vgail.npz")
    env = V.stub_env(g)
    takes = []
    for i, e in enumerate(env.expert_arr):
        L = e["obs"].shape[0]
        takes.append(dict(e, qpos=np.zeros((L, 59)), qvel=np.zeros((L, 58)), head_height_lb=0.0, len=L))
    ex = ExpertSet(takes, env.cnn_feat)
    tab, off = ex.obs_table(None, "cpu", torch.float64, "reference")
    np.testing.assert_array_equal(tab.numpy(), np.concatenate([e["obs"] for e in env.expert_arr], 0))
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum([e["obs"].shape[0] for e in env.expert_arr])]))
    assert ex.obs_table(None, "cpu", torch.float64, "reference")[0] is tab              # cached per (device, dtype, mode)
    with pytest.raises(ValueError, match="13.*14|14.*13"):                              # both widths named
        expert_obs_rows(env.expert_arr, None, "reference", obs_dim=14)
    with pytest.raises(ValueError):
        expert_obs_rows(env.expert_arr, None, "no-such-mode")
    with pytest.raises(ValueError, match="kernel context"):                              # derived rows need the device
        expert_obs_rows([dict(qpos=np.zeros((3, 59)))], None, "reference")


def test_slice_leaving_its_take_raises():
    g = load_golden("vgail.npz")
    agent, _ = V.build_agent(g)
    _, masks, v_metas = V.inputs(g)
    v_metas = v_metas.copy()
    take = int(v_metas[0, 0])
    v_metas[:50, 1] = g["obs%d" % take].shape[0] - 49            # 50 rows from there: one past the take's end
    with pytest.raises(ValueError, match="leave take"):
        agent.get_expert_states(v_metas, masks)
    with pytest.raises(ValueError, match="leave take"):
        agent.update_discriminator(*V.inputs(g)[:2], v_metas)
    v_metas[:50, 1] = -1
    with pytest.raises(ValueError, match="leave take"):
        agent.get_expert_states(v_metas, masks)


def test_obs_phase_is_refused():
    g = load_golden("vgail.npz")
    env = V.stub_env(g)
    env.cfg.obs_phase = True
    with pytest.raises(NotImplementedError, match="obs_phase"):
        V.build_agent(g, env=env)


def test_constructor_defaults_and_module_lists():
    g = load_golden("vgail.npz")
    agent, mods = V.build_agent(g)
    assert agent.discrim_num_update == 10 and agent.discrim_grad_clip == 40.0 and agent.expert_obs == "reference"
    assert agent.discrim_reward_weight == 0.0
    for m in (mods["d"], mods["d_vs"]):
        assert any(m is x for x in agent.sample_modules) and any(m is x for x in agent.update_modules)
    agent.pre_sample()
    assert mods["d_vs"].mode == "test" and agent.policy_vs_net.mode == "test"
    with pytest.raises(ValueError):
        V.build_agent(g, expert_obs="velocities")


# ------------------------------------------------------------------------------------------------ two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(1)
    g = load_golden("vgail.npz")
    agent, mods = V.build_agent(g)
    cut = int(g["ep_lens"][0] + g["ep_lens"][1])                  # episodes 0-1 -> rank 0, episode 2 -> rank 1
    e_loss = V.run_update(agent, g, rows=slice(0, cut) if rank == 0 else slice(cut, None))
    final = {"%s__%s" % (n, k): v.numpy() for n, m in mods.items() for k, v in m.state_dict().items()}
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), e_loss=e_loss, **final)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_update_discriminator_equals_single_process_reference(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    g = load_golden("vgail.npz")
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    n = 0
    for k in g.files:
        if not k.startswith("final_"):
            continue
        key = k[len("final_"):]
        np.testing.assert_allclose(r0[key], g[k], rtol=1e-9, atol=1e-10, err_msg=key)     # == the reference's single process
        np.testing.assert_array_equal(r0[key], r1[key])                                      # ranks stay bit-identical
        n += 1
    assert n == 14
    np.testing.assert_allclose(float(r0["e_loss"]), float(g["e_loss"]), rtol=1e-9)
    assert float(r0["e_loss"]) == float(r1["e_loss"])
