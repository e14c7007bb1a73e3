"""egp_policy_step_f32's validation of an egp_policy_desc, on the host alone: every case here is refused (or, with n == 0,
accepted) before anything is launched, so no device and no context are needed."""
import ctypes as C

import pytest

from egopose_amd import _lib as L


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def mem():
    """64 bytes of host memory at a 16-byte boundary: the dummy target of every non-null pointer (never dereferenced)."""
    buf = C.create_string_buffer(64 + 16)
    return buf, (C.addressof(buf) + 15) & ~15


def _table(p, dims):
    t = (L.MlpLayer * (len(dims) - 1))()
    for l, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        t[l].wt, t[l].bias, t[l].in_dim, t[l].out_dim = p, p, i, o
    return t


def _plain(p, table):
    """A plain step of one row over 8 -> 4 -> 2: 3 context columns + 5 state columns."""
    d = L.PolicyDesc()
    d.n, d.ctx_rows, d.ctx_row_stride, d.ctx_dim, d.t_idx = 1, p, 3, 3, p
    d.state, d.state_dim = p, 5
    d.layers, d.n_layers, d.activation, d.action = table, len(table), 0, p
    return d


def _staged(d, p):
    d.stage_src, d.stage_dst, d.stage_bytes = p, p, 8


def _cell_and_critic(d, p):
    d.cell, d.vlayers = _table(p, (8, 4)), _table(p, (8, 4, 1))


def _staged_cell(d, p):
    _staged(d, p)
    d.cell = _table(p, (8, 4))


def _staged_critic(d, p):
    _staged(d, p)
    d.vlayers = _table(p, (8, 4, 1))


def _noise(d, p):
    d.noise = p


def _nine_layers(d, p):
    d.n_layers = 9


def _broken_chain(d, p):
    d.layers = (L.MlpLayer * 2)(_table(p, (8, 4))[0], _table(p, (3, 2))[0])


def _activation(d, p):
    d.activation = 3


def _odd_slab(d, p):
    d.stage_src, d.stage_dst, d.stage_bytes = p, p, 6


def _negative_rows(d, p):
    d.n = -1


@pytest.mark.parametrize("spoil, message", [
    (_cell_and_critic, "cell with vlayers"),
    (_staged_cell, "a staging slab rides in the plain step only"),
    (_staged_critic, "a staging slab rides in the plain step only"),
    (_noise, "noise needs log_std"),
    (_nine_layers, "1..8 layers"),
    (_broken_chain, "layer dims do not chain"),
    (_activation, "activation: 0 tanh, 1 relu, 2 sigmoid"),
    (_odd_slab, "bad staging slab"),
    (_negative_rows, "n < 0"),
], ids=lambda v: v.__name__.strip("_") if callable(v) else None)
def test_refused_with_the_rule_s_message(lib, mem, spoil, message):
    p = mem[1]
    d = _plain(p, _table(p, (8, 4, 2)))
    spoil(d, p)
    assert lib.egp_policy_step_f32(C.byref(d), None) == -1
    assert message in lib.egp_last_error().decode()


def test_no_rows_is_ok_before_any_pointer_is_looked_at(lib):
    assert lib.egp_policy_step_f32(C.byref(L.PolicyDesc()), None) == L.EGP_OK
