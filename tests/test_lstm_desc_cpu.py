"""egp_lstm_fwd_f32 / egp_lstm_bwd_f32's validation of an egp_lstm_desc, on the host alone: every case here is refused (or,
with nothing to sweep, accepted) before anything is launched, so no device is needed."""
import ctypes as C

import pytest

from egopose_amd import _lib as L

H = 64


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def mem():
    """64 bytes of host memory at a 16-byte boundary: the dummy target of every non-null pointer (never dereferenced)."""
    buf = C.create_string_buffer(64 + 16)
    return buf, (C.addressof(buf) + 15) & ~15


def _training(p):
    """Two problems over T = 3, B = 5, pairs (ld_h = 2H), ragged, saves on: valid for the forward and for the backward sweep."""
    d = L.LstmDesc(T=3, B=5, hidden=H, n_problems=2, reverse_mask=0b10, w_hh=p)
    d.gates_x, d.gates_save, d.cells_save = p, p, p
    d.h_out[0], d.h_out[1], d.ld_h = p, p, 2 * H
    d.dh_out[0], d.dh_out[1], d.ld_dh, d.d_pre = p, p, 2 * H, p
    d.seq_order, d.seq_steps = p, p
    return d


def _window(p):
    """Last states of B = 5 windows of 3 frames of a table (last_only)."""
    d = L.LstmDesc(T=3, B=5, hidden=H, n_problems=1, reverse_mask=1, w_hh=p, gates_x=p, seq_base=p, last_only=1)
    d.h_out[0], d.ld_h = p, H + 8
    return d


def _set(**fields):
    def spoil(d, p):
        for k, v in fields.items():
            setattr(d, k, {"p": p, "q": p + 16}.get(v, v))      # "p": the dummy that every pointer holds, "q": another one
    spoil.__name__ = "_".join("%s_%s" % (k, "NULL" if v is None else v) for k, v in fields.items()).replace("-", "minus_")
    return spoil


def _no_second_h_out(d, p):
    d.h_out[1] = None


def _no_second_dh_out(d, p):
    d.dh_out[1] = None


BOTH = [
    (_set(T=-1), "negative size"),
    (_set(B=-1), "negative size"),
    (_set(hidden=32), "hidden size 64 and 128"),
    (_set(hidden=256), "hidden size 64 and 128"),
    (_set(n_problems=0), "1..4 problems"),
    (_set(n_problems=5), "1..4 problems"),
    (_set(ld_g=2 * 4 * H - 4), "gate row stride below n_problems * 4H"),
    (_set(ld_g=2 * 4 * H + 2), "not a multiple of 4"),
    (_set(seq_order=None), "seq_order and seq_steps go together"),
    (_set(seq_steps=None), "seq_order and seq_steps go together"),
    (_set(cells_save=None), "gates_save and cells_save go together"),
    (_set(w_hh=None), "NULL pointer"),
]
FORWARD = BOTH + [
    (_set(gates_save=None), "gates_save and cells_save go together"),
    (_set(gates_x=None), "NULL pointer"),
    (_set(ld_h=H - 1), "row stride below the hidden size"),
    (_set(seq_base="p"), "a frame table cannot double as the saved gates"),
    (_no_second_h_out, "NULL h_out / dh_out of a problem"),
]
BACKWARD = BOTH + [
    (_set(gates_save=None, cells_save=None), "NULL pointer"),
    (_set(d_pre=None), "NULL pointer"),
    (_set(ld_dh=H - 1), "row stride below the hidden size"),
    (_set(d_bias_rows=1), "d_bias_rows without d_bias"),
    (_set(d_bias_rows=1, T=0), "d_bias_rows without d_bias"),
    (_no_second_dh_out, "NULL h_out / dh_out of a problem"),
]
WINDOW = [
    (_set(T=0), "a window has at least one step"),
    (_set(T=-2), "negative size"),
    (_set(B=-1), "negative size"),
    (_set(hidden=32), "hidden size 64 and 128"),
    (_set(seq_base=None), "last_only needs seq_base"),
    (_set(ld_g=4 * H - 4), "gate row stride below n_problems * 4H"),
    (_set(ld_g=4 * H + 2), "not a multiple of 4"),
    (_set(ld_h=H - 1), "row stride below the hidden size"),
    (_set(n_problems=2), "last_only sweeps one problem"),
    (_set(gates_save="q", cells_save="q"), "last_only saves nothing"),
    (_set(seq_order="p", seq_steps="p"), "last_only takes no seq_order / seq_steps"),
    (_set(gates_x=None), "NULL pointer"),
]
_ids = lambda v: v.__name__.strip("_") if callable(v) else None


def _refused(lib, fn, d, message):
    assert getattr(lib, fn)(C.byref(d), None) == -1
    assert message in lib.egp_last_error().decode()


@pytest.mark.parametrize("spoil, message", FORWARD, ids=_ids)
def test_forward_refused_with_the_rule_s_message(lib, mem, spoil, message):
    d = _training(mem[1])
    spoil(d, mem[1])
    _refused(lib, "egp_lstm_fwd_f32", d, message)


@pytest.mark.parametrize("spoil, message", BACKWARD, ids=_ids)
def test_backward_refused_with_the_rule_s_message(lib, mem, spoil, message):
    d = _training(mem[1])
    spoil(d, mem[1])
    _refused(lib, "egp_lstm_bwd_f32", d, message)


@pytest.mark.parametrize("spoil, message", WINDOW, ids=_ids)
def test_last_only_refused_with_the_rule_s_message(lib, mem, spoil, message):
    d = _window(mem[1])
    spoil(d, mem[1])
    _refused(lib, "egp_lstm_fwd_f32", d, message)


def test_null_descriptor_is_refused(lib):
    for fn in (lib.egp_lstm_fwd_f32, lib.egp_lstm_bwd_f32):
        assert fn(None, None) == -1
        assert "desc is NULL" in lib.egp_last_error().decode()


@pytest.mark.parametrize("T,B", [(0, 0), (0, 5), (3, 0)])
def test_nothing_to_sweep_is_ok_before_any_pointer_is_looked_at(lib, T, B):
    """An all-zero descriptor, and one with only T or only B set (every pointer NULL), from both functions."""
    for fn in (lib.egp_lstm_fwd_f32, lib.egp_lstm_bwd_f32):
        assert fn(C.byref(L.LstmDesc(T=T, B=B)), None) == L.EGP_OK


def test_last_only_without_windows_is_ok_with_null_pointers(lib):
    d = L.LstmDesc(T=3, B=0, hidden=H, n_problems=1, last_only=1, ld_h=H + 8)
    assert lib.egp_lstm_fwd_f32(C.byref(d), None) == L.EGP_OK
    d.d_bias_rows = 1                      # ... and the rows form of the backward has no row to fill
    assert lib.egp_lstm_bwd_f32(C.byref(d), None) == L.EGP_OK
