"""ModelEma's rule on the CPU: the numpy restatement (tests/v1_ema_ref.py) against torch's own evaluation of timm's expression, the
constants tvts_amd.hip hands the kernels, and the constructor's refusals.  No GPU."""
import numpy as np
import pytest
import torch

import v1_ema_ref as E

DECAYS = (0.9999, 0.99, 0.5, 0.999999)


def torch_rule(e, p, decay):
    """timm.utils.ModelEma.update's expression, verbatim, on CPU fp32 tensors with a Python-float decay"""
    ema_v, model_v = torch.from_numpy(e.copy()), torch.from_numpy(p.copy())
    return (ema_v * decay + (1. - decay) * model_v).numpy()


@pytest.fixture(scope="module")
def vec():
    e, p = E.ema_vector()
    tiny = np.finfo(np.float32).tiny
    for a in (e, p):
        assert a.dtype == np.float32 and not ((a != 0) & (np.abs(a) < tiny)).any(), "a denormal in the test vector"
    assert e.size == 65536 + 17 and (e[-8:] == p[-8:]).all() and np.signbit(e[65537]) and (np.abs(e) == np.float32(3e38)).any()
    return e, p


@pytest.mark.parametrize("decay", DECAYS)
def test_restatement_is_torch_bit_for_bit(vec, decay):
    e, p = vec
    want = torch_rule(e, p, decay)
    got = E.ema_ref(e, p, decay)
    assert np.isfinite(want).all()
    nz = want[want != 0]
    assert not (np.abs(nz) < np.finfo(np.float32).tiny).any(), "a denormal result"
    assert got.dtype == np.float32 and np.array_equal(E.bits(got), E.bits(want)), int((E.bits(got) != E.bits(want)).sum())
    # a second application, from the first one's result (the average is fed back)
    assert np.array_equal(E.bits(E.ema_ref(got, p, decay)), E.bits(torch_rule(want, p, decay)))


def test_vector_tells_both_wrong_forms_from_torch(vec):
    e, p = vec
    want = E.bits(torch_rule(e, p, 0.9999))
    d32, o32 = E.ema_pair(0.9999)
    assert float(np.float32(1.0) - d32) != float(o32) and abs(float(o32) - 9.99999975e-5) < 1e-12
    assert abs(float(np.float32(1.0) - d32) - 1.00016594e-4) < 1e-12
    n_o32 = int((E.bits(E.ema_wrong_o32(e, p, 0.9999)) != want).sum())
    n_fused = int((E.bits(E.ema_wrong_fused(e, p, 0.9999)) != want).sum())
    print(f"\n   differing elements of {e.size}: fp32 (1 - d32) {n_o32}, one fused rounding {n_fused}")
    assert n_o32 > 1000 and n_fused > 1000, (n_o32, n_fused)


def test_constant_is_not_kept():
    """d32 + o32 != 1: the rule applied to e == p moves it; the fixed point is x * o32 / (1 - d32)"""
    d32, o32 = E.ema_pair(0.9999)
    assert float(d32) + float(o32) != 1.0
    assert abs(float(o32) / (1.0 - float(d32)) - 0.999834) < 1e-6
    x = np.random.RandomState(3).standard_normal(4096).astype(np.float32)
    e = x.copy()
    for _ in range(50):
        e = E.ema_ref(e, x, 0.9999)
    moved = float((E.bits(e) != E.bits(x)).mean())
    print(f"\n   50 applications to a constant: {100 * moved:.1f} % of the elements moved")
    assert moved > 0.05


@pytest.mark.parametrize("decay", DECAYS + (0.0, 1.0))
def test_hip_pair_is_the_restatements(decay):
    from tvts_amd import hip
    d32, o32 = hip.ema_pair(decay)
    rd, ro = E.ema_pair(decay)
    assert isinstance(d32, float) and isinstance(o32, float)
    assert np.float32(d32).tobytes() == rd.tobytes() and np.float32(o32).tobytes() == ro.tobytes()
    assert float(np.float32(d32)) == d32 and float(np.float32(o32)) == o32  # fp32 values: ctypes passes them on unchanged


def test_chunk_gate_of_the_restatement():
    e, p = E.ema_vector(1, 3 * E.CH)
    e, p = e[:3 * E.CH], p[:3 * E.CH]
    out = E.ema_ref_chunks(e, p, [0, 255, 63], 0.99)
    assert np.array_equal(E.bits(out[E.CH:2 * E.CH]), E.bits(e[E.CH:2 * E.CH]))
    assert np.array_equal(E.bits(out[:E.CH]), E.bits(E.ema_ref(e[:E.CH], p[:E.CH], 0.99)))
    assert np.array_equal(E.bits(out[2 * E.CH:]), E.bits(E.ema_ref(e[2 * E.CH:], p[2 * E.CH:], 0.99)))


class _NoDevice:
    """a model whose every attribute access fails: a constructor that refuses first never reaches it"""

    def __getattr__(self, name):
        raise AssertionError(f"ModelEma touched model.{name} before refusing")


def test_constructor_refuses_before_touching_a_device():
    from tvts_amd.downstream.finetune_v1 import ModelEma
    m = _NoDevice()
    with pytest.raises(NotImplementedError, match="device"):
        ModelEma(m, 0.9999, "cpu", "")
    with pytest.raises(NotImplementedError, match="resume"):
        ModelEma(m, decay=0.9999, device="", resume="checkpoint.pth")
    for bad in (-0.1, 1.0001, float("nan"), 2):
        with pytest.raises(ValueError, match="decay"):
            ModelEma(m, decay=bad)
    for bad in (-1e-9, 1.5):
        from tvts_amd import hip
        with pytest.raises(ValueError):
            hip.ema_pair(bad)
