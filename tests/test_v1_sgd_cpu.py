"""tests/v1_sgd_ref.py (the numpy restatement of torch.optim.SGD's single-tensor arithmetic with an exact fp32 FMA) against
torch.optim.SGD(foreach=False) on the CPU, bit for bit, and its FMA against rational arithmetic.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import v1_sgd_ref as G

LR, MU = 0.1, 0.9
MODES = {"nesterov": dict(momentum=MU, nesterov=True), "momentum": dict(momentum=MU, nesterov=False),
         "momentum0": dict(momentum=0.0, nesterov=False)}


def torch_run(p0, grads, *, lr, wd, momentum, nesterov):
    """len(grads) steps of torch.optim.SGD over one CPU tensor -> per step (p, momentum_buffer or None) as numpy"""
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=momentum, weight_decay=wd, nesterov=nesterov, foreach=False)
    out = []
    for g in grads:
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        buf = opt.state[tp].get("momentum_buffer") if momentum else None
        out.append((tp.detach().numpy().copy(), None if buf is None else buf.numpy().copy()))
    return out


def data(n, seed, steps=4):
    rng = np.random.RandomState(seed)
    return rng.standard_normal(n).astype(np.float32), [(rng.standard_normal(n) * 0.3).astype(np.float32) for _ in range(steps)]


@pytest.mark.parametrize("wd", [0.0, 1e-9, 0.05])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [1, 7, 8, 1024, 4099])
def test_restatement_equals_torch_sgd_bit_for_bit(n, mode, wd):
    p0, grads = data(n, 1000 + n)
    kw = MODES[mode]
    want = torch_run(p0, grads, lr=LR, wd=wd, **kw)
    p, buf = p0, None
    for k, g in enumerate(grads):
        p, buf = G.sgd_ref(p, g, buf, lr=LR, wd=wd, first=k == 0, **kw)
        assert np.array_equal(G.bits(p), G.bits(want[k][0])), (n, mode, wd, k, "p")
        if kw["momentum"]:
            assert np.array_equal(G.bits(buf), G.bits(want[k][1])), (n, mode, wd, k, "momentum_buffer")
        else:
            assert buf is None and want[k][1] is None


def test_unfused_form_is_not_what_torch_computes():
    """the guard against a comparison that compares nothing: the three-roundings form differs from torch on the 1024-element
    case, in p after the first step already"""
    p0, grads = data(1024, 2024)
    for wd in (0.0, 0.05):
        want = torch_run(p0, grads, lr=LR, wd=wd, **MODES["nesterov"])
        p, _ = G.sgd_unfused(p0, grads[0], None, lr=LR, wd=wd, first=True, **MODES["nesterov"])
        differ = int((G.bits(p) != G.bits(want[0][0])).sum())
        print(f"unfused form against torch, weight_decay {wd}: {differ} of 1024 elements of p differ after one step")
        assert differ > 0, (wd, differ)


def test_double_rounded_fma_is_not_the_exact_one():
    """a * b + c in float64 cast to fp32 differs from the exact FMA on a constructed boundary case (and only on such cases)"""
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)      # a * b = 1 + 2^-11 + 2^-24: the midpoint of 1 + 2^-11 and its successor
    c = np.float32(2.0 ** -60)                                           # pushes the exact sum just past the midpoint; lost in float64
    exact = G.fma32([a], [b], [c])[0]
    twice = G.fma32_double_rounded([a], [b], [c])[0]
    assert float(exact) == G.fma_fraction(a, b, c) == 1 + 2.0 ** -11 + 2.0 ** -23
    assert float(twice) == 1 + 2.0 ** -11  # ties-to-even of the rounded sum: the wrong neighbour


def test_first_update_keeps_the_bits_of_d():
    """buf = clone(d_p): a gradient holding -0.0 leaves -0.0 in the buffer after the first update (mu * 0 + -0.0 would give +0.0)"""
    p0 = np.array([1.0, -2.0, 0.5, 3.0], dtype=np.float32)
    g = np.array([-0.0, 0.0, -0.0, 1.0], dtype=np.float32)
    for mode in ("nesterov", "momentum"):
        want = torch_run(p0, [g], lr=LR, wd=0.0, **MODES[mode])[0]
        p, buf = G.sgd_ref(p0, g, None, lr=LR, wd=0.0, first=True, **MODES[mode])
        assert G.bits(buf).tolist() == G.bits(g).tolist() == G.bits(want[1]).tolist()
        assert G.bits(buf)[0] == 0x80000000 and G.bits(buf)[1] == 0
        assert np.array_equal(G.bits(p), G.bits(want[0]))
        later = G.sgd_ref(p0, g, np.zeros(4, dtype=np.float32), lr=LR, wd=0.0, first=False, **MODES[mode])[1]
        assert G.bits(later)[0] == 0  # the later-update rule on a zero buffer loses the sign: the two rules are told apart


def adversarial_triples():
    """(a, b, c) fp32: products that land exactly on rounding boundaries with addends far below them (both signs), cancellation
    (c = -fl(a * b), the FMA returns the product's rounding error), subnormal results, and random triples with a scaled addend"""
    rng = np.random.RandomState(7)
    out = []
    for k in range(1, 24):
        x = np.float32(1 + 2.0 ** -k)
        y = np.float32(1 + 2.0 ** -(24 - k)) if 24 - k >= 1 else np.float32(1.5)
        for c in (2.0 ** -60, -2.0 ** -60, 2.0 ** -30, -2.0 ** -30, 0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25):
            out.append((x, y, np.float32(c)))
            out.append((x, np.float32(-y), np.float32(c)))
    for _ in range(120):
        a, b = np.float32(rng.standard_normal()), np.float32(rng.standard_normal())
        out.append((a, b, np.float32(-(a * b))))                                   # cancellation
        out.append((a, b, np.float32(rng.standard_normal() * 2.0 ** rng.randint(-40, 3))))
    for _ in range(40):  # subnormal results
        a, b = np.float32(rng.standard_normal() * 2.0 ** -70), np.float32(rng.standard_normal() * 2.0 ** -70)
        out.append((a, b, np.float32(rng.standard_normal() * 2.0 ** -140)))
    return out


def test_exact_fma_agrees_with_rational_arithmetic():
    tr = adversarial_triples()
    assert len(tr) > 300
    a, b, c = (np.array([t[i] for t in tr], dtype=np.float32) for i in range(3))
    got = G.fma32(a, b, c)
    want = np.array([G.fma_fraction(*t) for t in tr], dtype=np.float64)
    assert np.array_equal(got.astype(np.float64), want), [(tr[i], float(got[i]), want[i]) for i in np.nonzero(got != want)[0][:5]]
    assert all(float(np.float32(w)) == w for w in want)  # the rational rounding produced fp32 numbers
    twice = G.fma32_double_rounded(a, b, c).astype(np.float64)
    assert (twice != want).any()  # the set holds cases the double-rounded form gets wrong
    assert G.round_fraction_f32(Fraction(1, 3)) == float(np.float32(1.0) / np.float32(3.0))


def test_bf16_bits_is_torch_rounding():
    x = np.concatenate([np.random.RandomState(3).standard_normal(4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 3e38, -1e-30], dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(G.bf16_bits(x), want)
