"""timm.utils.ModelEma.update restated in numpy (a plain helper module, imported by the tests).

The reference's loop (v1/downstream/engine_for_finetuning.py:84-85,97-98) calls ``model_ema.update(model)``, which computes per
state-dict entry ``ema_v.copy_(ema_v * self.decay + (1. - self.decay) * model_v)`` on fp32 tensors with a Python-float decay.
torch wraps both Python scalars as fp32 for the fp32 tensors, so the expression is three separately rounded fp32 operations:

    d32 = fp32(decay)
    o32 = fp32(1.0 - decay)          the difference formed in DOUBLE (Python floats), rounded once
    ema' = fl( fl(ema * d32) + fl(o32 * p) )

`ema_ref` is that; tests/test_v1_ema_cpu.py holds it to torch's own evaluation of the expression on the CPU, bit for bit.  The two
forms below it are the mistakes a kernel could make; both differ from torch at decay 0.9999 and the test vector shows it.
"""
import numpy as np

CH = 1024


def ema_pair(decay):
    """(d32, o32) as numpy float32 scalars"""
    decay = float(decay)
    return np.float32(decay), np.float32(1.0 - decay)


def ema_ref(e, p, decay):
    """one update of fp32 arrays e (average) and p (parameters): numpy rounds each of the three operations to fp32, no FMA"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d32, o32 = ema_pair(decay)
    a = e * d32
    b = o32 * p
    return a + b


def ema_wrong_o32(e, p, decay):
    """the first wrong form: 1 - decay taken in fp32 (1.00016594e-4 instead of 9.99999975e-5 at decay 0.9999)"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d32 = np.float32(float(decay))
    o32 = np.float32(1.0) - d32
    return e * d32 + o32 * p


def ema_wrong_fused(e, p, decay):
    """the second wrong form: the right constants, but the sum rounded once (what a contracted multiply-add chain gives: the fp32
    products are exact in double, 48 significant bits, and their double sum is rounded to fp32 at the end)"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d32, o32 = ema_pair(decay)
    return (e.astype(np.float64) * np.float64(d32) + np.float64(o32) * p.astype(np.float64)).astype(np.float32)


def ema_vector(seed=0, n=65536):
    """(e, p) fp32: n normal deviates each, then the special elements -- every sign combination of zero, 3e38 (the largest
    magnitudes: the rule must not overflow on them), and elements with e == p.  No denormals."""
    rng = np.random.RandomState(seed)
    e, p = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    same = rng.standard_normal(8).astype(np.float32)
    se = np.array([0.0, -0.0, 0.0, -0.0, 3e38, -3e38, 3e38, 1.0, -3e38], dtype=np.float32)
    sp = np.array([0.0, -0.0, -0.0, 0.0, 3e38, -3e38, 1.0, 3e38, 3e38], dtype=np.float32)
    return np.concatenate([e, se, same]), np.concatenate([p, sp, same])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def ema_ref_chunks(e, p, groups, decay):
    """the chunk gate of tvts_ema_update / tvts_adamw_torch with ema: 1024-element chunk c follows the rule iff groups[c] < 64, else it
    keeps every bit of e"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    steps = np.repeat(np.asarray(groups).astype(np.int64) < 64, CH)
    assert steps.size == e.size == p.size
    return np.where(steps, ema_ref(e, p, decay), e)
