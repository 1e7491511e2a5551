"""torch.optim.SGD (single-tensor form, dampening 0) restated in numpy (a plain helper module, imported by the tests).

The optimizer optim_factory.create_optimizer builds for `sgd` / `nesterov` / `momentum` (v1/downstream/optim_factory.py:121-126;
v1/scripts/linear_ssv2.sh: --opt sgd --lr 0.1 --momentum 0.9 --weight_decay 1e-9).  In ATen every ``add(x, alpha=a)`` of
torch/optim/sgd.py is ONE fused multiply-add, so per fp32 element, with lr, wd, mu the fp32 roundings of the Python scalars:

    gg  = g * gs
    d   = wd != 0 ? fma(wd, p, gg) : gg               d_p = d_p.add(param, alpha=weight_decay)
    mu != 0:
        first update:  buf = d                        buf = clone(d_p): the bits of d
        later updates: buf = fl(mu * buf) + d         buf.mul_(momentum).add_(d_p, alpha=1): two roundings
        d = nesterov ? fma(mu, buf, d) : buf          d_p.add(buf, alpha=momentum)
    p   = fma(-lr, d, p)                              param.add_(d_p, alpha=-lr)

`fma32` is an EXACT fp32 fused multiply-add: the float64 product of two fp32 numbers is exact (48 significant bits); TwoSum gives
the float64 sum s of product and addend with its exact error; s -> fp32 is the correctly rounded result unless s sits exactly on
an fp32 rounding boundary while the error is not zero, and there the error's sign decides.  (A plain float64 -> fp32 cast of the
sum rounds twice and is wrong on exactly those elements.)  `sgd_ref` is the rule; tests/test_v1_sgd_cpu.py holds it to
torch.optim.SGD(foreach=False) on the CPU bit for bit and fma32 to rational arithmetic.  `sgd_unfused` is the textbook form with
every product and sum rounded on its own: what a kernel without the FMAs would compute, and NOT what torch computes.
"""
from fractions import Fraction

import numpy as np

CH = 1024
F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise over fp32 arrays (finite inputs whose result does not overflow)"""
    a, b, c = (np.asarray(x, dtype=F32) for x in (a, b, c))
    with np.errstate(all="ignore"):
        prod = a.astype(F64) * b.astype(F64)             # exact
        c64 = c.astype(F64)
        s = prod + c64
        bb = s - prod
        err = (prod - (s - bb)) + (c64 - bb)              # TwoSum: prod + c64 == s + err exactly
        r = s.astype(F32)                                 # round to nearest even of the ROUNDED sum
        r64 = r.astype(F64)
        diff = s - r64                                    # exact: s and r64 are neighbours on the fp32 grid's scale
        nb = np.nextafter(r, np.where(diff > 0, F32(np.inf), F32(-np.inf)).astype(F32)).astype(F32)
        nb64 = nb.astype(F64)
        tie = (diff != 0) & (2.0 * s == r64 + nb64)       # s is the midpoint of r and its neighbour towards s
        hi, lo = np.maximum(r, nb), np.minimum(r, nb)
        fixed = np.where(err > 0, hi, np.where(err < 0, lo, r))
        out = np.where(tie, fixed, r).astype(F32)
    return out


def fma32_double_rounded(a, b, c):
    """the form that is NOT accepted: the float64 sum cast to fp32 (two roundings)"""
    a, b, c = (np.asarray(x, dtype=F32) for x in (a, b, c))
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def round_fraction_f32(x: Fraction) -> float:
    """a rational number rounded to the nearest fp32 (ties to even, subnormals included; no overflow handling) as a Python float"""
    if x == 0:
        return 0.0
    sign, x = (-1.0 if x < 0 else 1.0), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)
    n = x / q
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2):
        fl += 1
    return sign * float(fl * q)


def fma_fraction(a, b, c) -> float:
    """fl32(a * b + c) of three fp32 scalars in rational arithmetic"""
    return round_fraction_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def scale32(grad_scale, coef=None):
    """gs as the kernels form it: grad_scale alone, or fl(grad_scale * norm_coef[1])"""
    return F32(grad_scale) if coef is None else F32(grad_scale) * F32(coef)


def sgd_ref(p, g, buf, *, lr, wd, momentum, nesterov, first, gs=1.0):
    """one update of fp32 arrays -> (p', buf'); lr / wd: scalars or per-element arrays (the per-group values spread over the
    elements); buf may be None with momentum 0 (returned as it came); first: the first update"""
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    lr, wd = (np.broadcast_to(np.asarray(x, dtype=np.float64).astype(F32), p.shape) for x in (lr, wd))
    mu = F32(momentum)
    gg = g * F32(gs)
    d = np.where(wd != 0, fma32(wd, p, gg), gg)
    if mu != 0:
        if first:
            buf = d.copy()
        else:
            mb = mu * np.asarray(buf, dtype=F32)
            buf = mb + d
        d = fma32(np.full_like(p, mu), buf, d) if nesterov else buf
    return fma32(-lr, d, p), buf


def sgd_unfused(p, g, buf, *, lr, wd, momentum, nesterov, first, gs=1.0):
    """the same update with every product and every sum rounded to fp32 on its own (no FMA)"""
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    lr, wd, mu = F32(lr), F32(wd), F32(momentum)
    d = g * F32(gs)
    if wd != 0:
        d = wd * p + d
    if mu != 0:
        buf = d.copy() if first else mu * np.asarray(buf, dtype=F32) + d
        d = mu * buf + d if nesterov else buf
    return p - lr * d, buf


def bf16_bits(x):
    """fp32 array -> the uint16 bit patterns of its bf16 rounding (round to nearest even; finite inputs)"""
    u = np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32)


def sgd_ref_chunks(p, g, buf, groups, lr, wd, *, momentum, nesterov, first, gs=1.0):
    """the chunk frame of tvts_sgd_torch: 1024-element chunk c follows the rule with (lr[groups[c]], wd[groups[c]]) iff groups[c] <
    64, else it keeps every bit.  lr / wd: mappings group -> value.  -> (p', buf', stepped: bool per element)"""
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    groups = np.asarray(groups).astype(np.int64)
    assert groups.size * CH == p.size
    lr_g, wd_g = np.zeros(256), np.zeros(256)
    for k in lr:
        lr_g[k], wd_g[k] = lr[k], wd[k]
    stepped = np.repeat(groups < 64, CH)
    pn, bn = sgd_ref(p, g, buf, lr=np.repeat(lr_g[groups], CH), wd=np.repeat(wd_g[groups], CH), momentum=momentum,
                     nesterov=nesterov, first=first, gs=gs)
    if buf is not None and F32(momentum) != 0:
        bn = np.where(stepped, bn, np.asarray(buf, dtype=F32))
    else:
        bn = buf
    return np.where(stepped, pn, p), bn, stepped
