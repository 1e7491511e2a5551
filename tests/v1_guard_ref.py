"""The overflow guard of the v1 fine-tuning step as a numpy restatement (tvts_adamw_torch / tvts_sgd_torch with skipped, csrc/optim.hip):
a sequence of updating calls in which a call whose global gradient norm is not finite keeps every bit of the parameters, the
optimizer state and the average, does not advance the step counter, and counts one skip -- torch.cuda.amp.GradScaler's rule,
``optimizer.step()`` simply not called.  Built on the exact-arithmetic references: tests/v1_sgd_ref.sgd_ref (torch.optim.SGD bit
for bit) and tests/v1_ema_ref.ema_ref (timm's ModelEma rule bit for bit); ``adamw_ref`` is the kernel's own operation order in fp32
numpy (torch.optim.AdamW orders two operations differently, see tests/test_v1_loop_cpu.py)."""
import numpy as np

import v1_ema_ref as E
import v1_sgd_ref as G

F32 = np.float32


def norm_of(g, grad_scale=1.0):
    """|grad_scale| sqrt(sum g^2) as tvts_grad_sumsq leaves it (fp32 result of a double sum): finite iff the guard lets the call update"""
    with np.errstate(all="ignore"):
        return F32(abs(grad_scale)) * F32(np.sqrt(np.sum(np.asarray(g, dtype=np.float64) ** 2)))


def adamw_ref(p, g, m, v, *, lr, wd, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """one update in the order of adamw_torch_kernel: p *= fl(1 - lr wd); m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g;
    p -= fl(lr / bc1) m / (sqrt(v) / fl(sqrt(bc2)) + eps), every operation rounded to fp32, no FMA"""
    p, g, m, v = (np.asarray(x, dtype=F32) for x in (p, g, m, v))
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    decay, ss, rs = F32(1.0 - float(F32(lr)) * float(F32(wd))), F32(float(F32(lr)) / bc1), F32(np.sqrt(bc2))
    b1, b2, o1, o2 = F32(beta1), F32(beta2), F32(1.0 - beta1), F32(1.0 - beta2)
    p = p * decay
    m = b1 * m + o1 * g
    v = b2 * v + (o2 * g) * g
    return p - (ss * m) / (np.sqrt(v) / rs + F32(eps)), m, v


def guarded_run(kind, p, grads, *, lr, wd, decay=None, **kw):
    """the calls of `grads` in order under the guard -> dict(p, m, v, ema, step, skipped, norms).  kind "sgd": kw momentum,
    nesterov (m is the momentum buffer, None until the first update that counted); kind "adamw": kw beta1, beta2, eps.
    decay: also carry timm's average, updated on the calls that updated only."""
    p = np.asarray(p, dtype=F32).copy()
    m = v = None
    if kind == "adamw":
        m, v = np.zeros_like(p), np.zeros_like(p)
    ema = None if decay is None else p.copy()
    step = skipped = 0
    norms = []
    for g in grads:
        norms.append(norm_of(g))
        if not np.isfinite(norms[-1]):  # the whole rule: nothing moves, the step counter stays, one more skip
            skipped += 1
            continue
        step += 1
        if kind == "sgd":
            p, m = G.sgd_ref(p, g, m, lr=lr, wd=wd, first=step == 1, **kw)
        else:
            p, m, v = adamw_ref(p, g, m, v, lr=lr, wd=wd, step=step, **kw)
        if ema is not None:
            ema = E.ema_ref(ema, p, decay)
    return dict(p=p, m=m, v=v, ema=ema, step=step, skipped=skipped, norms=norms)
