"""Reference side of the pretraining step with gradient clipping / the overflow guard (tests/test_train_guard_*.py).

``clipped_oracle_step``: the oracle's train_step with ``torch.nn.utils.clip_grad_norm_`` between the backward and the per-tensor
HF-AdamW update -- composed here from the oracle's own pieces (step_losses with autograd, param_groups / GROUP_HPARAMS,
hf_adamw_step), the oracle itself is not changed.  ``clip_by_hand``: the clip rule written out for a list of tensors, which the
CPU test holds clip_grad_norm_ (and with it the composed step) to."""
import math

import torch

from oracle import tvts_oracle as O

CH = 1024
KERNEL_GROUPS = [0, 255, 3, 1, 0]  # the chunk table of every kernel test: the frozen chunk in the middle, the last chunk live
KERNEL_STEPS = (1, 7)
LR4, WD4 = (1e-2, 3e-3, 2e-3, 5e-4), (0.05, 0.0, 0.01, 0.0)


def clip_by_hand(grads, max_norm):
    """clip_grad_norm_'s rule on plain tensors, in double -> (total norm, coefficient, the clipped gradients)"""
    total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    coef = min(1.0, max_norm / (total + 1e-6))
    return total, coef, [g * coef for g in grads]


def clipped_oracle_step(P, batch, arch, opt_state, max_norm=None, norm_fraction=None, truncate_text=True):
    """One single-rank step in place on P, as O.train_step, with the gradients of the trainable leaves clipped to max_norm in
    between.  norm_fraction: max_norm = norm_fraction x this step's own unclipped norm (clipping active by construction).
    max_norm None and norm_fraction None: no clipping (O.train_step's update).  -> dict(loss1, loss2, norm, coef, max_norm)"""
    groups, frozen = O.param_groups(list(P.keys()), arch)
    leaves = {k: t.detach().clone().requires_grad_(k not in frozen) for k, t in P.items()}
    loss1, loss2, *_ = O.step_losses(leaves, batch, arch, truncate_text)
    (loss1 + loss2).backward()
    trainable = [leaves[k] for names in groups for k in names if leaves[k].grad is not None]
    norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(t.grad) for t in trainable])))
    if norm_fraction is not None:
        max_norm = norm_fraction * norm
    coef = 1.0
    if max_norm is not None:
        total = float(torch.nn.utils.clip_grad_norm_(trainable, max_norm))
        assert abs(total - norm) <= 1e-6 * norm
        coef = min(1.0, max_norm / (total + 1e-6))
    steps = opt_state.setdefault("steps", {})
    for gi, names in enumerate(groups):
        lr, wd = O.GROUP_HPARAMS[gi]
        for k in names:
            g = leaves[k].grad
            if g is None:
                if k not in steps:
                    continue
                g = torch.zeros_like(P[k])
            m = opt_state.setdefault("m", {}).setdefault(k, torch.zeros_like(P[k]))
            v = opt_state.setdefault("v", {}).setdefault(k, torch.zeros_like(P[k]))
            steps[k] = steps.get(k, 0) + 1
            O.hf_adamw_step(P[k], g, m, v, steps[k], lr, wd)
    return dict(loss1=float(loss1.detach()), loss2=float(loss2.detach()), norm=norm, coef=coef, max_norm=max_norm)


def kernel_state(seed=2500):
    """fp32 p, g, m, v over the chunks of KERNEL_GROUPS (host tensors; callers copy, nobody writes)"""
    gen = torch.Generator().manual_seed(seed)
    n = CH * len(KERNEL_GROUPS)
    return dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen) * 0.1, m=torch.randn(n, generator=gen) * 0.05,
                v=torch.rand(n, generator=gen) * 1e-2)


def prescaled(g, grad_scale, coef):
    """fl32(fl32(g * grad_scale) * coef): the gradient the clipped launch forms, as a buffer for the launch without a coefficient"""
    f32 = torch.float32
    return (g.to(f32) * torch.full_like(g, grad_scale, dtype=f32)) * torch.full_like(g, coef, dtype=f32)


def nan_pixel(batch, arch, sample=0):
    """a copy of the batch whose clip carries ONE NaN pixel (a numeric input: nothing else about the batch changes).  The pixel is the
    first one of a patch the tube mask KEEPS for that sample (keep_ind), in frame 0: a pixel of a masked patch never reaches the model."""
    out = dict(batch)
    v = batch["video"].clone()
    p = arch["patch"]
    g = arch["image"] // p
    k = int(batch["keep_ind"][sample if batch["keep_ind"].shape[0] > 1 else 0][0])
    v[sample, 0, 0, (k // g) * p, (k % g) * p] = float("nan")
    out["video"] = v
    return out
