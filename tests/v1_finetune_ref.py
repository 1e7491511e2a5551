"""Test-side reference of the v1 fine-tuning step (tvts_amd/downstream/finetune_v1.py) -- TEST INFRASTRUCTURE ONLY, like
tests/v1_downstream_synth.py.  It holds

  * the integer restatement of the stochastic-depth draw (tvts_drop_path_table),
  * a torch restatement of the training forward (oracle.tvts_v1_oracle.video_tokens + a block loop that takes a scale table),
    gradients by autograd, the two losses, the grouping rule of optim_factory.py and a torch.optim.AdamW run over its groups,
  * float64 per-element references with derived bounds for the four arithmetic kernels (the way tests/kernel_bounds.py derives
    them: one unit roundoff u = 2^-24 per fp32 operation the kernel performs, propagated to first order).

It is pinned against the reference's own classes by tests/golden/v1_finetune.npz (tests/test_v1_finetune_cpu.py).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import tvts_v1_oracle as V

try:  # under pytest the tests directory itself is on the path (as the other test files import these two)
    import kernel_bounds as KB
    import v1_downstream_synth as S
except ImportError:  # tests/golden/make_golden_v1_finetune.py
    from tests import kernel_bounds as KB
    from tests import v1_downstream_synth as S

U = KB.U32
M64 = (1 << 64) - 1
SITE_STRIDE = 0x632BE59BD9B4E019   # tvts_amd.hip.DROP_SITE_STRIDE
STEP_STRIDE = 0x51ED270B7F4A7C15   # EngineV1.DROP_STEP_STRIDE
FT_SITE_BASE = 1 << 20             # EngineV1.FT_SITE_BASE

# the fixture's run (tests/golden/make_golden_v1_finetune.py)
FX = dict(seed=61, clip_seed=62, target_seed=63, B=3, T=8, classes=7, drop_path_rate=0.2, drop_seed=0x9A3C5F1B7E24D694,
          lr=1e-3, weight_decay=0.05, layer_decay=0.75, steps=2)
FULL_GRADS = ("head.bias", "head.weight", "norm.weight", "cls_token", "blocks.1.attn.qkv.bias", "blocks.0.mlp.fc2.bias")


# ------------------------------------------------------------------------------------------------ the draw, in integers
def draw_bits(seed: int, site: int, b: int) -> int:
    """the upper 32 bits of the generator at (seed + site * SITE_STRIDE, b): the kernel comment of drop_path_table_kernel"""
    z = (seed + site * SITE_STRIDE) & M64
    z = (z + b * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


def draw_table(seed: int, p_sites, B: int, site_base: int = FT_SITE_BASE) -> np.ndarray:
    """scale [nsites, B] fp32 as tvts_drop_path_table writes it; seed: the unsigned 64-bit value of seed_dev[0]"""
    p32 = np.asarray(p_sites, dtype=np.float32)
    out = np.empty((len(p32), B), dtype=np.float32)
    for s, p in enumerate(p32):
        if not p > 0:
            out[s] = 1.0
            continue
        thr = int(float(p) * 4294967296.0)  # fp32 -> double exact, the product exact (a power of two), truncation
        inv = np.float32(1.0) / (np.float32(1.0) - p)
        for b in range(B):
            out[s, b] = inv if draw_bits(seed & M64, site_base + s, b) >= thr else np.float32(0.0)
    return out


def site_rates(drop_path_rate: float, depth: int):
    """video_encoder.py:138, both branches of a block share its rate"""
    return [torch.linspace(0, drop_path_rate, depth)[l].item() for l in range(depth) for _ in (0, 1)]


def step_seed(seed0: int, k: int) -> int:
    """seed_dev[0] during the k-th finetune_forward (k = 1, 2, ...) of an engine whose seed was seed0"""
    return (seed0 + k * STEP_STRIDE) & M64


# ------------------------------------------------------------------------------------------------ model, losses, grouping
def state(kw=S.TINY, seed=FX["seed"], classes=FX["classes"]):
    return S.synth_state(kw, seed, classes)


def soft_targets(B, C, seed):
    """mixup-like rows: two classes share the mass 1 - 0.1, the smoothing 0.1 is spread over all"""
    g = torch.Generator().manual_seed(seed)
    t = torch.full((B, C), 0.1 / C)
    lam = torch.rand(B, generator=g) * 0.6 + 0.2
    a, b = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    for i in range(B):
        t[i, a[i]] += 0.9 * lam[i]
        t[i, b[i]] += 0.9 * (1 - lam[i])
    return t


def logits_of(sd, clip, kw, table=None):
    """VisionTransformer.forward of v1/downstream/video_encoder.py in training mode with the DropPath scales of `table`
    [2 * depth, B] (None: no stochastic depth).  sd: the class's own names; dtype follows sd / clip."""
    a = S.oracle_arch(kw)
    P = {("" if k.startswith("head.") else S.PREFIX) + k: v for k, v in sd.items()}
    B, _, T = clip.shape[:3]
    tubes, ppf = T // a["tubelet"], (a["image"] // a["patch"]) ** 2
    keep = torch.arange(ppf).view(1, 1, ppf).expand(B, tubes, ppf)
    x = V.video_tokens(P, clip.permute(0, 2, 1, 3, 4), keep, a)
    _, Sq, W = x.shape
    h = a["heads"]
    dh = W // h
    for i in range(a["layers"]):
        p = f"video_model.blocks.{i}."
        sa = sm = 1.0
        if table is not None:
            sa, sm = table[2 * i].to(x.dtype)[:, None, None], table[2 * i + 1].to(x.dtype)[:, None, None]
        y = V.layer_norm(x, P[p + "norm1.weight"], P[p + "norm1.bias"], 1e-6)
        qkv = V.linear(y, P[p + "attn.qkv.weight"], P[p + "attn.qkv.bias"]).reshape(B, Sq, 3, h, dh)
        o = V._softmax_attend(qkv[:, :, 0].permute(0, 2, 1, 3) * dh ** -0.5, qkv[:, :, 1].permute(0, 2, 1, 3),
                              qkv[:, :, 2].permute(0, 2, 1, 3))
        x = x + sa * V.linear(o.permute(0, 2, 1, 3).reshape(B, Sq, W), P[p + "attn.proj.weight"], P[p + "attn.proj.bias"])
        y = V.layer_norm(x, P[p + "norm2.weight"], P[p + "norm2.bias"], 1e-6)
        x = x + sm * V.linear(V.gelu_erf(V.linear(y, P[p + "mlp.fc1.weight"], P[p + "mlp.fc1.bias"])), P[p + "mlp.fc2.weight"],
                              P[p + "mlp.fc2.bias"])
    feat = V.layer_norm(x[:, 0], P["video_model.norm.weight"], P["video_model.norm.bias"], 1e-6)
    return V.linear(feat, P["head.weight"], P["head.bias"])


def soft_ce(logits, t):
    """timm SoftTargetCrossEntropy"""
    return torch.sum(-t * torch.log_softmax(logits, dim=-1), dim=-1).mean()


def smooth_ce(logits, labels, eps):
    """timm LabelSmoothingCrossEntropy"""
    lp = torch.log_softmax(logits, dim=-1)
    nll = -lp.gather(-1, labels[:, None].long())[:, 0]
    return ((1 - eps) * nll + eps * (-lp.mean(dim=-1))).mean()


def group_rule(names_shapes, weight_decay, layer_decay, depth, skip=("pos_embed", "cls_token"), trainable="all"):
    """optim_factory.get_parameter_groups + LayerDecayValueAssigner restated over (name, shape) pairs
    -> [(group name, weight_decay, lr_scale, [member names])] in first-seen order"""
    scales = [layer_decay ** (depth + 1 - i) for i in range(depth + 2)] if layer_decay < 1.0 else None
    out = {}
    for name, shape in names_shapes:
        if trainable == "head" and not name.startswith("head."):
            continue
        nd = len(shape) == 1 or name.endswith(".bias") or name in skip
        g, sc = ("no_decay" if nd else "decay"), 1.0
        if scales is not None:
            if name in ("cls_token", "mask_token", "pos_embed") or name.startswith("patch_embed"):
                lid = 0
            elif name.startswith("blocks"):
                lid = int(name.split(".")[1]) + 1
            else:
                lid = len(scales) - 1
            g, sc = "layer_%d_%s" % (lid, g), scales[lid]
        out.setdefault(g, (g, 0.0 if nd else weight_decay, sc, []))[3].append(name)
    return list(out.values())


def train_run(sd, clip, targets, tables, kw=S.TINY, lr=FX["lr"], weight_decay=FX["weight_decay"], layer_decay=FX["layer_decay"],
              clip_grad=None, smoothing=0.0):
    """len(tables) steps of the reference's loop in torch fp32: forward with tables[k], loss (soft targets [B, C] or int64
    labels with smoothing), clip_grad_norm_, torch.optim.AdamW over the layer-decay groups (lr * lr_scale per group).
    -> (per step: dict(logits, loss, grad_norm, grads), the final parameters)"""
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    groups = [dict(params=[leaves[n] for n in names], weight_decay=wd, lr=lr * sc)
              for _, wd, sc, names in group_rule([(k, tuple(v.shape)) for k, v in sd.items()], weight_decay, layer_decay, kw["depth"])]
    opt = torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    steps = []
    for table in tables:
        opt.zero_grad(set_to_none=True)
        logits = logits_of(leaves, clip, kw, table)
        loss = soft_ce(logits, targets) if targets.dim() == 2 else smooth_ce(logits, targets, smoothing)
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in leaves.items()}
        gn = torch.nn.utils.clip_grad_norm_(list(leaves.values()), clip_grad if clip_grad else float("inf"))
        steps.append(dict(logits=logits.detach().clone(), loss=float(loss), grad_norm=float(gn), grads=grads))
        opt.step()
    return steps, {k: v.detach().clone() for k, v in leaves.items()}


def delta_for_compare(name, delta):
    """the part of a parameter's update that two correct runs can be compared on.  The KEY third of attn.qkv.bias has a gradient
    that is identically zero in exact arithmetic (softmax is invariant under a shift common to all scores of a query, and a key
    bias shifts them by q . b_k): what a run computes there is its own rounding noise, which Adam normalises to a full-size step
    m / (sqrt(v) + eps) of arbitrary sign (and, next to eps = 1e-8, arbitrary size).  Those W elements are left out; the query and
    value thirds stay."""
    if name.endswith("attn.qkv.bias"):
        W = delta.numel() // 3
        return torch.cat([delta[:W], delta[2 * W:]])
    return delta


# ------------------------------------------------------------------------------------------------ per-element kernel references
def drop_path_rows_check(y, scale, S_, residual, out, out_bf16, what):
    """out[r] = residual[r] + scale[r // S] * y[r]: t = fl(s y) (|err| <= u |s y|), out = fl(res + t) (<= u |out|): per element
    |err| <= u (|s y| + |ref|); the bf16 output adds its own rounding u_bf16 |ref|.  Rows of a dropped sample (scale 0): the
    residual's bits (zeros without one); scale 1: the bits of the fp32 add."""
    s = scale.repeat_interleave(S_)[:, None]
    t = torch.where(s == 0, torch.zeros_like(y, dtype=torch.float64), s.double() * y.double())  # (a dropped row's y is not read)
    ref = t if residual is None else residual.double() + t
    bound = U * (t.abs() + ref.abs()) * 1.001 + 1e-45
    worst = 0.0
    exact = (y * s) if residual is None else (residual + y * s)  # fp32 torch: the same two roundings where s is 0 or 1
    rows01 = ((s == 0) | (s == 1))[:, 0]
    if residual is not None:
        exact = torch.where(s == 0, residual, exact)
    else:
        exact = torch.where(s == 0, torch.zeros_like(y), exact)
    if out is not None:
        worst = max(worst, KB.assert_within(out, ref, bound, f"{what}: fp32 out"))
        KB.assert_equal_bits(out[rows01], exact[rows01], f"{what}: rows of scale 0 / 1, fp32")
    if out_bf16 is not None:
        worst = max(worst, KB.assert_within(out_bf16, ref, bound + KB.U_OUT[torch.bfloat16] * ref.abs(), f"{what}: bf16 out"))
        KB.assert_equal_bits(out_bf16[rows01], exact[rows01].bfloat16(), f"{what}: rows of scale 0 / 1, bf16")
    return worst


def soft_ce_ref(x, soft=None, labels=None, eps=0.0, scale=1.0):
    """float64 loss, dlogits, hits of tvts_soft_ce from the fp32 inputs, and the bounds.  With n = ceil(C / 256) + 9 (a thread's
    serial share of a row, six butterfly steps, three wave sums) and z = x - max (|err| <= u |z|):
      e^z          relative (|z| + 3) u                       (the rounding of z, expf within 2 ulp, its own rounding)
      se = sum e^z relative r_se = weighted mean of the above + n u
      lse = log se |err| <= e_lse = r_se + 3 u |lse| + u
      logp = z - lse            <= e_lp = u |z| + e_lse + u |logp|
      t (labels)   relative 3 u ((1 - eps) + eps / C in fp32), exact for soft targets
      loss_b       <= sum |t| e_lp + (n + 5) u sum |t logp|
      loss         <= scale (mean e_b + (ceil(B / 256) + 12) u mean |loss_b|) + u |cell|
      dlogits      <= g (sm st ((|z| + 3) u + r_se + n u + 4 u) + 3 u |t| + u |sm st - t|) + 2 u |ref| + 2e-38 g   (g = scale / B)"""
    B, C = x.shape
    xd = x.double()
    if soft is not None:
        t = soft.double()
        t_rel = 0.0
    else:
        t = torch.full((B, C), eps / C, dtype=torch.float64)
        t[torch.arange(B), labels.long()] += 1.0 - eps
        t_rel = 3 * U
    n = math.ceil(C / 256) + 9
    z = xd - xd.max(dim=1, keepdim=True).values
    ez = z.exp()
    se = ez.sum(dim=1, keepdim=True)
    r_exp = (z.abs() + 3) * U
    r_se = (ez * r_exp).sum(dim=1, keepdim=True) / se + n * U
    lse = se.log()
    e_lse = r_se + 3 * U * lse.abs() + U
    logp = z - lse
    e_lp = U * z.abs() + e_lse + U * logp.abs()
    tl = t * logp
    loss_b = -tl.sum(dim=1)
    e_b = (t.abs() * e_lp).sum(dim=1) + (n + 5 + t_rel / U) * U * tl.abs().sum(dim=1)
    loss = scale * float(loss_b.mean())
    e_loss = scale * (float(e_b.mean()) + (math.ceil(B / 256) + 12) * U * float(loss_b.abs().mean()))
    st = t.sum(dim=1, keepdim=True)
    sm = ez / se
    g = scale / B
    dref = g * (sm * st - t)
    e_d = (g * (sm * st.abs() * (r_exp + r_se + n * U + 4 * U) + (3 * U + t_rel) * t.abs() + U * (sm * st - t).abs())
           + 2 * U * dref.abs() + 2e-38 * g) * 1.01
    hits = int((xd.argmax(dim=1) == t.argmax(dim=1)).sum())
    return loss, e_loss * 1.01, dref, e_d, hits


def grad_norm_ref(g, chunk_group, max_norm, grad_scale=1.0):
    """float64 norm and coef of tvts_grad_sumsq and their bounds.  A chunk's partial: 4 squares and 3 sums per thread, 6 butterfly
    steps, 3 wave sums -- non-negative terms, relative error <= 14 u; the second stage is double (exact next to that).
    norm = grad_scale sqrt(sum): (14 / 2 + 1 (sqrt, rounding to fp32) + 1 (product)) u = 9 u relative; coef = min(1, max_norm /
    (norm + 1e-6)): 9 u + 3 u relative (the sum, the division, fp32(1e-6))."""
    act = (chunk_group != 255).repeat_interleave(1024)
    tot = float((g.double()[act] ** 2).sum())
    norm = abs(grad_scale) * math.sqrt(tot)
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    return norm, 9 * U * norm * 1.01 + 1e-45, coef, (12 * U * coef * 1.01 if coef < 1.0 else 0.0)


def adamw_torch_check(p0, g, m0, v0, p1, m1, v1, shadow, *, lr, wd, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0,
                      coef=None, what):
    """One torch.optim.AdamW step of tvts_adamw_torch on one parameter group against float64 of the stated operation order, from
    the fp32 p0, g, m0, v0 the kernel read.  Constants as the kernel has them: fp32 betas / 1 - betas / eps / lr / wd,
    decay = fp32(1 - lr wd), ss = fp32(lr / bc1), rs = fp32(sqrt(bc2)) formed in double from the double betas.  With
    gs = grad_scale coef (one rounding when there is a coef) and gg = g gs (one more: 2 u relative):
      p' = p0 decay                   |err| <= e_p' = 2 u |p'|                              (decay's rounding, the product)
      m1 = b1 m0 + o1 gg              <= e_m = 4 u (|b1 m0| + |o1 gg|)                      (gg, two products, the sum)
      v1 = b2 v0 + o2 gg gg           <= e_v = 7 u v1                                       (gg twice, two products, the sum)
      r  = sqrt(v1) / rs              <= e_r = (3.5 + 2 + 3) u r                            (sqrt as two roundings; rs, the division)
      d  = r + eps                    <= e_d = e_r + u d
      q  = ss m1 / d                  <= e_q = ss e_m / d + |q| (5 u + e_d / d)
      p1 = p' - q                     <= e_p' + e_q + u |p1|
    -> worst ratio; the shadow is bit for bit bf16(p1)."""
    f = KB.f32_const
    b1, b2, o1, o2, e32, lr32, wd32 = f(beta1), f(beta2), f(1.0 - beta1), f(1.0 - beta2), f(eps), f(lr), f(wd)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    decay, ss, rs = f(1.0 - lr32 * wd32), f(lr32 / bc1), f(math.sqrt(bc2))
    gs = f(grad_scale) if coef is None else f(f(grad_scale) * f(coef))
    p, gg, m, v = p0.double(), g.double() * gs, m0.double(), v0.double()
    pd = p * decay
    e_pd = 2 * U * pd.abs()
    mr = b1 * m + o1 * gg
    e_m = 4 * U * ((b1 * m).abs() + (o1 * gg).abs())
    vr = b2 * v + o2 * gg * gg
    e_v = 7 * U * vr
    r = vr.sqrt() / rs
    e_r = 8.5 * U * r * 1.001
    d = r + e32
    e_d = e_r + U * d
    q = ss * mr / d
    e_q = ss * e_m / d + q.abs() * (5 * U + e_d / d) * 1.001
    pr = pd - q
    e_p = e_pd + e_q + U * pr.abs()
    w = KB.assert_within(m1, mr, e_m + 1e-45, f"{what}: m")
    w = max(w, KB.assert_within(v1, vr, e_v + 1e-45, f"{what}: v"))
    w = max(w, KB.assert_within(p1, pr, e_p + 1e-45, f"{what}: p"))
    if shadow is not None:
        KB.assert_equal_bits(shadow, p1.bfloat16(), f"{what}: bf16 shadow")
    return w
