"""The overflow guard of the v1 fine-tuning step and the epoch loop around it, on the GPU (run with -m gpu).

1. the kernels: tvts_adamw_torch / tvts_sgd_torch with `skipped` (the guarded launch) against the unguarded launch, bit for bit, with the norm a real
   tvts_grad_sumsq left on the device (so a NaN inside a FROZEN chunk is seen not to skip), and every byte kept on a skipped launch;
2. FinetuneStep(skip_nonfinite=True) against a real torch.optim.SGD / torch.optim.AdamW on the CPU whose step() is not called on
   the poisoned call, fed this project's own gradients (the construction of tests/test_v1_sgd_gpu.py);
3. train_one_epoch, save_model, auto_load_model.
Everything is bit equality except the torch.optim.AdamW comparison: this project's AdamW kernel is torch's arithmetic in another
operation order (ss * m / denom here, addcdiv's p + value * (m / denom) there; tests/test_v1_finetune_gpu.py holds it to a
per-element bound for that reason), so three updates are held to ADAM_TOL below and, bit for bit, to this project's own unguarded
step with the poisoned call left out.  Step tests: tests/v1_downstream_synth.TINY, 7 classes, B = 3, T = 8."""
import argparse
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
import v1_downstream_synth as S  # noqa: E402
import v1_ema_ref as E  # noqa: E402
import v1_finetune_ref as R  # noqa: E402
from test_v1_finetune_gpu import build, fwd_bwd, store_grads  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
NAN, INF = float("nan"), float("inf")
F = R.FX
CH = 1024
PAD = 1024  # sentinel elements in front of and behind every guarded buffer
EINVAL = -22
DECAY = 0.9999
GROUPS = [0, 1, 255, 1]  # chunk 2 is frozen
VARIANTS = {"adamw": dict(kind="adamw", ema=False), "adamw_ema": dict(kind="adamw", ema=True),
            "sgd": dict(kind="sgd", ema=False, momentum=0.9, nesterov=True), "sgd_ema": dict(kind="sgd", ema=True, momentum=0.9, nesterov=True),
            "sgd_mom0": dict(kind="sgd", ema=False, momentum=0.0, nesterov=False)}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b, what):
    assert torch.equal(bits(a), bits(b)), what


# ================================================================================================ 1. the kernels
_STATE = {}


def kernel_state():
    """fp32 p, g, m, v, e over the four chunks, made once and left unchanged"""
    if not _STATE:
        gen = torch.Generator().manual_seed(2400)
        n = CH * len(GROUPS)
        _STATE["s"] = dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen) * 0.1, m=torch.randn(n, generator=gen) * 0.05,
                           v=torch.rand(n, generator=gen) * 1e-2, e=torch.randn(n, generator=gen))
    return _STATE["s"]


def hyper_table():
    h = torch.full((128,), 7.0)
    h[0], h[1], h[64], h[65] = 1e-2, 3e-3, 0.05, 0.0
    return h


def padded(t, fill):
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=DEV)
    v = buf[PAD:PAD + t.numel()]
    v.copy_(t)
    return v, buf


def launch(K, variant, g, *, guard, step0):
    """grad_sumsq on the device, then one optimizer launch on sentinel-padded copies -> ({name: whole padded buffer}, step_dev,
    skipped, norm).  The unguarded launch gets the device step counter the guarded one forms itself (step0 + 1)."""
    cfg, s = VARIANTS[variant], kernel_state()
    bufs, views = {}, {}
    for k in ("p", "m", "v", "e"):
        views[k], bufs[k] = padded(s[k], 5.0)
    views["sh"], bufs["sh"] = padded(torch.full((s["p"].numel(),), -3.0, dtype=BF16), 9.0)
    gv = g.to(DEV)
    cg = torch.tensor(GROUPS, dtype=torch.uint8, device=DEV)
    nc, partial = torch.zeros(2, dtype=F32, device=DEV), torch.zeros(len(GROUPS), dtype=F32, device=DEV)
    K.grad_sumsq(gv, cg, partial, nc, max_norm=1.0, grad_scale=0.5)
    sd = torch.tensor([step0], dtype=torch.int32, device=DEV)
    sk = torch.tensor([5], dtype=torch.int64, device=DEV)
    hyper = hyper_table().to(DEV)
    ema = dict(ema=views["e"], ema_decay=DECAY) if cfg["ema"] else {}
    if cfg["kind"] == "adamw":
        if guard:
            K.adamw_torch(views["p"], gv, views["m"], views["v"], views["sh"], cg, hyper, 0, grad_scale=0.5, step_dev=sd, norm_coef=nc, skipped=sk, **ema)
        else:
            sd += 1
            K.adamw_torch(views["p"], gv, views["m"], views["v"], views["sh"], cg, hyper, 0, grad_scale=0.5, step_dev=sd, norm_coef=nc, **ema)
    else:
        mom = dict(momentum=cfg["momentum"], nesterov=cfg["nesterov"])
        buf = views["m"] if cfg["momentum"] else None
        if guard:
            K.sgd_torch(views["p"], gv, buf, views["sh"], cg, hyper, 0, grad_scale=0.5, step_dev=sd, norm_coef=nc, skipped=sk, **mom, **ema)
        else:
            sd += 1
            K.sgd_torch(views["p"], gv, buf, views["sh"], cg, hyper, 0, grad_scale=0.5, step_dev=sd, norm_coef=nc, **mom, **ema)
    torch.cuda.synchronize()
    same_bits(gv, g, "the gradient must stay")
    return {k: b.cpu() for k, b in bufs.items()}, int(sd.item()), int(sk.item()), float(nc[0])


def before(variant):
    """the padded buffers as they are in front of a launch"""
    s = kernel_state()
    out = {k: torch.cat([torch.full((PAD,), 5.0), s[k], torch.full((PAD,), 5.0)]) for k in ("p", "m", "v", "e")}
    out["sh"] = torch.cat([torch.full((PAD,), 9.0, dtype=BF16), torch.full((s["p"].numel(),), -3.0, dtype=BF16), torch.full((PAD,), 9.0, dtype=BF16)])
    return out


def poisoned(case):
    g = kernel_state()["g"].clone()
    if case == "inf_first":
        g[0] = INF
    elif case == "nan_last":
        g[-1] = NAN
    elif case == "nan_frozen":
        g[2 * CH + 17] = NAN
    return g


@pytest.mark.parametrize("step0", [0, 3])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_guarded_launch(K, variant, step0):
    """(a) finite: the unguarded launch, step_dev + 1; (b) inf at element 0 of chunk 0 and (c) NaN at the last element of chunk 3:
    every byte kept, sentinels included, step_dev kept, skipped + 1; (d) NaN only inside the frozen chunk: the norm does not see
    it, the launch is (a)"""
    start = before(variant)
    plain, sd, sk, norm = launch(K, variant, poisoned("finite"), guard=False, step0=step0)
    assert math.isfinite(norm) and sd == step0 + 1 and sk == 5
    for k in ("p", "sh"):
        assert not torch.equal(bits(plain[k]), bits(start[k])), f"the unguarded launch must change {k}"
    for case in ("finite", "nan_frozen"):
        got, sd, sk, norm = launch(K, variant, poisoned(case), guard=True, step0=step0)
        assert math.isfinite(norm) and sd == step0 + 1 and sk == 5, (case, norm, sd, sk)
        for k in got:
            same_bits(got[k], plain[k], f"{variant} {case}: {k} against the unguarded launch")
    for case in ("inf_first", "nan_last"):
        got, sd, sk, norm = launch(K, variant, poisoned(case), guard=True, step0=step0)
        assert not math.isfinite(norm) and sd == step0 and sk == 6, (case, norm, sd, sk)
        for k in got:
            same_bits(got[k], start[k], f"{variant} {case}: every byte of {k} (and of its sentinels) must stay")
    for k in ("p", "m", "v", "e", "sh"):  # the sentinels of the launches that did update
        assert torch.equal(bits(plain[k][:PAD]), bits(start[k][:PAD])) and torch.equal(bits(plain[k][-PAD:]), bits(start[k][-PAD:])), k


def test_guard_entry_points_refuse_with_einval(K):
    lib = K._lib.load()
    n = 2 * CH
    t = {k: torch.ones(n + 8, dtype=F32, device=DEV) for k in ("p", "g", "m", "v", "ema")}
    sh = torch.ones(n + 8, dtype=BF16, device=DEV)
    grp = torch.zeros(2, dtype=torch.uint8, device=DEV)
    hyper = hyper_table().to(DEV)
    sdev = torch.ones(2, dtype=torch.int32, device=DEV)
    skp = torch.zeros(2, dtype=torch.int64, device=DEV)
    nc = torch.ones(2, dtype=F32, device=DEV)

    def ptr(x, off=0):
        return None if x is None else ctypes.c_void_p(x.data_ptr() + off)

    def call(kind, **o):
        a = dict(p=ptr(t["p"]), g=ptr(t["g"]), m=ptr(t["m"]), v=ptr(t["v"]), shadow=ptr(sh), chunk_group=ptr(grp), nchunks=2, hyper=ptr(hyper),
                 step=0, step_dev=ptr(sdev), norm_coef=ptr(nc), skipped=ptr(skp), ema=ptr(t["ema"]), momentum=0.9, nesterov=1)
        a.update(o)
        if kind == "adamw":
            return lib.tvts_adamw_torch(a["p"], a["g"], a["m"], a["v"], a["shadow"], a["chunk_group"], a["nchunks"], a["hyper"], a["step"],
                                        a["step_dev"], 0.9, 0.999, 1e-8, 1.0, a["norm_coef"], a["ema"], 0.5, 0.5, a["skipped"], None)
        return lib.tvts_sgd_torch(a["p"], a["g"], a["m"], a["shadow"], a["chunk_group"], a["nchunks"], a["hyper"], a["step"], a["step_dev"],
                                  a["momentum"], a["nesterov"], 1.0, a["norm_coef"], a["ema"], 0.5, 0.5, a["skipped"], None)
    # (skipped=None is the UNGUARDED launch: refused here because its step is 0 and the device counter goes with it)
    common = [dict(p=None), dict(g=None), dict(m=None), dict(chunk_group=None), dict(hyper=None), dict(step_dev=None), dict(norm_coef=None),
              dict(skipped=None, step_dev=None), dict(nchunks=0), dict(nchunks=-3), dict(p=ptr(t["p"], 4)), dict(g=ptr(t["g"], 8)), dict(m=ptr(t["m"], 4)),
              dict(ema=ptr(t["ema"], 4)), dict(shadow=ptr(sh, 2)), dict(shadow=ptr(sh, 4)), dict(skipped=ptr(skp, 4)), dict(step_dev=ptr(sdev, 2)),
              dict(norm_coef=ptr(nc, 2))]
    for o in common + [dict(v=None), dict(v=ptr(t["v"], 4))]:
        assert call("adamw", **o) == EINVAL, ("adamw", o)
    for o in common + [dict(momentum=0.0, nesterov=1)]:
        assert call("sgd", **o) == EINVAL, ("sgd", o)
    # guarded without its cells, with a host step that would do unguarded; the unguarded tvts_adamw_torch refuses misalignment too
    for o in (dict(step=1, step_dev=None), dict(step=1, norm_coef=None)):
        for kind in ("adamw", "sgd"):
            assert call(kind, **o) == EINVAL, (kind, o)
    for o in (dict(p=ptr(t["p"], 4)), dict(shadow=ptr(sh, 2))):
        assert call("adamw", step=1, skipped=None, ema=None, **o) == EINVAL, ("adamw unguarded", o)
    torch.cuda.synchronize()
    for k, x in t.items():
        assert bool((x == 1).all()), k
    assert bool((sh == 1).all()) and sdev.tolist() == [1, 1] and skp.tolist() == [0, 0]
    # accepted: no shadow, no average; momentum 0 without a buffer
    assert call("adamw", shadow=None, ema=None) == 0 and call("sgd", momentum=0.0, nesterov=0, m=None, ema=None) == 0
    torch.cuda.synchronize()
    assert sdev.tolist() == [3, 1] and skp.tolist() == [0, 0] and not bool((t["p"][:n] == 1).any()) and bool((t["p"][n:] == 1).all())


# ================================================================================================ 2. the step
@pytest.fixture(scope="module")
def data():
    """five calls' clips and soft targets, computed once and left unchanged"""
    return [(S.synth_clip(S.TINY, F["B"], F["T"], F["clip_seed"] + 10 * k), R.soft_targets(F["B"], F["classes"], F["target_seed"] + 10 * k))
            for k in range(5)]


def nan_pixel(clip):
    c = clip.clone()
    c[1, 2, 3, 4, 5] = NAN
    return c


def make(m, kind, *, guard, trainable="all", clip_grad=5.0, update_freq=1, with_ema=False):
    from tvts_amd.downstream.finetune_v1 import FinetuneStep, FusedTorchAdamW, FusedTorchSGD, ModelEma, param_groups
    groups = param_groups(m, F["weight_decay"], F["layer_decay"], trainable=trainable)
    lr = F["lr"] if kind == "adamw" else 0.1
    opt = (FusedTorchAdamW(groups, m.store, lr=lr, model=m) if kind == "adamw"
           else FusedTorchSGD(groups, m.store, lr=lr, momentum=0.9, nesterov=True, model=m))
    for g in opt.param_groups:
        g["lr"] = lr * g["lr_scale"]
    ema = ModelEma(m, decay=DECAY) if with_ema else None
    return FinetuneStep(m, opt, clip_grad=clip_grad, update_freq=update_freq, trainable=trainable, model_ema=ema, skip_nonfinite=guard), opt, ema


def cpu_twin(opt, m, kind):
    byptr = {p.data_ptr(): n for n, p in m.named_parameters()}
    leaves, groups = {}, []
    for g in opt.param_groups:
        names = [byptr[p.data_ptr()] for p in g["params"]]
        for n, p in zip(names, g["params"]):
            leaves[n] = p.detach().cpu().clone().requires_grad_(True)
        groups.append(dict(params=[leaves[n] for n in names], lr=g["lr"], weight_decay=g["weight_decay"]))
    if kind == "adamw":
        return leaves, torch.optim.AdamW(groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    return leaves, torch.optim.SGD(groups, lr=0.1, momentum=0.9, nesterov=True, foreach=False)


def run_with_poison(K, data, kind, poison_at, calls=4):
    """`calls` calls of the guarded step, call `poison_at` (0-based) with one NaN pixel; a real torch optimizer on the CPU takes this
    project's gradients and its step() is not called on the poisoned call -> (model, optimizer, step, leaves, torch optimizer)"""
    m = build(rate=0.0)
    step, opt, _ = make(m, kind, guard=True)
    leaves, topt = cpu_twin(opt, m, kind)
    for k in range(calls):
        clip, tg = data[k]
        if k == poison_at:
            m._fresh_shadows()  # (a new model derives its shadows on first use: the snapshot holds the derived ones)
            before_ = {nm: t.clone() for nm, t in (("flat", m.store.flat), ("m", m.store.m), ("shadow", m.store.shadow))}
            out = step.step(nan_pixel(clip), tg)
            assert not math.isfinite(float(out["grad_norm"])) and not math.isfinite(float(out["loss"]))
            for nm, t in (("flat", m.store.flat), ("m", m.store.m), ("shadow", m.store.shadow)):
                same_bits(t, before_[nm], f"{kind}: the poisoned call must keep {nm}")
            assert not bool(m.store.grad.any()), "the gradient buffer is zeroed on a skipped call too"
            continue
        twin = build(rate=0.0, sd={n: v.detach().cpu().clone() for n, v in m.state_dict().items()})
        fwd_bwd(K, twin, clip, tg)
        grads = {n: g.cpu() for n, g in store_grads(twin).items()}
        out = step.step(clip, tg)
        coef = step.norm_coef[1].cpu()
        for n, leaf in leaves.items():
            leaf.grad = grads[n] * coef
        topt.step()
        assert math.isfinite(float(out["grad_norm"]))
    assert int(step.skipped.item()) == 1 and int(opt.step_dev.item()) == calls - 1
    return m, opt, step, leaves, topt


@pytest.mark.parametrize("poison_at", [1, 0])
def test_sgd_step_skips_like_an_omitted_torch_step(K, data, poison_at):
    """poison_at 0: the second call is then torch's FIRST update (the buffer is written, not read)"""
    m, opt, step, leaves, topt = run_with_poison(K, data, "sgd", poison_at)
    params = dict(m.named_parameters())
    sd = opt.state_dict()
    assert len(sd["state"]) == len(leaves) and opt.global_step == 3
    for n, leaf in leaves.items():
        same_bits(params[n], leaf, f"{n} against torch.optim.SGD without the poisoned step")
        same_bits(opt.state[params[n]]["momentum_buffer"], topt.state[leaf]["momentum_buffer"], f"momentum_buffer of {n}")
    fresh = torch.optim.SGD([dict(params=[leaves[n] for n in g["param_names"]]) for g in opt.param_groups], lr=1.0, foreach=False)
    fresh.load_state_dict(sd)  # the real class takes the checkpoint
    opt.load_state_dict(topt.state_dict())  # and back; loading leaves the guard's counter alone
    assert int(opt.step_dev.item()) >= 1 and int(step.skipped.item()) == 1


def test_sgd_skipped_first_call_leaves_no_state(K, data):
    m = build(rate=0.0)
    step, opt, _ = make(m, "sgd", guard=True)
    m.store.m.fill_(NAN)  # the first update that counts must not read the buffer
    step.step(nan_pixel(data[0][0]), data[0][1])
    assert opt.state_dict()["state"] == {} and opt.global_step == 0 and int(step.skipped.item()) == 1
    step.step(*data[1])
    off = m.store.off[m.store_name("head.weight")]
    assert len(opt.state_dict()["state"]) > 0 and opt.global_step == 1 and bool(torch.isfinite(m.store.m[off:off + 64]).all())


# the torch.optim.AdamW comparison (module docstring): per update |dp| <= lr' * |m / (sqrt(v) / rs + eps)| with lr' = lr / bc1 and the
# ratio at most ~ 1 / (1 - b1) in the first steps; the two operation orders differ by a few roundings of that update (relative 2^-22
# at most for four of them) plus one rounding of p per update.  Three updates: 3 * (10 lr 2^-22 + 2^-23 |p|) -- against an update
# that was wrongly applied or wrongly left out, which moves p by about lr.
def adam_tol(p, lr):
    return 3 * (10 * lr * 2.0 ** -22 + 2.0 ** -23 * p.abs())


def test_adamw_step_skips_like_an_omitted_step(K, data):
    m, opt, step, leaves, topt = run_with_poison(K, data, "adamw", 1)
    sd = opt.state_dict()
    assert opt.global_step == 3 and all(s["step"] == 3 for s in sd["state"].values()) and len(sd["state"]) == len(leaves)
    params = dict(m.named_parameters())
    lr_of = {n: g["lr"] for g in opt.param_groups for n in g["param_names"]}
    for n, leaf in leaves.items():
        got, want = params[n].detach().cpu(), leaf.detach()
        assert bool(((got - want).abs() <= adam_tol(want, lr_of[n])).all()), f"{n} against torch.optim.AdamW without the poisoned step"
        assert int(topt.state[leaf]["step"]) == 3
        ea, eb = opt.state[params[n]]["exp_avg"].cpu(), topt.state[leaf]["exp_avg"]
        # (torch forms exp_avg with lerp, m + w (g - m): a few roundings at the magnitude of the larger operand)
        assert float((ea - eb).abs().max()) <= 2.0 ** -20 * float(eb.abs().max()), f"exp_avg of {n}"
    fresh = torch.optim.AdamW([dict(params=[leaves[n] for n in g["param_names"]]) for g in opt.param_groups], lr=1.0, foreach=False)
    fresh.load_state_dict(sd)
    # bit for bit: this project's own unguarded step with the poisoned call left out
    b = build(rate=0.0)
    sb, ob, _ = make(b, "adamw", guard=False)
    for k in (0, 2, 3):
        sb.step(*data[k])
    for nm, x, y in (("flat", m.store.flat, b.store.flat), ("exp_avg", m.store.m, b.store.m), ("exp_avg_sq", m.store.v, b.store.v),
                     ("shadow", m.store.shadow, b.store.shadow)):
        same_bits(x, y, f"{nm} against the unguarded step without the poisoned call")
    opt.load_state_dict(topt.state_dict())  # and back
    assert int(opt.step_dev.item()) == 3


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_average_follows_only_the_calls_that_updated(K, data, kind):
    m = build(rate=0.0)
    step, opt, ema = make(m, kind, guard=True, with_ema=True)
    groups = opt.chunk_group.cpu().numpy()
    want = ema.flat.cpu().numpy().copy()
    for k in range(4):
        clip, tg = data[k]
        step.step(nan_pixel(clip) if k == 1 else clip, tg)
        if k != 1:  # timm's rule on calls 1, 3 and 4 only
            want = E.ema_ref_chunks(want, m.store.flat.cpu().numpy(), groups, DECAY)
    same_bits(ema.flat, torch.from_numpy(np.ascontiguousarray(want)), "the average after one skipped call of four")
    assert bool(torch.isfinite(ema.flat).all()) and int(step.skipped.item()) == 1


@pytest.mark.parametrize("clip_grad", [5.0, None])
@pytest.mark.parametrize("trainable", ["all", "head"])
@pytest.mark.parametrize("update_freq", [1, 2])
def test_finite_data_guarded_equals_unguarded(K, data, update_freq, trainable, clip_grad):
    a, b = build(), build()
    for m in (a, b):
        m.engine.set_drop_seed_base(F["drop_seed"])
    sa, oa, _ = make(a, "adamw", guard=True, trainable=trainable, clip_grad=clip_grad, update_freq=update_freq)
    sb, ob, _ = make(b, "adamw", guard=False, trainable=trainable, clip_grad=clip_grad, update_freq=update_freq)
    for k in range(3 * update_freq):
        ra, rb = sa.step(*data[k % 5]), sb.step(*data[k % 5])
        for key in ("loss", "logits", "grad_norm"):
            assert (ra[key] is None) == (rb[key] is None)
            if ra[key] is not None:
                same_bits(ra[key], rb[key], f"call {k}: {key}")
        for nm, x, y in (("flat", a.store.flat, b.store.flat), ("m", a.store.m, b.store.m), ("v", a.store.v, b.store.v),
                         ("shadow", a.store.shadow, b.store.shadow), ("shadow_t", a.store.shadow_t, b.store.shadow_t)):
            same_bits(x, y, f"call {k}: {nm}")
    assert int(sa.skipped.item()) == 0 and int(oa.step_dev.item()) == 3 == int(ob.step_dev.item())
    assert oa.state_dict()["state"][0]["step"] == 3 == ob.state_dict()["state"][0]["step"]


def test_without_the_guard_the_nan_batch_poisons_the_weights(K, data):
    """what the guard is for: one NaN pixel reaches every trained weight in one launch"""
    m = build(rate=0.0)
    step, opt, _ = make(m, "adamw", guard=False)
    step.step(nan_pixel(data[0][0]), data[0][1])
    off = m.store.off[m.store_name("head.weight")]
    assert bool(torch.isnan(m.store.flat[off:off + 8]).all()) and bool(torch.isnan(m.store.m[off:off + 8]).all())
    assert int(step.skipped.item()) == 0


# ================================================================================================ 3. the loop
def loader5(data, poison_at=None):
    return [(nan_pixel(c) if k == poison_at else c, t) for k, (c, t) in enumerate(data)]


def test_train_one_epoch_stop_and_skip(K, data):
    from tvts_amd.downstream.finetune_v1 import train_one_epoch
    ref = build(rate=0.0)
    sr, _, _ = make(ref, "adamw", guard=True)
    for k in (0, 1):
        sr.step(*data[k])
    after1 = ref.store.flat.clone()
    m = build(rate=0.0)
    step, opt, _ = make(m, "adamw", guard=True)
    with pytest.raises(FloatingPointError, match=r"iteration 2\b"):
        train_one_epoch(step, loader5(data, 2), 0, print_freq=2, on_nonfinite="stop")
    same_bits(m.store.flat, after1, "behind the stop the weights are those after iteration 1")
    # "skip": the epoch runs through; the meters are the means of the per-step outputs
    m = build(rate=0.0)
    step, opt, _ = make(m, "adamw", guard=True)
    stats = train_one_epoch(step, loader5(data, 2), 0, print_freq=2, on_nonfinite="skip")
    twin = build(rate=0.0)
    st, ot, _ = make(twin, "adamw", guard=True)
    outs = [st.step(*b) for b in loader5(data, 2)]
    same_bits(m.store.flat, twin.store.flat, "the loop is the step called five times")
    fin = [k for k in range(5) if k != 2]
    lrs = [g["lr"] for g in opt.param_groups]
    want = dict(loss=sum(float(outs[k]["loss"]) for k in fin) / 4, grad_norm=sum(float(outs[k]["grad_norm"]) for k in fin) / 4,
                class_acc=sum(float(o["class_acc"]) for o in outs) / 5, lr=max(lrs), min_lr=min(lrs), weight_decay=F["weight_decay"], skipped=1.0)
    assert set(stats) == set(want)
    for k, v in want.items():
        assert stats[k] == pytest.approx(v, rel=1e-12, abs=0.0), k
    assert stats["skipped"] == 1
    unguarded, _, _ = make(build(rate=0.0), "adamw", guard=False)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        train_one_epoch(unguarded, loader5(data), 0, on_nonfinite="skip")


def resume_parts(rate=0.1):
    m = build(rate=rate)
    m.engine.set_drop_seed_base(F["drop_seed"])
    step, opt, ema = make(m, "adamw", guard=True, with_ema=True)
    return m, step, opt, ema


def test_resume_continues_bit_for_bit(K, data, tmp_path):
    from tvts_amd.downstream.finetune_v1 import auto_load_model, cosine_scheduler, save_model, train_one_epoch
    lr_sched = cosine_scheduler(F["lr"], 1e-6, 2, 3, warmup_epochs=1)
    wd_sched = cosine_scheduler(F["weight_decay"], F["weight_decay"], 2, 3)
    epochs = [[data[0], data[1], data[2]], [data[3], data[4], data[0]]]

    def epoch(step, e):
        return train_one_epoch(step, epochs[e], e, start_steps=3 * e, lr_schedule_values=lr_sched, wd_schedule_values=wd_sched,
                               num_training_steps_per_epoch=3, print_freq=2)
    ma, sa, oa, ea = resume_parts()
    epoch(sa, 0)
    epoch(sa, 1)
    mb, sb, ob, eb = resume_parts()
    epoch(sb, 0)
    args = argparse.Namespace(output_dir=str(tmp_path / "run"), auto_resume=True, resume="", start_epoch=0)
    save_model(args, 0, mb, ob, model_ema=eb, step=sb)
    ck = torch.load(os.path.join(args.output_dir, "checkpoint-0.pth"), map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch", "args", "model_ema", "drop_seed_base", "calls", "skipped"} and ck["calls"] == 3
    mc, sc, oc, ec = resume_parts()
    mc.store.flat.mul_(0.5)  # a fresh model with other weights, another seed: everything comes from the file
    mc.engine.set_drop_seed_base(1234)
    auto_load_model(args, mc, oc, model_ema=ec, step=sc)
    assert args.start_epoch == 1 and args.resume.endswith("checkpoint-0.pth") and sc.calls == 3
    epoch(sc, 1)
    for nm, x, y in (("flat", ma.store.flat, mc.store.flat), ("m", ma.store.m, mc.store.m), ("v", ma.store.v, mc.store.v), ("ema", ea.flat, ec.flat)):
        same_bits(x, y, f"resumed run against the continuous run: {nm}")
    assert not torch.equal(ea.flat, ma.store.flat)
    assert [s["step"] for s in oa.state_dict()["state"].values()] == [s["step"] for s in oc.state_dict()["state"].values()] == [6] * len(oc.state)
    # the newest all-digit checkpoint wins; checkpoint-best.pth is not one
    save_model(args, 1, mc, oc, model_ema=ec, step=sc)
    torch.save({}, os.path.join(args.output_dir, "checkpoint-best.pth"))
    pick = argparse.Namespace(output_dir=args.output_dir, auto_resume=True, resume="", start_epoch=0)
    auto_load_model(pick, mc, oc, model_ema=ec, step=sc)
    assert pick.resume.endswith("checkpoint-1.pth") and pick.start_epoch == 2
    with pytest.raises(ValueError, match="URL"):
        auto_load_model(argparse.Namespace(output_dir=args.output_dir, auto_resume=False, resume="https://example.org/x.pth", start_epoch=0), mc, oc)
