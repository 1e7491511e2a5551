"""Gradient clipping by global norm and the device overflow guard of the PRETRAINING step (run with -m gpu).

1. the kernels on flat buffers: tvts_adamw_hf_guarded against tvts_adamw_hf (bit equality: a clipped launch is the plain launch on
   a pre-scaled gradient; coefficient 1 and no coefficient are today's launch; the guard either is the unguarded launch or keeps
   every byte), tvts_fp8_update_scales_guarded per float, the host refusals;
2. StepRunner(clip_grad=, skip_nonfinite=) on the tiny architectures: the default step unchanged, the clipped step against the
   oracle composed in tests/train_guard_ref.py, the overflow sequence in bf16 and under e4m3 weight gradients, the named refusals;
3. GraphReplay and the trainer's two config keys.
The two-rank run is tests/test_train_guard_dist_gpu.py."""
import ctypes
import logging
import math
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_guard_ref as G  # noqa: E402

from oracle import tvts_oracle as O  # noqa: E402  (checker only)

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
NAN, INF = float("nan"), float("inf")
CH, PAD, EINVAL = 1024, 1024, -22
ARGS = types.SimpleNamespace(local_rank=0, rank=0, world_size=1)
COEF = 0.37


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


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ================================================================================================ 1. the kernels
_STATE = {}


def kstate():
    if not _STATE:
        _STATE["s"] = G.kernel_state()
    return _STATE["s"]


def padded(t, fill):
    """a device copy of t between two runs of PAD sentinel elements -> (the view the kernel gets, the whole buffer)"""
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=DEV)
    v = buf[PAD:PAD + t.numel()]
    v.copy_(t)
    return v, buf


def before():
    s = kstate()
    out = {k: torch.cat([torch.full((PAD,), 5.0), s[k], torch.full((PAD,), 5.0)]) for k in ("p", "m", "v")}
    out["sh"] = torch.cat([torch.full((PAD,), 9.0, dtype=BF16), torch.full((s["p"].numel(),), -3.0, dtype=BF16), torch.full((PAD,), 9.0, dtype=BF16)])
    return out


def launch(K, entry, g, *, step, hyper, grad_scale=1.0, norm_coef=None, guard=False, bufs=None, dev_step=False):
    """one launch of K.adamw_hf ("hf") or K.adamw_hf_guarded ("new") on sentinel-padded copies of the kernel state (or on `bufs`, the
    buffers an earlier call returned) -> dict(whole padded buffers ..., step_dev, skipped).  hyper: lr / wd travel in the device
    table (with the device step counter) and the host lists hold other numbers; else host lists and the host step (dev_step: host
    lists and the device step counter).  guard: the device counter starts at step - 1 and the launch advances it."""
    s = kstate()
    if bufs is None:
        views, whole = {}, {}
        for k in ("p", "m", "v"):
            views[k], whole[k] = padded(s[k], 5.0)
        views["sh"], whole["sh"] = padded(torch.full((s["p"].numel(),), -3.0, dtype=BF16), 9.0)
        bufs = dict(views=views, whole=whole, sd=torch.tensor([step - 1 if guard else step], dtype=torch.int32, device=DEV),
                    sk=torch.zeros(1, dtype=torch.int64, device=DEV))
    views, sd, sk = bufs["views"], bufs["sd"], bufs["sk"]
    gv = g.to(DEV)
    cg = torch.tensor(G.KERNEL_GROUPS, dtype=torch.uint8, device=DEV)
    kw = dict(grad_scale=grad_scale)
    lr4, wd4 = G.LR4, G.WD4
    if hyper:
        kw.update(step_dev=sd, hyper_dev=torch.tensor(G.LR4 + G.WD4, dtype=F32, device=DEV))
        lr4, wd4 = (7.0,) * 4, (7.0,) * 4  # (never read: the table is)
    elif guard or dev_step:
        kw.update(step_dev=sd)
    nc = None if norm_coef is None else torch.tensor(norm_coef, dtype=F32, device=DEV)
    host_step = 0 if (hyper or guard or dev_step) else step
    if entry == "hf":
        K.adamw_hf(views["p"], gv, views["m"], views["v"], views["sh"], cg, lr4, wd4, host_step, **kw)
    else:
        K.adamw_hf_guarded(views["p"], gv, views["m"], views["v"], views["sh"], cg, lr4, wd4, host_step, norm_coef=nc,
                           skipped=sk if guard else None, **kw)
    torch.cuda.synchronize()
    same_bits(gv, g, "the gradient must stay")
    out = {k: b.cpu() for k, b in bufs["whole"].items()}
    out.update(step_dev=int(sd.item()), skipped=int(sk.item()), bufs=bufs)
    return out


def frozen_and_sentinels_kept(got, what):
    start = before()
    lo, hi = PAD + CH, PAD + 2 * CH  # chunk 1 of KERNEL_GROUPS is the frozen one
    for k in ("p", "m", "v", "sh"):
        same_bits(got[k][lo:hi], start[k][lo:hi], f"{what}: the frozen chunk of {k}")
        same_bits(got[k][:PAD], start[k][:PAD], f"{what}: the sentinels in front of {k}")
        same_bits(got[k][-PAD:], start[k][-PAD:], f"{what}: the sentinels behind {k}")
        assert not torch.equal(bits(got[k][PAD:lo]), bits(start[k][PAD:lo])), f"{what}: chunk 0 of {k} must change"
        assert not torch.equal(bits(got[k][-PAD - CH:-PAD]), bits(start[k][-PAD - CH:-PAD])), f"{what}: the last chunk of {k} must change"


@pytest.mark.parametrize("hyper", [False, True])
@pytest.mark.parametrize("step", G.KERNEL_STEPS)
def test_clipped_launch_is_the_plain_launch_on_a_prescaled_gradient(K, step, hyper):
    """norm_coef = [n, 0.37], grad_scale 0.3: the bits of K.adamw_hf (grad_scale 1) on a buffer holding fl32(fl32(g * 0.3) * 0.37)"""
    g = kstate()["g"]
    got = launch(K, "new", g, step=step, hyper=hyper, grad_scale=0.3, norm_coef=[2.5, COEF])
    want = launch(K, "hf", G.prescaled(g, 0.3, COEF), step=step, hyper=hyper, grad_scale=1.0)
    for k in ("p", "m", "v", "sh"):
        same_bits(got[k], want[k], f"step {step} hyper_dev {hyper}: {k}")
    frozen_and_sentinels_kept(got, f"step {step} hyper_dev {hyper}")
    unclipped = launch(K, "hf", g, step=step, hyper=hyper, grad_scale=0.3)
    assert not torch.equal(bits(got["m"]), bits(unclipped["m"]))  # (the coefficient does something)


@pytest.mark.parametrize("hyper", [False, True])
@pytest.mark.parametrize("step", G.KERNEL_STEPS)
def test_coefficient_one_and_no_coefficient_are_todays_launch(K, step, hyper):
    g = kstate()["g"]
    want = launch(K, "hf", g, step=step, hyper=hyper, grad_scale=0.3)
    for nc in ([2.5, 1.0], None):
        got = launch(K, "new", g, step=step, hyper=hyper, grad_scale=0.3, norm_coef=nc)
        for k in ("p", "m", "v", "sh"):
            same_bits(got[k], want[k], f"step {step} hyper_dev {hyper} norm_coef {nc}: {k}")
        frozen_and_sentinels_kept(got, f"norm_coef {nc}")
        assert got["step_dev"] == step and got["skipped"] == 0


@pytest.mark.parametrize("hyper", [False, True])
@pytest.mark.parametrize("step", G.KERNEL_STEPS)
def test_guarded_launch(K, step, hyper):
    """finite norm: the unguarded launch with step = step_dev + 1, step_dev advanced; inf, then NaN, on the same buffers: every byte
    (sentinels included) kept, step_dev kept, skipped 1, then 2"""
    g = kstate()["g"]
    plain = launch(K, "new", g, step=step, hyper=hyper, grad_scale=0.3, norm_coef=[2.5, COEF], dev_step=True)
    hf = launch(K, "hf", G.prescaled(g, 0.3, COEF), step=step, hyper=hyper, dev_step=True)
    got = launch(K, "new", g, step=step, hyper=hyper, grad_scale=0.3, norm_coef=[2.5, COEF], guard=True)
    for k in ("p", "m", "v", "sh"):
        same_bits(plain[k], hf[k], f"step {step} hyper_dev {hyper}: the unguarded launch against K.adamw_hf, {k}")
    assert got["step_dev"] == step and got["skipped"] == 0
    for k in ("p", "m", "v", "sh"):
        same_bits(got[k], plain[k], f"step {step} hyper_dev {hyper}: guarded against unguarded, {k}")
    frozen_and_sentinels_kept(got, "guarded, finite norm")
    for n, bad in enumerate((INF, NAN), 1):
        again = launch(K, "new", g, step=step, hyper=hyper, grad_scale=0.3, norm_coef=[bad, COEF], guard=True, bufs=got["bufs"])
        assert again["step_dev"] == step and again["skipped"] == n, (bad, again["step_dev"], again["skipped"])
        for k in ("p", "m", "v", "sh"):
            same_bits(again[k], got[k], f"norm {bad}: every byte of {k} (and of its sentinels) must stay")
    # a skipped FIRST call: the counters say so and the state is the initial one
    first = launch(K, "new", g, step=step, hyper=hyper, grad_scale=0.3, norm_coef=[-INF, COEF], guard=True)
    assert first["step_dev"] == step - 1 and first["skipped"] == 1
    start = before()
    for k in ("p", "m", "v", "sh"):
        same_bits(first[k], start[k], f"skipped first call: {k}")


def test_guarded_scale_update(K):
    """slots {3.5, 0, inf, NaN, -0.0} over old scales {2, 2, 2, 2, 0}: only the finite positive maximum becomes a scale, the slot
    that has never had one gets 1.0, amax is zeroed; a non-finite guard norm keeps every scale; the old entry point is unchanged"""
    amax0 = torch.tensor([3.5, 0.0, INF, NAN, -0.0], dtype=F32)
    scale0 = torch.tensor([2.0, 2.0, 2.0, 2.0, 0.0], dtype=F32)
    q = (torch.tensor(3.5, dtype=F32) / torch.tensor(448.0, dtype=F32)).item()

    def run(fn, *extra):
        a, s = amax0.to(DEV), scale0.to(DEV)
        fn(a, s, *extra)
        torch.cuda.synchronize()
        return a.cpu(), s.cpu()
    a, s = run(K.fp8_update_scales_guarded)
    same_bits(s, torch.tensor([q, 2.0, 2.0, 2.0, 1.0], dtype=F32), f"guarded scales {s.tolist()}")
    same_bits(a, torch.zeros(5, dtype=F32), f"amax {a.tolist()}")
    a, s = run(K.fp8_update_scales_guarded, torch.tensor([1.25, 1.0], dtype=F32, device=DEV))  # finite norm: the same rule
    same_bits(s, torch.tensor([q, 2.0, 2.0, 2.0, 1.0], dtype=F32), f"guarded scales, finite norm {s.tolist()}")
    for bad in (INF, NAN):
        a, s = run(K.fp8_update_scales_guarded, torch.tensor([bad, 1.0], dtype=F32, device=DEV))
        same_bits(s, torch.tensor([2.0, 2.0, 2.0, 2.0, 1.0], dtype=F32), f"norm {bad}: {s.tolist()}")
        same_bits(a, torch.zeros(5, dtype=F32), f"amax {a.tolist()}")
    a, s = run(K.fp8_update_scales)  # as it was: inf becomes a scale, NaN compares false and keeps, the zero slot gets 1.0
    same_bits(s, torch.tensor([q, 2.0, INF, 2.0, 1.0], dtype=F32), f"old entry point {s.tolist()}")
    same_bits(a, torch.zeros(5, dtype=F32), "old entry point amax")
    # an amax whose quotient underflows to 0, and stale non-finite scales: never left for a quantiser to divide by
    a_, s_ = torch.tensor([1e-45, 0.0, 0.0, 5.0], dtype=F32, device=DEV), torch.tensor([NAN, INF, NAN, NAN], dtype=F32, device=DEV)
    K.fp8_update_scales_guarded(a_, s_)
    assert s_.cpu().tolist() == [1.0, 1.0, 1.0, (torch.tensor(5.0) / 448.0).item()] and a_.cpu().tolist() == [0.0] * 4


def test_new_entry_points_refuse_with_einval(K):
    lib = K._lib.load()
    n = 2 * CH
    t = {k: torch.ones(n + 8, dtype=F32, device=DEV) for k in ("p", "g", "m", "v")}
    sh = torch.ones(n + 8, dtype=BF16, device=DEV)
    grp = torch.zeros(2, dtype=torch.uint8, device=DEV)
    hyper = torch.full((8,), 1e-3, dtype=F32, device=DEV)
    sdev = torch.ones(2, dtype=torch.int32, device=DEV)
    skp = torch.zeros(2, dtype=torch.int64, device=DEV)
    nc = torch.ones(2, dtype=F32, device=DEV)
    lr = (ctypes.c_float * 4)(1e-3, 1e-3, 1e-3, 1e-3)
    wd = (ctypes.c_float * 4)(0.0, 0.0, 0.0, 0.0)

    def ptr(x, off=0):
        return None if x is None else ctypes.c_void_p(x.data_ptr() + off)

    def call(**o):
        a = dict(p=ptr(t["p"]), g=ptr(t["g"]), m=ptr(t["m"]), v=ptr(t["v"]), shadow=ptr(sh), chunk_group=ptr(grp), nchunks=2,
                 lr=ctypes.cast(lr, ctypes.c_void_p), wd=ctypes.cast(wd, ctypes.c_void_p), step=0, step_dev=ptr(sdev), hyper=ptr(hyper),
                 norm_coef=ptr(nc), skipped=ptr(skp))
        a.update(o)
        return lib.tvts_adamw_hf_guarded(a["p"], a["g"], a["m"], a["v"], a["shadow"], a["chunk_group"], a["nchunks"], a["lr"], a["wd"],
                                         a["step"], a["step_dev"], a["hyper"], 0.9, 0.999, 1e-6, 1.0, a["norm_coef"], a["skipped"], None)
    refused = [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(chunk_group=None), dict(lr=None), dict(wd=None),
               dict(nchunks=0), dict(nchunks=-3), dict(p=ptr(t["p"], 4)), dict(g=ptr(t["g"], 8)), dict(m=ptr(t["m"], 4)),
               dict(v=ptr(t["v"], 12)), dict(shadow=ptr(sh, 2)), dict(shadow=ptr(sh, 4)), dict(skipped=ptr(skp, 4)),
               dict(step_dev=ptr(sdev, 2)), dict(norm_coef=ptr(nc, 2)), dict(hyper=ptr(hyper, 2)),
               dict(step_dev=None, hyper=None), dict(norm_coef=None),              # under the guard both cells are required
               dict(step=1, step_dev=None, hyper=None), dict(step=1, norm_coef=None),   # ... a host step does not replace them
               dict(skipped=None, step_dev=None, hyper=None),                      # unguarded: step 0 without the device counter
               dict(skipped=None, step=1, step_dev=None)]                          # the table without the device counter
    for o in refused:
        assert call(**o) == EINVAL, o
    for o in (dict(amax=None), dict(scale=None), dict(n=0), dict(n=-1), dict(norm=ptr(nc, 2))):
        a = dict(amax=ptr(t["p"]), scale=ptr(t["m"]), n=4, norm=ptr(nc))
        a.update(o)
        assert lib.tvts_fp8_update_scales_guarded(a["amax"], a["scale"], a["n"], a["norm"], None) == EINVAL, o
    torch.cuda.synchronize()
    for k, x in t.items():
        assert bool((x == 1).all()), k
    assert bool((sh == 1).all()) and sdev.tolist() == [1, 1] and skp.tolist() == [0, 0]
    # accepted: no shadow, no table, no coefficient
    assert call(shadow=None) == 0 and call(skipped=None, norm_coef=None, hyper=None, step_dev=None, step=3) == 0
    torch.cuda.synchronize()
    assert sdev.tolist() == [2, 1] and skp.tolist() == [0, 0] and not bool((t["p"][:n] == 1).any()) and bool((t["p"][n:] == 1).all())


# ================================================================================================ 2. the step
def make(a, P, *, lr_mul=1.0, **runner_kw):
    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner
    m = TVTSv2Base(ARGS, arch=a)
    m.load_state_dict(P, strict=True)
    groups = [[], [], [], []]
    for name, p in m.named_parameters():
        gi = A.param_group_of(name, a)
        if gi < 0:
            p.requires_grad = False
        else:
            groups[gi].append(p)
    opt = FusedHFAdamW([dict(params=groups[i], lr=A.GROUP_HPARAMS[i][0] * lr_mul, weight_decay=A.GROUP_HPARAMS[i][1])
                        for i in range(4) if groups[i]], m.store, model=m)
    return m, opt, StepRunner(m, opt, **runner_kw)


def snapshot(m):
    st = m.store
    torch.cuda.synchronize()
    return {k: getattr(st, k).clone() for k in ("flat", "m", "v", "shadow", "shadow_t")}


def same_state(m, snap, what):
    cur = snapshot(m)
    for k in snap:
        same_bits(cur[k], snap[k], f"{what}: store.{k}")


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import arch as A
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    P = O.synth_params(oarch, seed=31)
    batches = [O.synth_batch(oarch, B=2, T=2, seed=40 + i, caption_len=8) for i in range(3)]
    return a, oarch, P, batches


def test_default_step_is_unchanged(K, tiny):
    a, oarch, P, batches = tiny
    m0, opt0, r0 = make(a, P)
    m1, opt1, r1 = make(a, P, clip_grad=None, skip_nonfinite=False)
    assert opt1.norm_coef is None and not r1.guarding and r1.clip_grad is None and r1.skip_nonfinite is False
    for b in batches:
        o0, o1 = r0.step(b), r1.step(b)
        assert list(o0) == list(o1) == ["loss1", "loss2"]
        same_bits(o0["loss1"], o1["loss1"], "loss1")
        same_bits(o0["loss2"], o1["loss2"], "loss2")
    same_state(m1, snapshot(m0), "explicit defaults against no arguments")
    assert opt0.global_step == opt1.global_step == 3 and int(opt1.skipped.item()) == 0


def test_clipped_step_against_the_composed_oracle(K, tiny):
    """Three steps, max_norm = 0.5 x the oracle's own unclipped norm of step 1.  Gates: parameters rel-L2 < 2e-2, the bound
    tests/test_model_gpu.py::test_training_curve_tracks_oracle applies to this architecture's parameters; grad_norm within 1 % of the
    oracle's total norm, the bound check_grads applies to the gradient norm there.  The UNCLIPPED step's margin against the same
    gates is printed beside the clipped one (pytest -s)."""
    a, oarch, P, batches = tiny
    Pu, Pc = {k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in P.items()}
    su, sc = {}, {}
    ref_u = [G.clipped_oracle_step(Pu, b, oarch, su) for b in batches]
    max_norm = 0.5 * ref_u[0]["norm"]
    ref_c = [G.clipped_oracle_step(Pc, b, oarch, sc, max_norm=max_norm) for b in batches]
    assert all(r["coef"] < 0.9 for r in ref_c), [r["coef"] for r in ref_c]   # clipping is active by construction
    mu, _, ru = make(a, P)
    mc, optc, rc = make(a, P, clip_grad=max_norm)
    norms = []
    for b in batches:
        ru.step(b)
        out = rc.step(b)
        assert list(out) == ["loss1", "loss2", "grad_norm"] and out["grad_norm"].is_cuda
        norms.append(float(out["grad_norm"]))
    keys = ("pred_model.head.weight", "video_model.transformer.resblocks.1.timeattn.proj.weight")
    mar_u = max(rel(mu.store.p(k), Pu[k]) for k in keys)
    mar_c = max(rel(mc.store.p(k), Pc[k]) for k in keys)
    mar_n = max(abs(n - r["norm"]) / r["norm"] for n, r in zip(norms, ref_c))
    print(f"   [margins] parameters rel-L2 (gate 2e-2): unclipped {mar_u:.3e}, clipped {mar_c:.3e}; grad_norm (gate 1e-2): {mar_n:.3e}; "
          f"oracle coefficients {[round(r['coef'], 4) for r in ref_c]}")
    assert mar_u < 2e-2 and mar_c < 2e-2, (mar_u, mar_c)
    assert mar_n < 1e-2, (norms, [r["norm"] for r in ref_c])
    # the coefficient reached the update: after step 1 |m| = (1 - b1) * coef * |g| = 0.1 * max_norm * norm / (norm + 1e-6), whatever
    # the gradient's own error is (fp32 roundings only: 1e-4 is generous) -- the unclipped first moment is twice as long
    mc1, _, rc1 = make(a, P, clip_grad=max_norm)
    mu1, _, ru1 = make(a, P)
    rc1.step(batches[0]); ru1.step(batches[0])
    live = (optc.chunk_group < 255).repeat_interleave(CH)
    got, n1 = float(mc1.store.m[live].double().norm()), float(rc1.norm_coef[0])
    want = 0.1 * max_norm * n1 / (n1 + 1e-6)
    assert abs(got - want) <= 1e-4 * want, (got, want)
    assert float(mu1.store.m[live].double().norm()) > 1.8 * got
    assert float(rc1.norm_coef[1]) < 0.9


def test_large_max_norm_is_the_unclipped_step(K, tiny):
    a, oarch, P, batches = tiny
    m0, opt0, r0 = make(a, P)
    m1, opt1, r1 = make(a, P, clip_grad=1e9)
    for b in batches[:2]:
        o0, o1 = r0.step(b), r1.step(b)
        same_bits(o0["loss1"], o1["loss1"], "loss1")
    assert float(r1.norm_coef[1]) == 1.0 and math.isfinite(float(o1["grad_norm"])) and float(o1["grad_norm"]) > 0
    same_state(m1, snapshot(m0), "max_norm 1e9 against the plain step")


def overflow_sequence(a, P, batches, bad_at, oarch):
    """three (or more) guarded steps, batch `bad_at` (0-based) with one NaN pixel -> what the tests look at"""
    m, opt, r = make(a, P, skip_nonfinite=True)
    seen = []
    for i, b in enumerate(batches):
        r.step(G.nan_pixel(b, oarch, sample=1) if i == bad_at else b)
        torch.cuda.synchronize()
        f8 = None if getattr(m.engine, "_f8_scale", None) is None else (m.engine._f8_scale.clone(), m.engine._f8_amax.clone())
        seen.append(dict(state=snapshot(m), skipped=int(r.skipped.item()), step_dev=int(opt.step_dev.item()), f8=f8,
                         norm=float(r.norm_coef[0]), grad=m.store.grad.clone()))
    return m, opt, r, seen


def test_overflow_sequence(K, tiny):
    a, oarch, P, batches = tiny
    m, opt, r, seen = overflow_sequence(a, P, batches, 1, oarch)
    assert [s["skipped"] for s in seen] == [0, 1, 1] and [s["step_dev"] for s in seen] == [1, 1, 2]
    assert math.isfinite(seen[0]["norm"]) and not math.isfinite(seen[1]["norm"]) and math.isfinite(seen[2]["norm"])
    for k in seen[0]["state"]:
        same_bits(seen[1]["state"][k], seen[0]["state"][k], f"after the bad step: every bit of store.{k} is the one after step 1")
    assert not bool(torch.isfinite(seen[1]["grad"]).all()) and bool(torch.isfinite(seen[2]["grad"]).all())  # zeroed as usual
    for k, t in seen[2]["state"].items():
        assert bool(torch.isfinite(t.float()).all()), k
    assert opt.state_dict()["state"][0]["step"] == 2 and opt.global_step == 2
    # the unguarded runner: step 1 on batch 1 gives the same state; from there batch 3 with step count 2 gives the guarded end state
    # (the unguarded runner reads its step count from the device as well: the guarded launch's code path)
    mu, optu, ru = make(a, P)
    ru.step(batches[0], device_step=True)
    same_state(mu, seen[0]["state"], "guarded step 1 against the unguarded step 1")
    ru.step(batches[2], device_step=True)
    assert optu.global_step == 2
    same_state(mu, seen[2]["state"], "guarded steps 1, (2), 3 against unguarded steps on batches 1 and 3")
    same_bits(mu.store.grad, seen[2]["grad"], "the gradient of step 3")
    # without the guard the NaN batch poisons the weights (the property the guard exists for)
    mp, _, rp = make(a, P)
    rp.step(batches[0]); rp.step(G.nan_pixel(batches[1], oarch, sample=1))
    assert not bool(torch.isfinite(mp.store.flat).all())


@pytest.fixture(scope="module")
def tiny_h():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import arch as A
    a = A.small_arch_h(width=640, heads=8, fp8_wgrad=True)
    oarch = O.tiny_arch(**a)
    P = O.synth_params(oarch, seed=33)
    batches = [O.synth_batch(oarch, B=2, T=2, seed=50 + i, caption_len=8) for i in range(4)]
    return a, oarch, P, batches


def test_overflow_behind_calibration_keeps_the_e4m3_scales(K, tiny_h):
    """small_h with e4m3 weight gradients, the bad step is step 3 (steps 1 calibrates, 2 runs per tensor): the skipped step changes
    no scale, and step 4 goes on from the state and the scales of step 2"""
    a, oarch, P, batches = tiny_h
    m, opt, r, seen = overflow_sequence(a, P, batches, 2, oarch)
    n = len(m.engine._f8_ids)
    assert n == 12 * oarch["layers"] and m.engine._f8_tensor_mode
    assert [s["skipped"] for s in seen] == [0, 0, 1, 1] and [s["step_dev"] for s in seen] == [1, 2, 2, 3]
    s2, s3 = seen[1]["f8"][0][:n], seen[2]["f8"][0][:n]
    assert bool(torch.isfinite(s3).all()) and bool((s3 > 0).all())
    same_bits(s3, s2, "the scales after the bad step are the scales before it")
    assert float(seen[2]["f8"][1].abs().max()) == 0.0  # the maxima of the bad step are gone
    for k in seen[1]["state"]:
        same_bits(seen[2]["state"][k], seen[1]["state"][k], f"after the bad step: store.{k}")
    for k, t in seen[3]["state"].items():
        assert bool(torch.isfinite(t.float()).all()), k
    s4 = seen[3]["f8"][0][:n]
    assert bool(torch.isfinite(s4).all()) and bool((s4 > 0).all()) and not torch.equal(s4, s3)
    # the finite steps are the unguarded runner's, bit for bit (the guarded scale update of a finite step is the plain update)
    mu, optu, ru = make(a, P)
    ru.step(batches[0], device_step=True); ru.step(batches[1], device_step=True)
    same_state(mu, seen[1]["state"], "guarded steps 1, 2 against the unguarded runner")
    same_bits(mu.engine._f8_scale[:n], s2, "scales after step 2")


def test_overflow_in_the_calibration_step(K, tiny_h):
    """the bad step is step 1: no slot has had a usable maximum, every one gets 1.0 (the stated rule) -- no zero, no non-finite
    scale remains -- and steps 2 and 3 are finite"""
    a, oarch, P, batches = tiny_h
    m, opt, r, seen = overflow_sequence(a, P, batches[:3], 0, oarch)
    n = len(m.engine._f8_ids)
    assert n == 12 * oarch["layers"]
    assert [s["skipped"] for s in seen] == [1, 1, 1] and [s["step_dev"] for s in seen] == [0, 1, 2]
    s1 = seen[0]["f8"][0][:n]
    assert s1.tolist() == [1.0] * n, s1.tolist()
    for s in seen[1:]:
        sc = s["f8"][0][:n]
        assert bool(torch.isfinite(sc).all()) and bool((sc > 0).all()) and math.isfinite(s["norm"])
    for k, t in seen[2]["state"].items():
        assert bool(torch.isfinite(t.float()).all()), k
    same_bits(seen[0]["state"]["flat"], make(a, P)[0].store.flat, "the skipped first step leaves the loaded weights")


def test_named_refusals(K, tiny):
    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.step import StepRunner
    a, oarch, P, batches = tiny
    for kw in (dict(clip_grad=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(RuntimeError, match="adamw_ranges / TVTS_ADAMW_RANGES=1"):
            make(A.small_arch(adamw_ranges=True), P, **kw)
        m = TVTSv2Base(ARGS, arch=a)
        m.load_state_dict(P, strict=True)
        with pytest.raises(RuntimeError, match="needs the fused optimizer .* got AdamW"):
            StepRunner(m, torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4), **kw)
    m, opt, r = make(a, P, clip_grad=1.0)
    with pytest.raises(RuntimeError, match="ranged updates .* gradient clipping"):
        opt.begin_ranges()
    m, opt, r = make(a, P)
    with pytest.raises(RuntimeError, match="ranged updates .* the overflow guard"):
        opt.begin_ranges(guard=True)
    with pytest.raises(RuntimeError, match="needs norm_coef"):
        opt.step(guard=True)
    make(A.small_arch(adamw_ranges=True), P)[2].step(batches[0])  # the ranged step without the options still runs


# ================================================================================================ 3. graph replay and the trainer
def test_graph_replay_with_clipping_is_the_eager_step(K, monkeypatch):
    """clip_grad only: the coefficient is a device scalar, the step stays capturable.  Five GraphReplay steps of one signature (first
    sight eager, the second captured and replayed, three more replays) against five eager steps: losses, grad_norm and the state bit
    for bit.  With skip_nonfinite GraphReplay captures nothing and steps eagerly."""
    from tvts_amd import arch as A
    from tvts_amd.step import GraphReplay
    monkeypatch.setenv("TVTS_TRAINER_GRAPH", "1")
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    P = O.synth_params(oarch, seed=21)
    batch = O.synth_batch(oarch, B=4, T=2, seed=22, caption_len=9)

    def five(replayed, **kw):
        m, opt, r = make(a, P, **kw)
        rep = GraphReplay(r)
        rows = []
        for _ in range(5):
            out = rep.step(batch) if replayed else r.step(batch, device_step=True)
            torch.cuda.synchronize()
            rows.append((bits(out["loss1"]).tolist(), bits(out["loss2"]).tolist(), bits(out["grad_norm"]).tolist(), float(out["grad_norm"])))
        return m, opt, rep, rows
    me, opte, _, rows_e = five(False, clip_grad=0.05)
    mg, optg, rep, rows_g = five(True, clip_grad=0.05)
    assert rep.usable and rep.captures == 1 and rep.replays == 4 and rep.eager == 1, vars(rep)
    assert rows_g == rows_e, (rows_g, rows_e)
    assert all(math.isfinite(r[3]) and r[3] > 0.05 for r in rows_e), rows_e  # (the clip is active in every step)
    same_state(mg, snapshot(me), "five replayed steps against five eager steps")
    assert optg.state_dict()["state"][0]["step"] == opte.state_dict()["state"][0]["step"] == 5
    ms, opts, rep_s, _ = five(True, clip_grad=0.05, skip_nonfinite=True)
    assert not rep_s.usable and rep_s.captures == 0 and rep_s.replays == 0 and rep_s.eager == 5
    assert opts.state_dict()["state"][0]["step"] == 5 and int(opts.skipped.item()) == 0
    same_bits(ms.store.flat, me.store.flat, "the guarded eager steps on finite data are the clipped steps")


def build_trainer(tmp_path, epochs, resume=None, keys=None, bad=None):
    """the trainer of tests/test_trainer_gpu.py::build (two alternating loaders, no validation) with extra config['trainer'] keys;
    bad: index of the YT batch that carries a NaN pixel"""
    from test_trainer_gpu import Config, Loader
    from tvts_amd import arch as A
    from tvts_amd.model import metric as M
    from tvts_amd.model.loss import NormSoftmaxLoss
    from tvts_amd.trainer.trainer import Trainer_TVTSv2_B_16
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    args = types.SimpleNamespace(local_rank=0, rank=0, world_size=1, schedule=[])
    yt = [O.synth_batch(oarch, B=4, T=2, seed=10 + i, caption_len=9) for i in range(3)]
    if bad is not None:
        yt[bad] = G.nan_pixel(yt[bad], oarch, sample=2)
    wv = [O.synth_batch(oarch, B=4, T=2, seed=20 + i, n_trans=1, caption_len=9) for i in range(2)]
    cfg = Config(str(tmp_path), epochs)
    cfg["trainer"].update(keys or {})
    cfg.resume = resume
    # (the optimizer exists before the trainer, as in the kept entry points: resume loads into it inside the constructor)
    m, opt, _ = make(a, O.synth_params(oarch, seed=1), lr_mul=30.0)
    tr = Trainer_TVTSv2_B_16(args, m, NormSoftmaxLoss(), [M.t2v_metrics, M.v2t_metrics], opt, config=cfg,
                             data_loader=[Loader(yt, "YTTemporal", 4), Loader(wv, "WebVid", 4)], valid_data_loader=None,
                             max_samples_per_epoch=10 ** 9)
    return tr, m


def grab_lines(tr, fn):
    lines = []

    class Grab(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    h = Grab(level=logging.DEBUG)
    old = tr.logger.level
    tr.logger.addHandler(h)
    tr.logger.setLevel(logging.DEBUG)
    try:
        fn()
    finally:
        tr.logger.removeHandler(h)
        tr.logger.setLevel(old)
    return lines


def test_trainer_config_keys(K, tmp_path):
    """config['trainer'] = {clip_grad, skip_nonfinite}: the lazy log lines carry grad_norm, the epoch summary and the checkpoint the
    skip count, and a resumed run continues bit for bit -- with one NaN batch per epoch in the way.  Without the keys: the log text
    and the checkpoint keys of the plain trainer."""
    keys = dict(clip_grad=0.5, skip_nonfinite=True)
    for d in ("a", "b", "p"):
        (tmp_path / d).mkdir()
    tr_a, m_a = build_trainer(tmp_path / "a", 2, keys=keys, bad=1)
    assert tr_a.runner.clip_grad == 0.5 and tr_a.runner.skip_nonfinite and not tr_a.replay.usable
    lines = grab_lines(tr_a, tr_a.train)
    steps = [ln for ln in lines if ln.startswith("Train Epoch")]
    assert len(steps) == 8 and all(" grad_norm: " in ln for ln in steps), steps   # 2 epochs x (batch_idx 0, 2) x 2 loaders
    for ln in steps:
        assert math.isfinite(float(ln.rsplit("grad_norm: ", 1)[1])) and ln.startswith(tr_a.LOG_LINE.split("{}")[0])
    assert [ln.split(":")[1].strip() for ln in lines if ln.strip().startswith("skipped")] == ["1", "2"], lines
    ck = torch.load(tmp_path / "a" / "checkpoint-epoch1.pth", map_location="cpu", weights_only=False)
    assert list(ck.keys()) == ["arch", "epoch", "state_dict", "optimizer", "monitor_best", "config", "tvts_amd"]
    assert ck["tvts_amd"] == {"skipped": 1} and ck["optimizer"]["state"][0]["step"] == 5   # 3 x 2 steps, one skipped
    ck2 = torch.load(tmp_path / "a" / "checkpoint-epoch2.pth", map_location="cpu", weights_only=False)
    assert ck2["tvts_amd"] == {"skipped": 2} and ck2["optimizer"]["state"][0]["step"] == 10
    assert bool(torch.isfinite(m_a.store.flat).all())
    # one epoch, a checkpoint, a rebuild with `resume`, the second epoch
    tr_b, m_b = build_trainer(tmp_path / "b", 1, keys=keys, bad=1)
    tr_b.train()
    tr_c, m_c = build_trainer(tmp_path / "b", 2, resume=tmp_path / "b" / "checkpoint-epoch1.pth", keys=keys, bad=1)
    assert tr_c.start_epoch == 2 and int(tr_c.runner.skipped.item()) == 1 and tr_c.optimizer.global_step == 5
    tr_c.train()
    assert int(tr_c.runner.skipped.item()) == 2
    same_state(m_c, snapshot(m_a), "the resumed run against the run in one go")
    # the same config without the keys: today's log text, today's checkpoint
    tr_p, m_p = build_trainer(tmp_path / "p", 1)
    assert not tr_p.runner.guarding
    plain = [ln for ln in grab_lines(tr_p, tr_p.train) if ln.startswith("Train Epoch")]
    assert len(plain) == 4 and not any("grad_norm" in ln for ln in plain)
    import re
    pat = re.compile(r"^Train Epoch: 1 dl[01] \[\d+/\d+ \(\d+%\)\] Loss_ct: \d+\.\d{6} Loss_ce: \d+\.\d{6} Loss: \d+\.\d{6}$")
    assert all(pat.match(ln) for ln in plain), plain
    ckp = torch.load(tmp_path / "p" / "checkpoint-epoch1.pth", map_location="cpu", weights_only=False)
    assert list(ckp.keys()) == ["arch", "epoch", "state_dict", "optimizer", "monitor_best", "config"]
