"""The v1 fine-tuning step (run with -m gpu): its five kernels per element against tests/v1_finetune_ref.py (float64 references
with derived bounds, the integer restatement of the draw, guarded buffers), the downstream class trained by
tvts_amd.downstream.finetune_v1.FinetuneStep against the run of the reference's own classes (tests/golden/v1_finetune.npz, masks
replayed through EngineV1.drop_path_override), the step's semantics (linear probing, gradient accumulation, dropped samples, the
seed rule, isolation from inference calls), a four-step curve against the fp32 helper, and one run at the real size.

Parameter deltas are compared through v1_finetune_ref.delta_for_compare, which leaves out the key third of attn.qkv.bias: its
gradient is identically zero in exact arithmetic, so its Adam step is normalised rounding noise in any implementation."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
import v1_downstream_synth as S  # noqa: E402
import v1_finetune_ref as R  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
U = KB.U32
F = R.FX
CH = 1024


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def guarded(rows, cols, dtype, pad=4, extra=2):
    """-> (view [rows, cols] with leading dimension cols + pad inside a NaN-filled buffer of rows + extra rows, the buffer)"""
    buf = torch.full((rows + extra, cols + pad), NAN, dtype=dtype, device=DEV)
    return buf[:rows, :cols], buf


def guards_intact(view, buf):
    rows, cols = view.shape
    assert torch.isnan(buf[:rows, cols:]).all() and torch.isnan(buf[rows:]).all(), "the kernel wrote outside its output"


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def min_cos(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float(torch.nn.functional.cosine_similarity(a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1), dim=1).min())


def u64_to_i64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


# ================================================================================================ 1. the draw
@pytest.mark.parametrize("B", [1, 3, 64, 65])
@pytest.mark.parametrize("nsites", [2, 24])
def test_drop_path_table_bits(K, B, nsites):
    rates = np.linspace(0.0, 0.6, nsites).astype(np.float32)
    rates[0] = 0.0
    p = torch.from_numpy(rates).to(DEV)
    for seed in (0x1234ABCD, 0xF00DFACE12345678):  # (the second has its top bit set: a negative int64 in device memory)
        sd = torch.tensor([u64_to_i64(seed)], dtype=torch.int64, device=DEV)
        buf = torch.full((nsites * B + 64,), NAN, dtype=F32, device=DEV)
        table = buf[:nsites * B].view(nsites, B)
        K.drop_path_table(sd, p, table, site_base=R.FT_SITE_BASE)
        want = R.draw_table(seed, rates, B)
        assert table.cpu().numpy().tobytes() == want.tobytes(), (hex(seed), table.cpu(), want)
        assert (table[0] == 1.0).all() and torch.isnan(buf[nsites * B:]).all()
        K.drop_path_table(sd, p, table, site_base=7)
        assert table.cpu().numpy().tobytes() == R.draw_table(seed, rates, B, site_base=7).tobytes()


# ================================================================================================ 2. residual + scale * branch
@pytest.mark.parametrize("outs", ["f32", "bf16", "both"])
@pytest.mark.parametrize("W", [128, 768])
@pytest.mark.parametrize("S_", [65, 1])
def test_drop_path_rows(K, S_, W, outs):
    """forward (residual) and backward (no residual): B = 3 with scales {0, 1, 1.25}; the dropped sample's y holds inf / NaN, which
    must not reach the output"""
    Bn = 3
    rows = Bn * S_
    scale = torch.tensor([0.0, 1.0, 1.25])
    y, res = rnd(rows, W, seed=11 + S_ + W), rnd(rows, W, seed=12 + S_ + W, scale=3.0)
    y[0, :4] = torch.tensor([float("inf"), -float("inf"), NAN, 1e38])
    res[0, 5] = -0.0
    yv, ybuf = guarded(rows, W, F32)
    rv, rbuf = guarded(rows, W, F32, pad=8)
    yv.copy_(y)
    rv.copy_(res)
    for residual in (rv, None):
        o32, b32 = guarded(rows, W, F32, pad=12) if outs in ("f32", "both") else (None, None)
        o16, b16 = guarded(rows, W, BF16, pad=8) if outs in ("bf16", "both") else (None, None)
        K.drop_path_rows(yv, scale.to(DEV), S_, residual=residual, out=o32, out_bf16=o16)
        w = R.drop_path_rows_check(y, scale, S_, res if residual is not None else None, None if o32 is None else o32.cpu(),
                                   None if o16 is None else o16.cpu(), f"drop_path_rows S={S_} W={W} {'fwd' if residual is not None else 'bwd'}")
        KB.bound_line(f"drop_path_rows S={S_} W={W} {outs}", w)
        for v, b in ((o32, b32), (o16, b16)):
            if v is not None:
                guards_intact(v, b)


# ================================================================================================ 3. soft-target cross entropy
@pytest.mark.parametrize("form", ["soft", "label", "smooth"])
@pytest.mark.parametrize("C", [1, 7, 174, 1025])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_soft_ce(K, B, C, form):
    """loss (added into a non-zero cell), dlogits and the hit count per element; a row of large logits (+-80), a row whose
    target mass sits on the argmax; with and without dlogits"""
    x = rnd(B, C, seed=100 + B + C, scale=2.0)
    x[0] = torch.where(torch.arange(C) % 2 == 0, 80.0, -80.0) + rnd(C, seed=5, scale=0.01)
    soft = labels = None
    eps = 0.0
    if form == "soft":
        soft = torch.softmax(rnd(B, C, seed=200 + B + C, scale=2.0), dim=1)
        soft[B - 1] = 0.1 / C
        soft[B - 1, int(x[B - 1].argmax())] += 0.9   # (the last row's target mass sits on its argmax: a hit)
    else:
        labels = torch.randint(0, C, (B,), generator=gen(300 + B + C))
        labels[B - 1] = int(x[B - 1].argmax())
        eps = 0.1 if form == "smooth" else 0.0
    scale, start = 0.5, 3.5
    loss, e_loss, dref, e_d, hits = R.soft_ce_ref(x, soft, labels, eps, scale)
    xv, xbuf = guarded(B, C, F32, pad=3)
    xv.copy_(x)
    tv = None
    if soft is not None:
        tv, _ = guarded(B, C, F32, pad=5)
        tv.copy_(soft)
    lab = None if labels is None else labels.to(torch.int32).to(DEV)
    ws = torch.full((2 * B + 8,), NAN, dtype=F32, device=DEV)
    results = []
    for with_d in (True, False):
        cell = torch.full((3,), NAN, dtype=F32, device=DEV)
        cell[1] = start
        hit = torch.full((3,), -7, dtype=torch.int32, device=DEV)
        dv, dbuf = guarded(B, C, F32, pad=3) if with_d else (None, None)
        K.soft_ce(xv, cell[1:2], ws, soft_targets=tv, labels=lab, smoothing=eps, scale=scale, dlogits=dv, hits=hit[1:2])
        got = float(cell[1]) - start
        assert abs(got - loss) <= e_loss + 2 * U * (start + abs(loss)), (got, loss, e_loss)
        assert int(hit[1]) == hits and int(hit[0]) == -7 and int(hit[2]) == -7 and torch.isnan(cell[0]) and torch.isnan(cell[2])
        assert hits >= 1 and torch.isnan(ws[2 * B:]).all()
        if with_d:
            w = KB.assert_within(dv.cpu(), dref, e_d, f"soft_ce {form} B={B} C={C}: dlogits")
            KB.bound_line(f"soft_ce {form} B={B} C={C} dlogits", w)
            guards_intact(dv, dbuf)
        results.append(cell[1].clone())
    assert torch.equal(results[0], results[1])  # the loss does not depend on whether dlogits is written


# ================================================================================================ 4. global norm + clip coefficient
@pytest.mark.parametrize("nchunks", [1, 6, 2500])
def test_grad_sumsq_and_coef(K, nchunks):
    """frozen chunks (group 255) in front, in the middle and at the end hold 1e30 and must not enter; clip off / not binding /
    binding; two runs give the same bits"""
    g = rnd(nchunks * CH, seed=400 + nchunks, scale=0.3)
    grp = torch.randint(0, 64, (nchunks,), generator=gen(401), dtype=torch.int64).to(torch.uint8)
    if nchunks > 1:
        for c in (0, nchunks // 2, nchunks - 1):
            grp[c] = 255
            g[c * CH:(c + 1) * CH] = 1e30
    gd, grpd = g.to(DEV), grp.to(DEV)
    norm0 = R.grad_norm_ref(g, grp, 0.0)[0]
    for max_norm, gs in ((0.0, 1.0), (2.0 * norm0, 1.0), (0.25 * norm0, 1.0), (0.1 * norm0, 0.5)):
        norm, e_n, coef, e_c = R.grad_norm_ref(g, grp, max_norm, gs)
        outs = []
        for _ in range(2):
            part = torch.full((nchunks + 4,), NAN, dtype=F32, device=DEV)
            nc = torch.full((4,), NAN, dtype=F32, device=DEV)
            K.grad_sumsq(gd, grpd, part, nc[1:3], max_norm=max_norm, grad_scale=gs)
            assert torch.isnan(part[nchunks:]).all() and torch.isnan(nc[0]) and torch.isnan(nc[3])
            outs.append((nc[1:3].clone(), part[:nchunks].clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        got_n, got_c = float(outs[0][0][0]), float(outs[0][0][1])
        assert abs(got_n - norm) <= e_n, (got_n, norm, e_n)
        assert abs(got_c - coef) <= e_c, (got_c, coef, e_c)
        assert (got_c == 1.0) == (max_norm <= 0 or max_norm >= norm)
        KB.bound_line(f"grad_sumsq nchunks={nchunks} max_norm={max_norm:.3g}", abs(got_n - norm) / e_n)


# ================================================================================================ 5. torch.optim.AdamW, multi-tensor
GROUPS = [0, 1, 40, 63, 255, 1]
LR = {0: 1e-2, 1: 3e-3, 40: 1e-4, 63: 1e-3}
WD = {0: 0.05, 1: 0.0, 40: 0.01, 63: 0.3}


def adam_state(seed):
    """fp32 p, g, m, v over six 1024-element chunks (the construction of test_adamw_per_element); chunk 0 carries the special
    elements: g = m = v = 0 (0..7), |g| = 1e-12 (8..15, m = v = 0), |p| = 1e4 (16)"""
    n = CH * len(GROUPS)
    p, g = rnd(n, seed=seed), rnd(n, seed=seed + 1, scale=0.1)
    m, v = rnd(n, seed=seed + 2, scale=0.05), torch.rand(n, generator=gen(seed + 3)) * 1e-2
    g[:8], m[:16], v[:16] = 0.0, 0.0, 0.0
    g[8:16] = torch.tensor([1e-12, -1e-12] * 4)
    p[16] = -1e4
    return p, g, m, v


def hyper_table():
    h = torch.full((128,), 7.0)  # (groups nobody uses hold a value that would show)
    for gi in LR:
        h[gi], h[64 + gi] = LR[gi], WD[gi]
    return h


def adam_run(K, state, step, *, step_dev=None, coef=None, grad_scale=0.5):
    p, g, m, v = (t.to(DEV).clone() for t in state)
    sh = torch.full((p.numel(),), -3.0, dtype=BF16, device=DEV)
    nc = None if coef is None else torch.tensor([123.0, coef], dtype=F32, device=DEV)
    K.adamw_torch(p, g, m, v, sh, torch.tensor(GROUPS, dtype=torch.uint8, device=DEV), hyper_table().to(DEV), step,
                  grad_scale=grad_scale, step_dev=step_dev, norm_coef=nc)
    return p.cpu(), m.cpu(), v.cpu(), sh.cpu()


@pytest.mark.parametrize("coef", [None, 0.37])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adamw_torch_per_element(K, step, coef):
    st = adam_state(seed=1300)
    p1, m1, v1, sh = adam_run(K, st, step, coef=coef)
    b = adam_run(K, st, 0, step_dev=torch.tensor([step], dtype=torch.int32, device=DEV), coef=coef)
    for nm, x, y in zip(("p", "m", "v", "shadow"), (p1, m1, v1, sh), b):
        KB.assert_equal_bits(x, y, f"adamw_torch host step vs device step {step}: {nm}")
    f32 = KB.f32_const
    gs = f32(0.5) if coef is None else f32(f32(0.5) * f32(coef))
    worst = 0.0
    for ci, grp in enumerate(GROUPS):
        sl = slice(ci * CH, (ci + 1) * CH)
        if grp == 255:
            for nm, got, was in (("p", p1, st[0]), ("m", m1, st[2]), ("v", v1, st[3])):
                KB.assert_equal_bits(got[sl], was[sl], f"adamw_torch group 255: {nm} must stay")
            KB.assert_equal_bits(sh[sl], torch.full((CH,), -3.0, dtype=BF16), "adamw_torch group 255: shadow must stay")
            continue
        kw = dict(lr=LR[grp], wd=WD[grp], step=step, grad_scale=0.5, coef=coef)
        worst = max(worst, R.adamw_torch_check(st[0][sl], st[1][sl], st[2][sl], st[3][sl], p1[sl], m1[sl], v1[sl], sh[sl],
                                               what=f"adamw_torch step {step} group {grp}", **kw))
        # one fp32 torch.optim.AdamW step on the CPU over the same tensors, inside the same bound
        tp = st[0][sl].clone().requires_grad_(True)
        tp.grad = st[1][sl] * gs
        opt = torch.optim.AdamW([tp], lr=f32(LR[grp]), betas=(0.9, 0.999), eps=1e-8, weight_decay=f32(WD[grp]), foreach=False)
        opt.state[tp] = dict(step=torch.tensor(float(step - 1)), exp_avg=st[2][sl].clone(), exp_avg_sq=st[3][sl].clone())
        opt.step()
        s = opt.state[tp]
        R.adamw_torch_check(st[0][sl], st[1][sl], st[2][sl], st[3][sl], tp.detach(), s["exp_avg"], s["exp_avg_sq"], None,
                            what=f"torch.optim.AdamW step {step} group {grp}", **kw)
    KB.bound_line(f"adamw_torch step={step} coef={coef}", worst)


# ================================================================================================ 6. the model against the reference's run
def build(kw=S.TINY, classes=F["classes"], rate=F["drop_path_rate"], sd=None):
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    m = VisionTransformer(num_classes=classes, drop_path_rate=rate, **kw)
    m.load_state_dict(R.state(kw, F["seed"], classes) if sd is None else sd, strict=True)
    return m


def stepper(m, trainable="all", clip_grad=None, update_freq=1, smoothing=0.0):
    from tvts_amd.downstream.finetune_v1 import FinetuneStep, FusedTorchAdamW, param_groups
    groups = param_groups(m, F["weight_decay"], F["layer_decay"], trainable=trainable)
    opt = FusedTorchAdamW(groups, m.store, lr=F["lr"], model=m)
    for g in opt.param_groups:
        g["lr"] = F["lr"] * g["lr_scale"]
    return FinetuneStep(m, opt, clip_grad=clip_grad, update_freq=update_freq, smoothing=smoothing, trainable=trainable), opt


def fwd_bwd(K, m, clip, targets, trainable="all", scale=1.0, zero=True):
    """one forward / loss / backward through the engine, the gradients left in the store -> (logits, loss)"""
    eng = m.engine
    m.set_trainable(trainable)
    m._fresh_shadows()
    if zero:
        K.zero_(m.store.grad)
    B, T = clip.shape[0], clip.shape[2]
    logits = eng.finetune_forward(clip.to(DEV), B, T // 2)
    cell = torch.zeros(1, dtype=F32, device=DEV)
    dl, ws = torch.empty_like(logits), torch.empty(2 * B, dtype=F32, device=DEV)
    K.soft_ce(logits, cell, ws, soft_targets=targets.to(DEV), scale=scale, dlogits=dl)
    eng.finetune_backward(dl, trainable)
    torch.cuda.synchronize()
    return logits.clone(), float(cell)


def store_grads(m):
    return {n: g.detach().clone() for n, g in m.grad_views().items()}


def by_store_name(m, d):
    return {m.store_name(n): v for n, v in d.items()}


@pytest.fixture(scope="module")
def fx(golden):
    """the fixture and the fp32 helper's run over its masks, computed once and shared"""
    f = golden("v1_finetune")
    sd = R.state()
    clip, targets = S.synth_clip(S.TINY, F["B"], F["T"], F["clip_seed"]), R.soft_targets(F["B"], F["classes"], F["target_seed"])
    tables = [torch.from_numpy(t) for t in f["tables"]]
    steps, final = R.train_run(sd, clip, targets, tables, clip_grad=float(f["clip_grad"]))
    return dict(f=f, sd=sd, clip=clip, targets=targets, tables=tables, steps=steps, final=final)


def logits_gate(got, ref, what):
    e, c = rel(got, ref), min_cos(got, ref)
    print(f"\n   [{what}] logits: rel {e:.3e}, worst-clip cosine {c:.7f}")
    assert e < 0.02 and c > 0.9995, (what, e, c)


def test_model_gradients_against_reference_run(K, fx):
    from test_v1_gpu import check_grads
    m = build()
    m.engine.drop_path_override = fx["tables"][0].to(DEV)
    logits, loss = fwd_bwd(K, m, fx["clip"], fx["targets"])
    f = fx["f"]
    logits_gate(logits, f["logits"][0], "step 1 masks")
    dmax = float(np.abs(logits.cpu().numpy() - f["logits"][0]).max())
    assert abs(loss - f["loss"][0]) <= 2 * dmax, (loss, f["loss"][0], dmax)  # soft-target CE is 2-Lipschitz in the sup norm
    check_grads(m.store, by_store_name(m, fx["steps"][0]["grads"]))
    for n in R.FULL_GRADS:  # the tensors the fixture stores in full, against the reference's own numbers
        c = float(torch.nn.functional.cosine_similarity(m.grad_views()[n].cpu().double().flatten(),
                                                        torch.from_numpy(f["grad." + n]).double().flatten(), dim=0))
        assert c > 0.985, (n, c)


def test_model_two_steps_against_reference_run(K, fx):
    f = fx["f"]
    m = build()
    step, opt = stepper(m, clip_grad=float(f["clip_grad"]))
    assert len(opt.param_groups) == len(f["all_names"])
    for k in range(2):
        m.engine.drop_path_override = fx["tables"][k].to(DEV)
        out = step.step(fx["clip"], fx["targets"])
        logits_gate(out["logits"], f["logits"][k], f"step {k + 1}")
        dmax = float(np.abs(out["logits"].cpu().numpy() - f["logits"][k]).max())
        assert abs(float(out["loss"]) - f["loss"][k]) <= 2 * dmax, (k, float(out["loss"]), f["loss"][k], dmax)
        gn = float(out["grad_norm"])
        print(f"   step {k + 1}: grad norm {gn:.5f} (reference {f['grad_norm'][k]:.5f})")
        assert abs(gn - f["grad_norm"][k]) < 0.01 * f["grad_norm"][k], (k, gn, f["grad_norm"][k])
        assert not bool(m.store.grad.any())  # zeroed behind the update
    names = [str(s) for s in f["param_names"]]
    after = {n: p.detach().cpu() for n, p in m.named_parameters()}
    worst = []
    for i, n in enumerate(names):
        mine = R.delta_for_compare(n, (after[n].double() - fx["sd"][n].double()).flatten())
        ref = R.delta_for_compare(n, (fx["final"][n].double() - fx["sd"][n].double()).flatten())
        c = float(torch.nn.functional.cosine_similarity(mine, ref, dim=0))
        worst.append((c, n, float(mine.norm()), f["delta_norms"][i]))
    worst.sort()
    print("   parameter deltas, worst tensors (cosine, name, norm, reference norm):", worst[:4])
    for c, n, nm, nr in worst:
        assert abs(nm - nr) < 0.01 * nr, (n, nm, nr)
    assert worst[0][0] > 0.985, worst[:6]


# ================================================================================================ 7. semantics
def test_rate_zero_logits_and_bit_reproducible_gradients(K, fx):
    m = build(rate=0.0)
    logits, _ = fwd_bwd(K, m, fx["clip"], fx["targets"])
    assert m.engine.ft_ctx["drop_path"] is None
    logits_gate(logits, R.logits_of(fx["sd"], fx["clip"], S.TINY, None), "drop_path_rate 0")
    m2 = build()
    runs = []
    for _ in range(2):
        m2.engine.set_drop_seed_base(F["drop_seed"])
        fwd_bwd(K, m2, fx["clip"], fx["targets"])
        runs.append((m2.store.grad.clone(), m2.engine.buf["ft.dp_table"].clone()))
    assert torch.equal(runs[0][1], runs[1][1]) and (runs[0][1] == 0).any()
    KB.assert_equal_bits(runs[0][0], runs[1][0], "two identical steps: the flat gradient buffer")


def test_linear_probe_touches_only_the_head(K, fx):
    m = build()
    m.engine.drop_path_override = fx["tables"][0].to(DEV)
    fwd_bwd(K, m, fx["clip"], fx["targets"], trainable="all")
    g_all = store_grads(m)
    fwd_bwd(K, m, fx["clip"], fx["targets"], trainable="head")
    g_head = store_grads(m)
    for n in g_all:
        if n.startswith("head."):
            KB.assert_equal_bits(g_head[n], g_all[n], f"linear probe: gradient of {n}")
            assert bool(g_head[n].any())
        else:
            assert not bool(g_head[n].any()), n
    K.zero_(m.store.grad)
    step, opt = stepper(m, trainable="head")
    assert [g["name"] for g in opt.param_groups] == [str(s) for s in fx["f"]["head_names"]]
    st = m.store
    before = [t.clone() for t in (st.flat, st.m, st.v, st.shadow, st.shadow_t)]
    step.step(fx["clip"], fx["targets"])
    torch.cuda.synchronize()
    lo = st.off["head.weight"]
    for nm, was, now in zip(("parameters", "exp_avg", "exp_avg_sq", "bf16 shadow"), before, (st.flat, st.m, st.v, st.shadow)):
        KB.assert_equal_bits(now[:lo], was[:lo], f"linear probe: {nm} of the tower")
        assert not torch.equal(now[lo:], was[lo:]), nm
    KB.assert_equal_bits(st.shadow_t, before[4], "linear probe: transposed shadows")


def test_update_freq_two_half_batches(K):
    from test_v1_gpu import check_grads
    B, C = 4, F["classes"]
    clip, targets = S.synth_clip(S.TINY, B, F["T"], 71), R.soft_targets(B, C, 72)
    m = build(rate=0.0)
    fwd_bwd(K, m, clip, targets)
    full = {m.store_name(n): g.cpu() for n, g in store_grads(m).items()}
    fwd_bwd(K, m, clip[:2], targets[:2], scale=0.5)
    fwd_bwd(K, m, clip[2:], targets[2:], scale=0.5, zero=False)
    check_grads(m.store, full)
    # the step object: the first of two calls only accumulates
    K.zero_(m.store.grad)
    step, _ = stepper(m, update_freq=2)
    p0 = m.store.flat.clone()
    o1 = step.step(clip[:2], targets[:2])
    assert o1["grad_norm"] is None and torch.equal(m.store.flat, p0) and bool(m.store.grad.any())
    o2 = step.step(clip[2:], targets[2:])
    gn_full = math.sqrt(sum(float(g.double().norm()) ** 2 for g in full.values()))
    assert abs(float(o2["grad_norm"]) - gn_full) < 0.01 * gn_full and not torch.equal(m.store.flat, p0)
    assert not bool(m.store.grad.any())


def test_sample_dropped_everywhere_keeps_only_the_residual_path(K, fx):
    m = build()
    table = torch.ones(4, F["B"])
    table[:, 1] = 0.0
    table[2:, 0] = 1.25
    m.engine.drop_path_override = table.to(DEV)
    fwd_bwd(K, m, fx["clip"], fx["targets"])
    Sq = m.engine.ft_ctx["S"]
    dA, dB = m.engine.buf["ft.dxA"], m.engine.buf["ft.dxB"]  # gradients of the inputs of block 0 / block 1 (Engine._ab)
    rows = slice(Sq, 2 * Sq)
    assert bool(dB[Sq].any()) and not bool(dB[Sq + 1:2 * Sq].any())  # only the CLS row carries a gradient: norm + head
    assert torch.equal(dA[rows], dB[rows])                          # block 0 adds nothing for this sample
    assert bool(dB[1:Sq].any()) and not torch.equal(dA[:Sq], dB[:Sq])  # a kept sample's branches do


def test_seed_advances_once_per_step_and_resumes(K, fx):
    m = build()
    eng = m.engine
    eng.set_drop_seed_base(F["drop_seed"])
    rates = R.site_rates(F["drop_path_rate"], S.TINY["depth"])
    step, _ = stepper(m)
    tabs, bases = [], []
    for k in range(1, 4):
        bases.append(eng.drop_seed_base())
        step.step(fx["clip"], fx["targets"])
        tabs.append(eng.buf["ft.dp_table"].cpu().clone())
        assert eng.drop_seed_base() == R.step_seed(F["drop_seed"], k)
        assert tabs[-1].numpy().tobytes() == R.draw_table(R.step_seed(F["drop_seed"], k), rates, F["B"]).tobytes()
    eng.set_drop_seed_base(bases[2])  # a checkpoint taken in front of the third step
    step.step(fx["clip"], fx["targets"])
    assert torch.equal(eng.buf["ft.dp_table"].cpu(), tabs[2])
    assert tabs[0].numpy().tobytes() == fx["f"]["tables"][0].tobytes()  # (the fixture's masks are this seed's draw)


def test_unsynced_hyper_table_is_refused_under_capture(K, monkeypatch):
    """as FusedHFAdamW: a device-step launch on a capturing stream cannot upload lr / weight_decay, so param_groups changed after
    sync_hyper() are refused.  No graph is built: only the host-side check of _begin() runs, the capture query patched"""
    _, opt = stepper(build())
    opt.sync_hyper()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    opt._begin(True)  # the table matches param_groups: accepted
    opt.param_groups[0]["lr"] *= 0.5
    with pytest.raises(RuntimeError, match="FusedTorchAdamW: call sync_hyper"):
        opt._begin(True)
    assert opt.global_step == 1 and int(opt.step_dev.item()) == 1  # (the refusal came before the counters moved)


def test_inference_between_steps_changes_nothing(K, fx):
    a, b = build(), build()
    sa, _ = stepper(a)
    sb, _ = stepper(b)
    for m in (a, b):
        m.engine.set_drop_seed_base(F["drop_seed"])
    before = b(fx["clip"]).clone()
    sa.step(fx["clip"], fx["targets"])
    sb.step(fx["clip"], fx["targets"])
    seen = b(fx["clip"]).clone()                      # an inference forward between two steps
    b.forward_features(fx["clip"][:2])
    sa.step(fx["clip"], fx["targets"])
    sb.step(fx["clip"], fx["targets"])
    KB.assert_equal_bits(b.store.flat, a.store.flat, "parameters after two steps, with / without inference calls between")
    KB.assert_equal_bits(b.store.m, a.store.m, "exp_avg")
    assert not torch.equal(seen, before)              # the first forward after a step sees the updated weights
    a1 = build()
    s1, _ = stepper(a1)
    a1.engine.set_drop_seed_base(F["drop_seed"])
    s1.step(fx["clip"], fx["targets"])
    fresh = build(sd={k: v.detach().cpu() for k, v in a1.state_dict().items()})
    KB.assert_equal_bits(seen, fresh(fx["clip"]), "forward after a step vs a fresh model holding the updated parameters")


def test_uint8_frames_are_the_fp32_path_bit_for_bit(K, fx):
    """FinetuneStep on uint8 frames [B, T, H0, W0, 3] (centre crop + normalisation on the device) against the same step on the
    host-normalised fp32 clip: logits, loss and every updated parameter"""
    B, T, img, H0, W0 = 3, 8, S.TINY["img_size"], S.TINY["img_size"] + 3, S.TINY["img_size"] + 6  # crop offsets 2 and 3
    frames = torch.randint(0, 256, (B, T, H0, W0, 3), generator=gen(91), dtype=torch.uint8)
    mean, std = torch.tensor((0.485, 0.456, 0.406)).view(1, 1, 1, 1, 3), torch.tensor((0.229, 0.224, 0.225)).view(1, 1, 1, 1, 3)
    clip = ((frames[:, :, 2:2 + img, 3:3 + img].float() / 255 - mean) / std).permute(0, 4, 1, 2, 3).contiguous()  # [B, 3, T, H, W]
    labels = torch.tensor([0, 3, 6])
    res = []
    for x in (frames, clip):
        m = build()
        m.engine.set_drop_seed_base(F["drop_seed"])
        step, _ = stepper(m, smoothing=0.1)
        out = step.step(x, labels)
        res.append((out["logits"], out["loss"].reshape(1), m.store.flat.clone(), out["class_acc"].reshape(1)))
    for nm, a, b in zip(("logits", "loss", "parameters", "class_acc"), *res):
        KB.assert_equal_bits(a, b, f"uint8 frames vs fp32 clip: {nm}")
    acc = float(res[0][3])
    want = float((res[0][0].argmax(dim=1).cpu() == labels).float().mean())
    assert acc == want, (acc, want)


# ================================================================================================ 8. curve
def test_finetune_curve_tracks_helper(K, fx):
    """four steps with drawn masks; the fp32 helper replays the tables read back from the device"""
    m = build()
    m.engine.set_drop_seed_base(F["drop_seed"] + 5)
    step, _ = stepper(m, clip_grad=float(fx["f"]["clip_grad"]))
    curve, tables = [], []
    for _ in range(4):
        out = step.step(fx["clip"], fx["targets"])
        curve.append(float(out["loss"]))
        tables.append(m.engine.buf["ft.dp_table"].cpu().clone())
    steps, _ = R.train_run(fx["sd"], fx["clip"], fx["targets"], tables, clip_grad=float(fx["f"]["clip_grad"]))
    curve, ref = np.array(curve), np.array([s["loss"] for s in steps])
    print("\n   curve", curve, "helper", ref)
    assert ref[-1] < ref[0] - 0.02, ref
    assert np.all(np.abs(curve - ref) < 0.02 * np.abs(ref) + 1e-2), (curve, ref)


# ================================================================================================ 9. the real size, once
def test_full_size_step(K):
    """ViT-B/16, 16 frames, C = 174, B = 2 (S = 1569): finite loss, a non-zero finite gradient in every trainable tensor, the
    device's grad norm against a float64 recomputation from the store (bound of v1_finetune_ref.grad_norm_ref)"""
    from tvts_amd.downstream.finetune_v1 import FusedTorchAdamW, param_groups
    B, C = 2, 174
    m = build(S.REAL, classes=C, rate=0.1, sd=S.synth_state(S.REAL, 81, C))
    clip = S.synth_clip(S.REAL, B, 16, 82)
    targets = R.soft_targets(B, C, 83)
    m.engine.set_drop_seed_base(F["drop_seed"])
    logits, loss = fwd_bwd(K, m, clip, targets)
    assert math.isfinite(loss) and torch.isfinite(logits).all() and m.engine.ft_ctx["S"] == 1569
    for n, g in m.grad_views().items():
        assert torch.isfinite(g).all() and bool(g.any()), n
    groups = param_groups(m, 0.05, 0.75)
    assert len(groups) == 28
    opt = FusedTorchAdamW(groups, m.store, lr=1e-3, model=m)
    part = torch.empty(opt.chunk_group.numel(), dtype=F32, device=DEV)
    nc = torch.empty(2, dtype=F32, device=DEV)
    K.grad_sumsq(m.store.grad, opt.chunk_group, part, nc, max_norm=1.0)
    ref = math.sqrt(sum(float((g.double() ** 2).sum()) for g in m.grad_views().values()))
    assert abs(float(nc[0]) - ref) <= 9 * U * ref * 1.01, (float(nc[0]), ref)
    p0 = m.store.flat.clone()
    opt.norm_coef = nc
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(m.store.flat).all() and not torch.equal(m.store.flat, p0)
    assert torch.isfinite(m(clip)).all()
