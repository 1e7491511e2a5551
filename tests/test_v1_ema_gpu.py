"""ModelEma on the GPU (run with -m gpu): tvts_ema_update, tvts_adamw_torch with ema and tvts_swap_f32_shadow per element, and the
class inside FinetuneStep -- everything bit equality against tests/v1_ema_ref.py (the numpy restatement of timm's rule, held to
torch on the CPU by tests/test_v1_ema_cpu.py), a twin step without an average, or the state before.  Kernel tests: six chunks with
the group bytes and the state construction of test_adamw_torch_per_element.  Step tests: tests/v1_downstream_synth.TINY, 7 classes,
the constants of tests/v1_finetune_ref.FX, B = 3, T = 8."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
import v1_downstream_synth as S  # noqa: E402
import v1_ema_ref as E  # noqa: E402
import v1_finetune_ref as R  # noqa: E402
from test_v1_finetune_gpu import GROUPS, adam_state, hyper_table  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
F = R.FX
CH = 1024
GUARD = 1024  # elements of NaN in front of and behind every guarded buffer (a multiple of 4: the view stays 16-byte aligned)
DECAY = 0.9999


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def guarded(t):
    """host tensor -> (device view holding it, the NaN-filled buffer around it)"""
    buf = torch.full((t.numel() + 2 * GUARD,), NAN, dtype=t.dtype, device=DEV)
    v = buf[GUARD:GUARD + t.numel()]
    v.copy_(t)
    return v, buf


def intact(buf, what):
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), f"{what}: the kernel wrote outside its buffer"


def np_bits_equal(got, want, what):
    """got: fp32 tensor, want: fp32 numpy array -> bit equality with the first differing element named"""
    KB.assert_equal_bits(got.detach().cpu().reshape(-1), torch.from_numpy(np.ascontiguousarray(want)).reshape(-1), what)


def ema_state(seed):
    """p of adam_state and an average beside it; chunk 0 (group 0, it steps) carries the special elements: +-0 in every
    combination, 3e38 of both signs, e == p"""
    p = adam_state(seed)[0].clone()
    e = torch.randn(p.numel(), generator=torch.Generator().manual_seed(seed + 7))
    e[:8] = torch.tensor([0.0, -0.0, 0.0, -0.0, 3e38, -3e38, 3e38, -3e38])
    p[:8] = torch.tensor([0.0, -0.0, -0.0, 0.0, 3e38, -3e38, -3e38, 1.0])
    e[8:16] = p[8:16]
    return e, p


def groups_dev():
    return torch.tensor(GROUPS, dtype=torch.uint8, device=DEV)


# ================================================================================================ 1. the kernels
@pytest.mark.parametrize("decay", [0.9999, 0.5])
def test_ema_update_per_element(K, decay):
    e, p = ema_state(1300)
    ev, ebuf = guarded(e)
    pv, pbuf = guarded(p)
    K.ema_update(ev, pv, groups_dev(), decay)
    want = E.ema_ref_chunks(e.numpy(), p.numpy(), GROUPS, decay)
    np_bits_equal(ev, want, f"ema_update decay {decay}")
    for ci, grp in enumerate(GROUPS):
        sl = slice(ci * CH, (ci + 1) * CH)
        if grp == 255:
            KB.assert_equal_bits(ev[sl].cpu(), e[sl], "ema_update group 255: the average must stay")
        else:
            assert not torch.equal(ev[sl].cpu(), e[sl]), ci
    KB.assert_equal_bits(pv.cpu(), p, "ema_update: p must stay")
    intact(ebuf, "ema")
    intact(pbuf, "p")
    # a second pass feeds the average back
    K.ema_update(ev, pv, groups_dev(), decay)
    np_bits_equal(ev, E.ema_ref_chunks(want, p.numpy(), GROUPS, decay), f"ema_update decay {decay}, second pass")


def adam_run(K, state, step, *, device_step, coef, ema=None):
    p, g, m, v = (t.to(DEV).clone() for t in state)
    sh = torch.full((p.numel(),), -3.0, dtype=BF16, device=DEV)
    nc = None if coef is None else torch.tensor([123.0, coef], dtype=F32, device=DEV)
    sd = torch.tensor([step], dtype=torch.int32, device=DEV) if device_step else None
    kw = {} if ema is None else dict(ema=ema, ema_decay=DECAY)
    K.adamw_torch(p, g, m, v, sh, groups_dev(), hyper_table().to(DEV), 0 if device_step else step, grad_scale=0.5, step_dev=sd,
                  norm_coef=nc, **kw)
    return p, m, v, sh


@pytest.mark.parametrize("coef", [None, 0.37])
@pytest.mark.parametrize("device_step", [False, True])
@pytest.mark.parametrize("step", [1, 1000])
def test_fused_launch_is_the_plain_launch_plus_the_separate_pass(K, step, device_step, coef):
    st = adam_state(seed=1300)
    e, _ = ema_state(1300)
    plain = adam_run(K, st, step, device_step=device_step, coef=coef)
    ev, ebuf = guarded(e)
    fused = adam_run(K, st, step, device_step=device_step, coef=coef, ema=ev)
    for nm, x, y in zip(("p", "m", "v", "shadow"), fused, plain):
        KB.assert_equal_bits(x, y, f"adamw_torch with an average against the launch without, step {step}: {nm}")
    assert not torch.equal(plain[0].cpu(), st[0])
    sep = e.to(DEV).clone()
    K.ema_update(sep, plain[0], groups_dev(), DECAY)
    KB.assert_equal_bits(ev, sep, f"the fused average against ema_update behind the plain launch, step {step}")
    np_bits_equal(ev, E.ema_ref_chunks(e.numpy(), plain[0].cpu().numpy(), GROUPS, DECAY), "the fused average against the restatement")
    c255 = GROUPS.index(255)
    KB.assert_equal_bits(ev[c255 * CH:(c255 + 1) * CH].cpu(), e[c255 * CH:(c255 + 1) * CH], "group 255: the average must stay")
    assert not torch.equal(ev[:CH].cpu(), e[:CH])
    intact(ebuf, "ema")


@pytest.mark.parametrize("n", [1024, 4])
def test_swap_f32_shadow(K, n):
    g = torch.Generator().manual_seed(50 + n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-3
    a[:4] = torch.tensor([0.0, -0.0, 3e38, float("inf")])
    b[:4] = torch.tensor([-0.0, 1e-30, -3e38, 1.0])
    av, abuf = guarded(a)
    bv, bbuf = guarded(b)
    sv, sbuf = guarded(torch.full((n,), -3.0, dtype=BF16))
    K.swap_f32_shadow(av, bv, sv)
    KB.assert_equal_bits(av.cpu(), b, "swap: a holds b")
    KB.assert_equal_bits(bv.cpu(), a, "swap: b holds a")
    KB.assert_equal_bits(sv.cpu(), b.to(BF16), "swap: the shadow is bf16(new a)")
    K.swap_f32_shadow(av, bv, sv)
    KB.assert_equal_bits(av.cpu(), a, "second swap: a restored")
    KB.assert_equal_bits(bv.cpu(), b, "second swap: b restored")
    KB.assert_equal_bits(sv.cpu(), a.to(BF16), "second swap: the shadow is bf16(a)")
    for buf, nm in ((abuf, "a"), (bbuf, "b"), (sbuf, "shadow")):
        intact(buf, nm)


def test_refusals_launch_nothing(K):
    """misaligned pointers, a length that is no multiple of 4, overlapping buffers, an average without a decay: refused on the host"""
    n = 2 * CH
    buf = torch.zeros(n + 8, dtype=F32, device=DEV)
    other = torch.ones(n + 8, dtype=F32, device=DEV)
    sh = torch.zeros(n + 8, dtype=BF16, device=DEV)
    grp = torch.zeros(2, dtype=torch.uint8, device=DEV)
    with pytest.raises(K.HipError):
        K.ema_update(buf[1:1 + n], other[:n], grp, DECAY)
    with pytest.raises(K.HipError):
        K.ema_update(buf[:n], other[2:2 + n], grp, DECAY)
    with pytest.raises(K.HipError):
        K.swap_f32_shadow(buf[:6], other[:6], sh[:6])
    with pytest.raises(K.HipError):
        K.swap_f32_shadow(buf[1:5], other[:4], sh[:4])
    with pytest.raises(K.HipError):
        K.swap_f32_shadow(buf[:8], buf[4:12], sh[:8])
    st = [t.to(DEV) for t in adam_state(1300)]
    with pytest.raises(ValueError):
        K.adamw_torch(*st, None, groups_dev(), hyper_table().to(DEV), 1, ema=torch.zeros_like(st[0]))
    with pytest.raises(K.HipError):
        K.adamw_torch(*st, None, groups_dev(), hyper_table().to(DEV), 1, ema=torch.zeros(st[0].numel() + 4, device=DEV)[1:], ema_decay=DECAY)
    torch.cuda.synchronize()
    assert not bool(buf.any()) and bool((other == 1).all())
    for t, was in zip(st, adam_state(1300)):
        KB.assert_equal_bits(t.cpu(), was, "a refused launch changed its operands")


# ================================================================================================ 2. the step
def build(rate=F["drop_path_rate"], sd=None):
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    m = VisionTransformer(num_classes=F["classes"], drop_path_rate=rate, **S.TINY)
    m.load_state_dict(R.state(S.TINY, F["seed"], F["classes"]) if sd is None else sd, strict=True)
    m.engine.set_drop_seed_base(F["drop_seed"])
    return m


def make(m, *, with_ema, trainable="all", update_freq=1, decay=DECAY):
    from tvts_amd.downstream.finetune_v1 import FinetuneStep, FusedTorchAdamW, ModelEma, param_groups
    ema = ModelEma(m, decay=decay) if with_ema else None
    opt = FusedTorchAdamW(param_groups(m, F["weight_decay"], F["layer_decay"], trainable=trainable), m.store, lr=F["lr"], model=m)
    for g in opt.param_groups:
        g["lr"] = F["lr"] * g["lr_scale"]
    step = FinetuneStep(m, opt, clip_grad=1.0, update_freq=update_freq, trainable=trainable, model_ema=ema)
    return step, opt, ema


@pytest.fixture(scope="module")
def data():
    """six calls' clips and soft targets, computed once and left unchanged"""
    return [(S.synth_clip(S.TINY, F["B"], F["T"], F["clip_seed"] + 10 * k), R.soft_targets(F["B"], F["classes"], F["target_seed"] + 10 * k))
            for k in range(6)]


def test_six_calls_at_update_freq_two_against_a_twin_without_an_average(K, data):
    a, b = build(), build()
    sa, oa, ema = make(a, with_ema=True, update_freq=2)
    sb, ob, _ = make(b, with_ema=False, update_freq=2)
    assert oa.ema is not None and ob.ema is None
    KB.assert_equal_bits(ema.flat, a.store.flat, "a new average is a bit copy of the masters")
    groups = oa.chunk_group.cpu().numpy()
    want = ema.flat.cpu().numpy().copy()
    changes = 0
    for k, (clip, tg) in enumerate(data):
        prev = ema.flat.clone()
        ra, rb = sa.step(clip, tg), sb.step(clip, tg)
        for key in ("loss", "logits"):
            KB.assert_equal_bits(ra[key].reshape(-1), rb[key].reshape(-1), f"call {k}: {key} against the twin")
        assert (ra["grad_norm"] is None) == (rb["grad_norm"] is None) == (k % 2 == 0)
        if ra["grad_norm"] is not None:
            KB.assert_equal_bits(ra["grad_norm"].reshape(1), rb["grad_norm"].reshape(1), f"call {k}: grad_norm against the twin")
        for nm, x, y in (("flat", a.store.flat, b.store.flat), ("exp_avg", a.store.m, b.store.m), ("exp_avg_sq", a.store.v, b.store.v),
                         ("shadow", a.store.shadow, b.store.shadow), ("shadow_t", a.store.shadow_t, b.store.shadow_t)):
            KB.assert_equal_bits(x, y, f"call {k}: {nm} against the twin")
        if k % 2 == 0:  # a call that only accumulates leaves the average alone
            KB.assert_equal_bits(ema.flat, prev, f"call {k} only accumulates: the average")
            continue
        assert not torch.equal(ema.flat, prev), k
        changes += 1
        want = E.ema_ref_chunks(want, b.store.flat.cpu().numpy(), groups, DECAY)
        np_bits_equal(ema.flat, want, f"the average after update {changes} against the restatement replayed from the twin's masters")
    assert changes == 3
    assert not torch.equal(ema.flat, a.store.flat)
    sd = ema.state_dict()
    for n, t in a.named_parameters():  # every trainable tensor, by name
        o = a.store.off[a.store_name(n)]
        np_bits_equal(sd[n], want[o:o + t.numel()], f"state_dict()[{n}] against the restatement")


def test_linear_probe_average_follows_the_head_and_keeps_the_tower(K, data):
    m = build()
    first = {n: t.detach().clone() for n, t in m.named_parameters()}
    step, opt, ema = make(m, with_ema=True, trainable="head", decay=0.99)
    groups = opt.chunk_group.cpu().numpy()
    assert (groups == 255).sum() > (groups != 255).sum() > 0
    want = ema.flat.cpu().numpy().copy()
    for k in range(3):
        step.step(*data[k])
        want = E.ema_ref_chunks(want, m.store.flat.cpu().numpy(), groups, 0.99)
    sd = ema.state_dict()
    for n, t in m.named_parameters():
        o = m.store.off[m.store_name(n)]
        if n.startswith("head."):
            np_bits_equal(sd[n], want[o:o + t.numel()], f"linear probe: the average of {n} against the restatement")
            assert not torch.equal(sd[n], t) and not torch.equal(t, first[n]), n
        else:
            KB.assert_equal_bits(sd[n], t.detach(), f"linear probe: the average of the frozen {n} is the parameter")
            KB.assert_equal_bits(sd[n], first[n], f"linear probe: the average of the frozen {n} kept its bits")


def test_applied_evaluates_from_the_average_and_restores(K, data):
    from tvts_amd.downstream.finetune_v1 import ModelEma
    m = build()
    step, opt, ema = make(m, with_ema=True, decay=0.5)
    for k in range(2):
        step.step(*data[k])
    x = data[2][0]
    st = m.store

    def snapshot():
        return dict(flat=st.flat.clone(), ema=ema.flat.clone(), shadow=st.shadow.clone(), shadow_t=st.shadow_t.clone(), logits=m(x).clone())
    before = snapshot()
    assert not torch.equal(before["flat"], before["ema"])
    fresh = build(rate=0.0, sd=ema.state_dict())
    want = fresh(x)
    assert not torch.equal(want, before["logits"])

    def restored(what):
        after = snapshot()
        for key in before:
            KB.assert_equal_bits(after[key], before[key], f"{what}: {key}")
    with ema.applied() as inside:
        assert inside is m
        KB.assert_equal_bits(m(x), want, "inside applied(): logits against a fresh model loaded from ema.state_dict()")
        KB.assert_equal_bits(st.flat, before["ema"], "inside applied(): the masters hold the average")
        KB.assert_equal_bits(ema.flat, before["flat"], "inside applied(): the average holds the masters")
        KB.assert_equal_bits(st.shadow, fresh.store.shadow, "inside applied(): the bf16 shadow")
        KB.assert_equal_bits(st.shadow_t, fresh.store.shadow_t, "inside applied(): the transposed shadow")
        with pytest.raises(RuntimeError, match="applied"):
            step.step(*data[2])
        for call in (ema.update, ema.state_dict, lambda: ema.load_state_dict({}), lambda: ema.applied().__enter__(),
                     lambda: ModelEma(m).applied().__enter__()):
            with pytest.raises(RuntimeError, match="applied"):
                call()
        KB.assert_equal_bits(m(x), want, "inside applied(), behind the refused calls: logits")
    restored("behind applied()")
    with pytest.raises(KeyError, match="thrown inside"):
        with ema.applied():
            raise KeyError("thrown inside")
    restored("behind an exception inside applied()")
    out = step.step(*data[2])  # and the step runs on
    assert out["grad_norm"] is not None and not torch.equal(st.flat, before["flat"])


def test_state_dict_has_the_models_keys_and_shapes(K):
    m = build()
    _, _, ema = make(m, with_ema=True)
    sd, msd = ema.state_dict(), m.state_dict()
    assert list(sd) == list(msd)
    for k in msd:
        assert sd[k].shape == msd[k].shape and sd[k].dtype == msd[k].dtype == F32 and sd[k].device == msd[k].device, k
        KB.assert_equal_bits(sd[k], msd[k].detach(), f"state_dict()[{k}] of a new average")
    was = ema.flat.clone()
    for v in sd.values():
        v.fill_(7.0)  # clones: writing to them does not reach the average
    KB.assert_equal_bits(ema.flat, was, "state_dict() returned views of the average")
    with pytest.raises(KeyError):
        ema.load_state_dict({k: v for k, v in sd.items() if k != "head.bias"})
    ema.load_state_dict(sd)
    assert all(bool((v == 7.0).all()) for v in ema.state_dict().values())
    assert int(ema.checksum()) == int(ema.flat.view(torch.int32).sum(dtype=torch.int64)) and ema.checksum().dtype == torch.int64


def test_update_alone_is_the_separate_pass(K, data):
    """a loop that calls update() itself, the way the reference does: the step without an average, then ModelEma.update(model) --
    the bits of the fused launch"""
    a, b = build(), build()
    sa, _, ea = make(a, with_ema=True)
    sb, ob, _ = make(b, with_ema=False)
    from tvts_amd.downstream.finetune_v1 import ModelEma
    eb = ModelEma(b, decay=DECAY)
    for k in range(2):
        sa.step(*data[k])
        sb.step(*data[k])
        eb.update(b)
    KB.assert_equal_bits(a.store.flat, b.store.flat, "the masters")
    KB.assert_equal_bits(eb.flat, ea.flat, "update() behind the step against the fused launch")
    assert not torch.equal(ea.flat, a.store.flat)


def test_resume_after_two_updates_continues_bit_for_bit(K, data):
    a = build()
    sa, _, ea = make(a, with_ema=True)
    for k in range(4):
        sa.step(*data[k])
    b = build()
    sb, ob, eb = make(b, with_ema=True)
    for k in range(2):
        sb.step(*data[k])
    ckpt = dict(model={k: v.detach().clone() for k, v in b.state_dict().items()}, model_ema=eb.state_dict(),
                optimizer=ob.state_dict(), seed=b.engine.drop_seed_base())
    c = build(sd=ckpt["model"])
    sc, oc, ec = make(c, with_ema=True)
    ec.load_state_dict(ckpt["model_ema"])
    oc.load_state_dict(ckpt["optimizer"])
    c.engine.set_drop_seed_base(ckpt["seed"])
    KB.assert_equal_bits(ec.flat, eb.flat, "the loaded average")
    for k in range(2, 4):
        sc.step(*data[k])
    KB.assert_equal_bits(c.store.flat, a.store.flat, "resumed run: the masters")
    KB.assert_equal_bits(ec.flat, ea.flat, "resumed run: the average against four uninterrupted updates")
    assert int(ec.checksum()) == int(ea.checksum())
