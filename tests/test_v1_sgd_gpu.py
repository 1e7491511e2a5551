"""torch.optim.SGD for the v1 linear probe on the GPU (run with -m gpu): tvts_sgd_torch without and with `ema` bit for bit against
tests/v1_sgd_ref.py (the numpy restatement with an exact FMA, held to torch on the CPU by tests/test_v1_sgd_cpu.py), FusedTorchSGD
inside FinetuneStep against a real torch.optim.SGD(foreach=False) on the CPU fed with the engine's own gradients, checkpoints in
both directions, gradient accumulation and create_optimizer.  Everything is bit equality: the rule is a chain of fp32 operations
with a defined rounding each, so there is no bound to derive.  Step tests: tests/v1_downstream_synth.TINY, 7 classes, B = 3,
T = 8, drop-path 0 (the engine's gradients are then bit-reproducible, and a twin model holding the same bits produces them)."""
import argparse
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
import v1_downstream_synth as S  # noqa: E402
import v1_ema_ref as E  # noqa: E402
import v1_finetune_ref as R  # noqa: E402
import v1_sgd_ref as G  # noqa: E402
from test_v1_finetune_gpu import build, fwd_bwd, store_grads  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
F = R.FX
CH = 1024
GUARD = 1024  # elements of NaN in front of and behind every guarded buffer (a multiple of 4: the view stays 16-byte aligned)
EINVAL = -22
MU = 0.9
MODES = {"nesterov": dict(momentum=MU, nesterov=True), "momentum": dict(momentum=MU, nesterov=False),
         "momentum0": dict(momentum=0.0, nesterov=False)}
# groups 0, 1, 63 step (weight decay in 0 and 63 only); 255 = frozen and 64 = a foreign group keep every bit
LR = {0: 0.1, 1: 3e-3, 63: 1e-2}
WD = {0: 1e-9, 1: 0.0, 63: 0.05}
SIX = [0, 1, 63, 255, 64, 1]


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
    KB.assert_equal_bits(got.detach().cpu().reshape(-1), torch.from_numpy(np.ascontiguousarray(want)).reshape(-1), what)


def group_table(nchunks):
    if nchunks == 1:
        return [0]
    if nchunks == 6:
        return list(SIX)
    rng = np.random.RandomState(17)
    t = rng.choice([0, 1, 63, 255, 64], size=nchunks).tolist()
    t[:6], t[-2:] = SIX, [255, 63]
    return t


def hyper_table():
    h = torch.full((128,), 7.0)  # (groups nobody uses hold a value that would show)
    for gi in LR:
        h[gi], h[64 + gi] = LR[gi], WD[gi]
    return h


_STATES = {}


def sgd_state(nchunks):
    """fp32 p, g, buf over nchunks chunks, made once per size and left unchanged; chunk 0 carries g = -0.0 / +0.0 (0..7), |g| =
    1e-12 (8..15), |p| = 1e4 (16); with more than one chunk, chunk 1 (group 1: no weight decay) starts with g = -0.0 too"""
    if nchunks not in _STATES:
        n = CH * nchunks
        gen = torch.Generator().manual_seed(2300 + nchunks)
        p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1
        b = torch.randn(n, generator=gen) * 0.05
        g[:8] = torch.tensor([-0.0, 0.0] * 4)
        g[8:16] = torch.tensor([1e-12, -1e-12] * 4)
        p[16] = -1e4
        if nchunks > 1:
            g[CH:CH + 4] = -0.0
        _STATES[nchunks] = (p, g, b)
    return _STATES[nchunks]


def launch(K, state, groups, step, mode, *, device_step=False, coef=None, grad_scale=0.5, ema=None, decay=None, nan_buf=False):
    """one launch on guarded copies -> (p, buf, shadow) device views; nan_buf: the buffer starts as NaN (a first update must not
    read it)"""
    p, g, b = state
    pv, pb = guarded(p)
    gv, gb = guarded(g)
    bv, bb = guarded(torch.full_like(b, NAN) if nan_buf else b)
    sv, sb = guarded(torch.full((p.numel(),), -3.0, dtype=BF16))
    nc = None if coef is None else torch.tensor([123.0, coef], dtype=F32, device=DEV)
    sd = torch.tensor([step], dtype=torch.int32, device=DEV) if device_step else None
    kw = {} if ema is None else dict(ema=ema, ema_decay=decay)
    K.sgd_torch(pv, gv, bv, sv, torch.tensor(groups, dtype=torch.uint8, device=DEV), hyper_table().to(DEV), 0 if device_step else step,
                grad_scale=grad_scale, step_dev=sd, norm_coef=nc, **MODES[mode], **kw)
    torch.cuda.synchronize()
    for buf, nm in ((pb, "p"), (gb, "g"), (bb, "buf"), (sb, "shadow")):
        intact(buf, nm)
    KB.assert_equal_bits(gv.cpu(), g, "the gradient must stay")
    return pv, bv, sv


# ================================================================================================ 1. the kernel
@pytest.mark.parametrize("coef", [None, 0.37])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("nchunks", [1, 6, 2500])
def test_sgd_torch_bit_for_bit(K, nchunks, step, mode, coef):
    state, groups = sgd_state(nchunks), group_table(nchunks)
    first, mom = step == 1, MODES[mode]["momentum"] != 0
    p0, g0, b0 = (t.numpy() for t in state)
    want_p, want_b, stepped = G.sgd_ref_chunks(p0, g0, b0, groups, LR, WD, first=first, gs=G.scale32(0.5, coef), **MODES[mode])
    host = launch(K, state, groups, step, mode, coef=coef, nan_buf=first and mom)
    if first and mom:  # the buffer was NaN: chunks that do not step keep the NaN bits, the others hold d
        want_b = np.where(stepped, want_b, np.float32(NAN))
        b_before = torch.full_like(state[2], NAN)
    else:
        b_before = state[2]
    np_bits_equal(host[0], want_p, f"sgd_torch {mode} step {step}: p against the restatement")
    np_bits_equal(host[1], want_b if mom else b0, f"sgd_torch {mode} step {step}: momentum buffer")
    if not mom:
        KB.assert_equal_bits(host[1].cpu(), state[2], "momentum 0: the buffer must stay")
    want_sh = np.where(stepped, G.bf16_bits(want_p), torch.tensor([-3.0], dtype=BF16).view(torch.int16).numpy().view(np.uint16)[0])
    assert np.array_equal(host[2].cpu().view(torch.int16).numpy().view(np.uint16), want_sh), "shadow == bf16(p) on stepped chunks, untouched elsewhere"
    for ci, grp in enumerate(groups[:64]):  # chunk by chunk: frozen and foreign chunks keep every bit
        sl = slice(ci * CH, (ci + 1) * CH)
        if grp >= 64:
            KB.assert_equal_bits(host[0][sl].cpu(), state[0][sl], f"group {grp}: p must stay")
            KB.assert_equal_bits(host[1][sl].cpu(), b_before[sl], f"group {grp}: buf must stay")
            KB.assert_equal_bits(host[2][sl].cpu(), torch.full((CH,), -3.0, dtype=BF16), f"group {grp}: shadow must stay")
        else:
            assert not torch.equal(host[0][sl].cpu(), state[0][sl]), ci
    assert stepped.any() and (nchunks == 1 or not stepped.all())
    if first and mom and nchunks > 1:  # group 1 has no weight decay: the first update leaves the gradient's -0.0 in the buffer
        assert host[1][CH:CH + 4].cpu().view(torch.int32).tolist() == [-(1 << 31)] * 4
    dev = launch(K, state, groups, step, mode, coef=coef, device_step=True, nan_buf=first and mom)
    again = launch(K, state, groups, step, mode, coef=coef, nan_buf=first and mom)
    for nm, x, y, z in zip(("p", "buf", "shadow"), host, dev, again):
        KB.assert_equal_bits(x, y, f"sgd_torch host step vs device step {step}: {nm}")
        KB.assert_equal_bits(x, z, f"sgd_torch, a second identical launch: {nm}")


def test_momentum_zero_takes_no_buffer(K):
    state, groups = sgd_state(6), SIX
    p, g, _ = state
    pv, pb = guarded(p)
    sv, _ = guarded(torch.full((p.numel(),), -3.0, dtype=BF16))
    K.sgd_torch(pv, g.to(DEV), None, sv, torch.tensor(groups, dtype=torch.uint8, device=DEV), hyper_table().to(DEV), 1, grad_scale=0.5)
    want_p, _, _ = G.sgd_ref_chunks(p.numpy(), g.numpy(), None, groups, LR, WD, first=True, gs=G.scale32(0.5), **MODES["momentum0"])
    np_bits_equal(pv, want_p, "momentum 0 without a buffer")
    intact(pb, "p")


# ================================================================================================ 2. the fused average
@pytest.mark.parametrize("device_step", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("step", [1, 1000])
def test_fused_average_is_the_plain_launch_plus_the_separate_pass(K, step, mode, device_step):
    decay = 0.9999
    state = sgd_state(6)
    e = torch.randn(state[0].numel(), generator=torch.Generator().manual_seed(77))
    e[:4] = torch.tensor([0.0, -0.0, 3e38, -3e38])
    plain = launch(K, state, SIX, step, mode, coef=0.37, device_step=device_step)
    ev, ebuf = guarded(e)
    fused = launch(K, state, SIX, step, mode, coef=0.37, device_step=device_step, ema=ev, decay=decay)
    for nm, x, y in zip(("p", "buf", "shadow"), fused, plain):
        KB.assert_equal_bits(x, y, f"sgd_torch with an average against the launch without, {mode} step {step}: {nm}")
    sep = e.to(DEV).clone()
    K.ema_update(sep, plain[0].contiguous(), torch.tensor(SIX, dtype=torch.uint8, device=DEV), decay)
    KB.assert_equal_bits(ev, sep, "the fused average against ema_update behind the plain launch")
    np_bits_equal(ev, E.ema_ref_chunks(e.numpy(), plain[0].cpu().numpy(), SIX, decay), "the fused average against the restatement")
    for c in (3, 4):
        KB.assert_equal_bits(ev[c * CH:(c + 1) * CH].cpu(), e[c * CH:(c + 1) * CH], f"group {SIX[c]}: the average must stay")
    assert not torch.equal(ev[:CH].cpu(), e[:CH])
    intact(ebuf, "ema")


# ================================================================================================ 3. refusals
def test_entry_points_refuse_with_einval(K):
    """every refusal of the host entry point, without and with an average, through the library itself; nothing is launched and the operands keep their bits"""
    lib = K._lib.load()
    n = 2 * CH
    t = {k: torch.ones(n + 8, dtype=F32, device=DEV) for k in ("p", "g", "buf", "ema")}
    sh = torch.ones(n + 8, dtype=BF16, device=DEV)
    grp = torch.zeros(2, dtype=torch.uint8, device=DEV)
    hyper = hyper_table().to(DEV)
    sdev = torch.ones(1, dtype=torch.int32, device=DEV)

    def ptr(x, off=0):
        return None if x is None else ctypes.c_void_p(x.data_ptr() + off)

    def call(ema=False, **o):
        a = dict(p=ptr(t["p"]), g=ptr(t["g"]), buf=ptr(t["buf"]), shadow=ptr(sh), chunk_group=ptr(grp), nchunks=2, hyper=ptr(hyper),
                 step=1, step_dev=None, momentum=0.9, nesterov=1, grad_scale=1.0, norm_coef=None, e=ptr(t["ema"]))
        a.update(o)
        args = [a[k] for k in ("p", "g", "buf", "shadow", "chunk_group", "nchunks", "hyper", "step", "step_dev", "momentum", "nesterov",
                               "grad_scale", "norm_coef")]
        return lib.tvts_sgd_torch(*args, a["e"] if ema else None, 0.5, 0.5, None, None)
    cases = [dict(p=None), dict(g=None), dict(buf=None), dict(chunk_group=None), dict(hyper=None), dict(nchunks=0), dict(nchunks=-3),
             dict(step=0), dict(step=-1), dict(momentum=0.0, nesterov=1),
             dict(p=ptr(t["p"], 4)), dict(g=ptr(t["g"], 8)), dict(buf=ptr(t["buf"], 4)), dict(shadow=ptr(sh, 2)), dict(shadow=ptr(sh, 4))]
    for fused in (False, True):
        for o in cases:
            assert call(ema=fused, **o) == EINVAL, (fused, o)
    assert call(ema=True, e=ptr(t["ema"], 4)) == EINVAL  # (a null ema is the launch without an average: the `fused=False` cases)
    torch.cuda.synchronize()
    for k, v in t.items():
        assert bool((v == 1).all()), k
    assert bool((sh == 1).all())
    # accepted: step 0 with a device counter; a null buffer with momentum 0
    assert call(step=0, step_dev=ptr(sdev)) == 0 and call(momentum=0.0, nesterov=0, buf=None) == 0
    torch.cuda.synchronize()
    assert not bool((t["p"][:n] == 1).any()) and bool((t["p"][n:] == 1).all())
    with pytest.raises(ValueError):
        K.sgd_torch(t["p"], t["g"], t["buf"], None, grp, hyper, 1, momentum=0.9, ema=t["ema"])
    with pytest.raises(K.HipError):
        K.sgd_torch(t["p"], t["g"], None, None, grp, hyper, 1, momentum=0.0, nesterov=True)


def sgd_opt(m, trainable="all", lr=0.1, wd=0.05, layer_decay=0.75, **kw):
    from tvts_amd.downstream.finetune_v1 import FusedTorchSGD, param_groups
    opt = FusedTorchSGD(param_groups(m, wd, layer_decay, trainable=trainable), m.store, lr=lr, model=m, **kw)
    for g in opt.param_groups:
        g["lr"] = lr * g["lr_scale"]
    return opt


def test_constructor_refusals_and_state_buffers(K):
    from tvts_amd.downstream.finetune_v1 import FusedTorchSGD
    from tvts_amd.optim import _FlatAdamW, _FlatOptimizer, FusedHFAdamW, FusedTorchAdamW
    assert issubclass(FusedTorchSGD, _FlatOptimizer) and not issubclass(FusedTorchSGD, _FlatAdamW) and FusedTorchSGD.MAX_GROUPS == 64
    assert issubclass(FusedTorchAdamW, _FlatAdamW) and issubclass(FusedHFAdamW, _FlatAdamW) and issubclass(_FlatAdamW, _FlatOptimizer)
    m = build(rate=0.0)
    ps = [p for _, p in m.named_parameters()]
    for kw in (dict(dampening=0.1), dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True)):
        with pytest.raises(NotImplementedError):
            FusedTorchSGD(ps, m.store, lr=0.1, momentum=0.9, **kw)
    with pytest.raises(ValueError, match="Nesterov"):
        FusedTorchSGD(ps, m.store, lr=0.1, momentum=0, nesterov=True)
    with pytest.raises(ValueError):
        FusedTorchSGD(ps, m.store, lr=-0.1)
    with pytest.raises(ValueError, match="flat store"):
        FusedTorchSGD([torch.nn.Parameter(torch.zeros(4, device=DEV))], m.store, lr=0.1)
    assert m.store.m is None and m.store.v is None
    o0 = FusedTorchSGD(ps, m.store, lr=0.1)  # momentum 0: no state at all
    assert m.store.m is None and m.store.v is None and len(o0.state) == 0
    m.store.grad.normal_(generator=torch.Generator(DEV).manual_seed(1))
    p0 = m.store.flat.clone()
    o0.step()
    assert m.store.m is None and len(o0.state_dict()["state"]) == 0 and not torch.equal(m.store.flat, p0)
    o1 = FusedTorchSGD(ps, m.store, lr=0.1, momentum=0.9, nesterov=True)
    assert m.store.m is not None and m.store.v is None and len(o1.state) == 0 and len(o1.state_dict()["state"]) == 0
    want = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1, momentum=0.9, nesterov=True).param_groups[0]
    assert [k for k in o1.param_groups[0] if k != "params"] == [k for k in want if k != "params"]
    o1.step()
    name0 = next(iter(dict(m.named_parameters())))
    buf0 = o1.state[ps[0]]["momentum_buffer"]  # a view of store.m at the parameter's offset, in the parameter's shape
    assert set(o1.state[ps[0]]) == {"momentum_buffer"} and buf0.shape == ps[0].shape
    assert buf0.data_ptr() == m.store.m.data_ptr() + 4 * m.store.off[m.store_name(name0)]
    o1.param_groups[0]["momentum"] = 0.0  # the buffer was allocated for momentum: switching it off afterwards is refused
    with pytest.raises(ValueError, match="momentum"):
        o1.step()


# ================================================================================================ 4. the model against torch.optim.SGD
@pytest.fixture(scope="module")
def data():
    """three calls' clips and soft targets, computed once and left unchanged"""
    return [(S.synth_clip(S.TINY, F["B"], F["T"], F["clip_seed"] + 10 * k), R.soft_targets(F["B"], F["classes"], F["target_seed"] + 10 * k))
            for k in range(3)]


def cpu_twin(opt, m, momentum, nesterov):
    """a real torch.optim.SGD over CPU copies of the optimizer's parameters, group by group with its lr / weight_decay"""
    byptr = {p.data_ptr(): n for n, p in m.named_parameters()}
    leaves, groups = {}, []
    for g in opt.param_groups:
        names = [byptr[p.data_ptr()] for p in g["params"]]
        for n, p in zip(names, g["params"]):
            leaves[n] = p.detach().cpu().clone().requires_grad_(True)
        groups.append(dict(params=[leaves[n] for n in names], lr=g["lr"], weight_decay=g["weight_decay"]))
    return leaves, torch.optim.SGD(groups, lr=0.1, momentum=momentum, nesterov=nesterov, foreach=False)


def run_against_torch(K, data, trainable, make_opt, clip_grad, momentum=MU, nesterov=True):
    from tvts_amd.downstream.finetune_v1 import FinetuneStep
    m = build(rate=0.0)
    opt = make_opt(m)
    step = FinetuneStep(m, opt, clip_grad=clip_grad, trainable=trainable)
    leaves, topt = cpu_twin(opt, m, momentum, nesterov)
    st = m.store
    m._fresh_shadows()  # (a new model derives its shadows on first use: the snapshot holds the derived ones)
    frozen0 = [t.clone() for t in (st.flat, st.shadow, st.shadow_t)]
    coefs = []
    for k, (clip, tg) in enumerate(data):
        twin = build(rate=0.0, sd={n: v.detach().cpu().clone() for n, v in m.state_dict().items()})
        KB.assert_equal_bits(twin.store.flat, st.flat, f"step {k}: the twin holds the model's bits")
        fwd_bwd(K, twin, clip, tg, trainable=trainable)
        grads = {n: g.cpu() for n, g in store_grads(twin).items()}
        out = step.step(clip, tg)
        coef = step.norm_coef[1].cpu()  # fp32 scalar
        coefs.append(float(coef))
        for n, leaf in leaves.items():
            leaf.grad = grads[n] * coef
        topt.step()
        params = dict(m.named_parameters())
        for n, leaf in leaves.items():
            KB.assert_equal_bits(params[n].detach().cpu(), leaf.detach(), f"{trainable} step {k}: {n} against torch.optim.SGD")
            KB.assert_equal_bits(opt.state[params[n]]["momentum_buffer"].cpu(), topt.state[leaf]["momentum_buffer"],
                                 f"{trainable} step {k}: momentum_buffer of {n} against torch.optim.SGD")
        assert (out["grad_norm"] is not None) and not bool(st.grad.any())
    return m, opt, coefs, frozen0, leaves


def test_probe_recipe_three_steps_against_torch_sgd(K, data):
    """(a) linear_ssv2.sh's optimizer line: --opt sgd --lr 0.1 --momentum 0.9 --weight_decay 1e-9, trainable="head" """
    from tvts_amd.downstream.finetune_v1 import FusedTorchSGD, create_optimizer
    args = argparse.Namespace(opt="sgd", lr=0.1, momentum=0.9, weight_decay=1e-9, opt_eps=1e-8, opt_betas=None)
    m, opt, coefs, frozen0, leaves = run_against_torch(K, data, "head", lambda m: create_optimizer(args, m, trainable="head"), None)
    assert isinstance(opt, FusedTorchSGD) and sorted(leaves) == ["head.bias", "head.weight"] and coefs == [1.0] * 3
    assert [(g["name"], g["weight_decay"]) for g in opt.param_groups] == [("decay", 1e-9), ("no_decay", 0.0)]
    st = m.store
    lo = st.off["head.weight"]
    assert lo == min(st.off[m.store_name(n)] for n in leaves)
    for nm, was, now in zip(("masters", "bf16 shadow"), frozen0, (st.flat, st.shadow)):
        KB.assert_equal_bits(now[:lo], was[:lo], f"linear probe: {nm} of the tower")
        assert not torch.equal(now[lo:], was[lo:]), nm
    KB.assert_equal_bits(st.shadow_t, frozen0[2], "linear probe: transposed shadows")
    KB.assert_equal_bits(st.m[:lo], torch.zeros_like(st.m[:lo]), "linear probe: momentum buffer of the tower")
    assert st.v is None


def test_all_layers_three_steps_against_torch_sgd(K, data):
    """(b) trainable="all", layer decay 0.75, weight_decay 0.05, a clip small enough to bind in every step"""
    m, opt, coefs, _, leaves = run_against_torch(K, data, "all", lambda m: sgd_opt(m, momentum=MU, nesterov=True), 0.05)
    assert all(0.0 < c < 1.0 for c in coefs), coefs
    assert len(leaves) == len(list(m.named_parameters())) and len(opt.param_groups) > 2
    assert len({g["lr"] for g in opt.param_groups}) > 1 and {g["weight_decay"] for g in opt.param_groups} == {0.0, 0.05}


# ================================================================================================ 5. checkpoints, accumulation
def fill_grad(m, leaves, seed):
    """the same random gradient into the store and into the CPU leaves"""
    g = torch.randn(m.store.grad.numel(), generator=torch.Generator().manual_seed(seed)) * 0.1
    m.store.grad.copy_(g)
    for n, leaf in leaves.items():
        o = m.store.off[m.store_name(n)]
        leaf.grad = g[o:o + leaf.numel()].view(leaf.shape).clone()


def assert_same(m, opt, leaves, topt, what):
    params = dict(m.named_parameters())
    for n, leaf in leaves.items():
        KB.assert_equal_bits(params[n].detach().cpu(), leaf.detach(), f"{what}: {n}")
        KB.assert_equal_bits(opt.state[params[n]]["momentum_buffer"].cpu(), topt.state[leaf]["momentum_buffer"], f"{what}: momentum_buffer of {n}")


@pytest.mark.parametrize("nesterov", [True, False])
def test_checkpoints_travel_both_ways(K, nesterov):
    m = build(rate=0.0)
    opt = sgd_opt(m, momentum=MU, nesterov=nesterov)
    leaves, topt = cpu_twin(opt, m, MU, nesterov)
    for k in range(2):
        fill_grad(m, leaves, 300 + k)
        opt.step()
    # fused -> torch: a fresh torch.optim.SGD over same-shaped CPU parameters loads the fused optimizer's state_dict
    params = dict(m.named_parameters())
    fresh = {n: params[n].detach().cpu().clone().requires_grad_(True) for n in leaves}
    byptr = {p.data_ptr(): n for n, p in params.items()}
    t2 = torch.optim.SGD([dict(params=[fresh[byptr[p.data_ptr()]] for p in g["params"]]) for g in opt.param_groups], lr=1.0, foreach=False)
    sd = opt.state_dict()
    assert len(sd["state"]) == len(leaves) and all(set(s) == {"momentum_buffer"} for s in sd["state"].values())
    t2.load_state_dict(sd)
    assert t2.param_groups[0]["momentum"] == MU and t2.param_groups[0]["nesterov"] == nesterov
    fill_grad(m, fresh, 310)
    opt.step()
    t2.step()
    assert_same(m, opt, fresh, t2, "one more step after fused -> torch")
    # torch -> fused: the twin that ran from the start (first update included) continues in a fresh fused optimizer
    for k in range(2):
        fill_grad(m, leaves, 300 + k)
        topt.step()
    m2 = build(rate=0.0, sd={n: leaves[n].detach().clone() if n in leaves else v.detach().cpu() for n, v in m.state_dict().items()})
    opt2 = sgd_opt(m2, momentum=MU, nesterov=nesterov)
    assert opt2.global_step == 0
    opt2.load_state_dict(topt.state_dict())
    assert opt2.global_step == 1 and int(opt2.step_dev.item()) == 1  # the next update is not a first one
    fill_grad(m2, leaves, 320)
    opt2.step()
    topt.step()
    assert_same(m2, opt2, leaves, topt, "one more step after torch -> fused")


def test_load_state_dict_first_update_rule(K):
    m = build(rate=0.0)
    opt = sgd_opt(m, momentum=MU, nesterov=True)
    leaves, topt = cpu_twin(opt, m, MU, True)
    fill_grad(m, leaves, 400)
    opt.step()
    sd = opt.state_dict()
    some = dict(sd, state={k: v for k, v in sd["state"].items() if k != 0})
    with pytest.raises(ValueError, match="all or none"):
        opt.load_state_dict(some)
    opt.load_state_dict(dict(sd, state={}))  # an empty state: the next update is a first one again
    assert opt.global_step == 0 and len(opt.state) == 0
    m.store.m.fill_(NAN)  # a first update writes the buffer without reading it
    leaves, topt = cpu_twin(opt, m, MU, True)
    fill_grad(m, leaves, 401)
    opt.step()
    topt.step()
    assert_same(m, opt, leaves, topt, "the first update after an empty state")


def test_update_freq_two_half_batches(K):
    """as the AdamW test: the first of two calls only accumulates, the second updates from the accumulated gradient"""
    from tvts_amd.downstream.finetune_v1 import FinetuneStep
    B, C = 4, F["classes"]
    clip, targets = S.synth_clip(S.TINY, B, F["T"], 71), R.soft_targets(B, C, 72)
    m = build(rate=0.0)
    fwd_bwd(K, m, clip, targets)
    full = {n: g.cpu() for n, g in store_grads(m).items()}
    K.zero_(m.store.grad)
    opt = sgd_opt(m, momentum=MU, nesterov=True)
    step = FinetuneStep(m, opt, update_freq=2)
    p0 = m.store.flat.clone()
    o1 = step.step(clip[:2], targets[:2])
    assert o1["grad_norm"] is None and torch.equal(m.store.flat, p0) and bool(m.store.grad.any()) and opt.global_step == 0
    acc = {n: g.cpu().clone() for n, g in store_grads(m).items()}
    o2 = step.step(clip[2:], targets[2:])
    gn_full = math.sqrt(sum(float(g.double().norm()) ** 2 for g in full.values()))
    assert abs(float(o2["grad_norm"]) - gn_full) < 0.01 * gn_full and not torch.equal(m.store.flat, p0)
    assert not bool(m.store.grad.any()) and opt.global_step == 1 and bool(acc["head.weight"].any())


# ================================================================================================ 6. create_optimizer
def test_create_optimizer_classes_groups_and_keywords(K):
    from tvts_amd.downstream.finetune_v1 import (FusedTorchAdamW, FusedTorchSGD, LayerDecayValueAssigner, create_optimizer,
                                                  layer_scales)
    depth = S.TINY["depth"]

    def check_groups(opt, m, wd, layer_decay, trainable):
        want = R.group_rule([(n, tuple(p.shape)) for n, p in m.named_parameters()], wd, layer_decay, depth, trainable=trainable)
        byptr = {p.data_ptr(): n for n, p in m.named_parameters()}
        got = [(g["name"], g["weight_decay"], g["lr_scale"], [byptr[p.data_ptr()] for p in g["params"]]) for g in opt.param_groups]
        assert got == [tuple(w) for w in want], (got, want)
    for name, cls, nes in (("sgd", FusedTorchSGD, True), ("nesterov", FusedTorchSGD, True), ("momentum", FusedTorchSGD, False),
                           ("SGD", FusedTorchSGD, True), ("adamw", FusedTorchAdamW, None)):
        for trainable, assigner in (("head", None), ("all", LayerDecayValueAssigner(layer_scales(depth, 0.75)))):
            m = build(rate=0.0)
            args = argparse.Namespace(opt=name, lr=0.1, momentum=0.9, weight_decay=0.05, opt_eps=1e-6, opt_betas=None)
            kw = {} if assigner is None else dict(get_num_layer=assigner.get_layer_id, get_layer_scale=assigner.get_scale)
            opt = create_optimizer(args, m, trainable=trainable, **kw)
            assert type(opt) is cls and opt.defaults["lr"] == 0.1 and opt.defaults["weight_decay"] == 0.0
            check_groups(opt, m, 0.05, 1.0 if assigner is None else 0.75, trainable)
            if cls is FusedTorchSGD:
                assert "eps" not in opt.defaults and "betas" not in opt.defaults
                assert all(g["momentum"] == 0.9 and g["nesterov"] is nes and g["dampening"] == 0 and g["lr"] == 0.1 for g in opt.param_groups)
                assert m.store.v is None
            else:
                assert opt.defaults["eps"] == 1e-6 and tuple(opt.defaults["betas"]) == (0.9, 0.999)
    # weight_decay 0 (or filter_bias_and_bn off): one group of every trainable parameter, the decay stays at the top level
    m = build(rate=0.0)
    opt = create_optimizer(argparse.Namespace(opt="momentum", lr=0.2, momentum=0.5, weight_decay=0.01), m, filter_bias_and_bn=False, trainable="head")
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["weight_decay"] == 0.01 and len(opt.param_groups[0]["params"]) == 2
    assert opt.param_groups[0]["momentum"] == 0.5 and opt.param_groups[0]["nesterov"] is False
    opt = create_optimizer(argparse.Namespace(opt="adamw", lr=1e-3, momentum=0.9, weight_decay=0.0, opt_eps=None, opt_betas=[0.9, 0.95]), m)
    assert len(opt.param_groups) == 1 and tuple(opt.defaults["betas"]) == (0.9, 0.95) and opt.defaults["eps"] == 1e-8
    for bad in ("adam", "fusedsgd", "lookahead_sgd", "rmsprop", "lamb"):
        with pytest.raises(NotImplementedError, match="built: adamw; sgd / nesterov"):
            create_optimizer(argparse.Namespace(opt=bad, lr=0.1, momentum=0.9, weight_decay=0.05), m)
    with pytest.raises(TypeError, match="opt_betas"):
        create_optimizer(argparse.Namespace(opt="sgd", lr=0.1, momentum=0.9, weight_decay=0.05, opt_betas=(0.9, 0.999)), m)
