"""Activation recomputation of the video towers (arch["recompute"] = "none" | "mlp" | "block", set_grad_checkpointing): a step that
evaluates its blocks (or their fc1) a second time in the backward leaves the BITS of the step that kept everything -- losses,
every gradient, the parameters after an update -- and keeps a fraction of its per-layer workspace.  DESIGN.md, "Activation
recomputation".

Shapes: the tiny architectures with layers = 3 (both slot parities and a middle block), odd batches off every tile edge, and the
alternation of two batch signatures that re-enters the grow-only buffers at two sizes (B = 3, NT = 4 -> B = 2, NT = 1 -> B = 3)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARGS = types.SimpleNamespace(local_rank=0, rank=0, world_size=1)
LAYERS = 3
BATCHES = ((3, 4, 4, 5), (2, 2, 1, 6), (3, 4, 4, 5))  # (B, T, NT, seed): the first again at the end


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def _arch(arch_name, layers=LAYERS, **over):
    from tvts_amd import arch as A
    fn = dict(small=A.small_arch, small_h=A.small_arch_h, v1=A.small_arch_v1)[arch_name]
    return fn(layers=layers, **over)


def _model(a):
    """the model with the training step's parameter groups and its StepRunner (tests/test_bench_path_gpu.py::_runner_of)"""
    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.model.model_dist_TVTS import TVTS
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner
    v1 = a.get("family") == "v1"
    m = (TVTS if v1 else TVTSv2Base)(ARGS, arch=a, init_seed=0)
    groups = [[], [], [], []]
    for name, p in m.named_parameters():
        gi = A.param_group_of(name, a)
        p.requires_grad = gi >= 0
        if gi >= 0:
            groups[gi].append(p)
    hp = ((1e-4, 0.0),) * 4 if v1 else A.GROUP_HPARAMS
    opt = FusedHFAdamW([dict(params=groups[i], lr=hp[i][0], weight_decay=hp[i][1]) for i in range(4) if groups[i]], m.store, model=m)
    if v1:
        m.engine.training = True  # DistilBERT's dropout (p = 0.1) on: the masks come from drop_seed
    return m, StepRunner(m, opt)


def _batch(a, B, T, NT, seed):
    from tvts_amd.data_loader import synth_batch, synth_batch_v1
    return (synth_batch_v1 if a.get("family") == "v1" else synth_batch)(a, B, T, seed=seed, n_trans=NT, caption_len=12)


def _grads(m, run, batch, seed0):
    """one forward / losses / backward as the training step runs them -> (flat gradient, loss1, loss2, recompute_count)"""
    eng = m.engine
    m._fresh_shadows(); m._sync_requires_grad()
    pb = eng.prepare_batch(batch)
    lab = batch["label"].reshape(-1).to(torch.int32).to(DEV) if "label" in batch and pb["NT"] != 1 else None
    if seed0 is not None:
        eng.drop_seed.copy_(seed0)
    m.store.grad.zero_()
    eng.embeds_ready = run.gather.start
    try:
        te, ve, pred = eng.forward(pb)
    finally:
        eng.embeds_ready = None
    l1, l2, dte, dve, dpred = run.losses_and_grads(pb, te, ve, pred, lab)
    eng.backward(dte, dve, dpred)
    torch.cuda.synchronize()
    return m.store.grad.clone(), float(l1), None if l2 is None else float(l2), eng.recompute_count


def _trace(arch_name, mode, flags, toggle=None):
    """the three alternating batches, then one StepRunner optimiser step -> ([(grad, l1, l2, count)], flat parameters).
    toggle: modes to switch to (set_grad_checkpointing) in front of each of the three batches, instead of a constructor mode."""
    a = _arch(arch_name, **dict(flags))
    if mode is not None:
        a["recompute"] = mode
    m, run = _model(a)
    eng = m.engine
    seed0 = eng.drop_seed.clone() if hasattr(eng, "drop_seed") else None
    out = []
    for i, (B, T, NT, seed) in enumerate(BATCHES):
        if toggle is not None:
            m.set_grad_checkpointing(toggle[i])
        out.append(_grads(m, run, _batch(a, B, T, NT, seed), seed0))
    if seed0 is not None:
        eng.drop_seed.copy_(seed0)
    run.step(_batch(a, *BATCHES[0]))
    torch.cuda.synchronize()
    return out, m.store.flat.clone(), eng


_REF = {}


def _reference(arch_name, flags):
    """the "none" run of a configuration: computed once, shared by the tests that compare against it, never written"""
    key = (arch_name, flags)
    if key not in _REF:
        out, flat, eng = _trace(arch_name, "none", flags)
        assert all(c == 0 for *_, c in out) and eng.recompute == "none"
        assert torch.isfinite(out[0][0]).all() and float(out[0][0].abs().max()) > 0
        _REF[key] = (out, flat)
    return _REF[key]


def _same(got, ref, what):
    for i, ((g, l1, l2, _), (g0, l10, l20, _)) in enumerate(zip(got[0], ref[0])):
        assert (l1, l2) == (l10, l20), f"{what}: losses of batch {i} differ: {(l1, l2)} against {(l10, l20)}"
        if not torch.equal(g, g0):
            d = (g - g0).abs()
            raise AssertionError(f"{what}: gradients of batch {i} differ: max |d| {float(d.max()):.3e} in {int((d > 0).sum())} elements")
    assert torch.equal(got[1], ref[1]), f"{what}: parameters differ after the optimiser step"


V2_CASES = [(n, f) for n in ("small", "small_h") for f in ((), (("hybrid_stream", False),), (("wgrad_stream", True),))] + \
           [("small", (("bf16_residual", True),)), ("small", (("tn_grouped", True),)), ("small", (("tn_grouped", False),)),
            ("small_h", (("wgrad_stream", True), ("hybrid_stream", False)))]


# ================================================================================================ 1. bit equality, v2
@pytest.mark.parametrize("mode", ["mlp", "block"])
@pytest.mark.parametrize("arch_name,flags", V2_CASES)
def test_v2_step_has_the_bits_of_the_step_that_keeps_everything(K, arch_name, flags, mode):
    ref = _reference(arch_name, flags)
    got = _trace(arch_name, mode, flags)
    eng = got[2]
    assert eng.recompute == mode
    for *_, count in got[0]:  # the slot's last writer (two of them beside the side stream) is not evaluated again
        assert LAYERS - 2 <= count <= LAYERS, count
    assert got[0][0][3] == (LAYERS - 2 if dict(flags).get("wgrad_stream") else LAYERS - 1)
    _same(got, ref, f"{arch_name} {flags} {mode}")
    if dict(flags).get("tn_grouped"):
        assert len(eng._tn_groups) == LAYERS  # (the grouped launches did run)


# ================================================================================================ 2. autograd path
@pytest.mark.parametrize("arch_name", ["small", "small_h"])
def test_autograd_path(K, arch_name):
    """loss.backward() through the model's autograd function: the same .grad bits in "block" as in "none" """
    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base, sim_matrix
    res = {}
    for mode in ("none", "block"):
        a = _arch(arch_name)
        m = TVTSv2Base(ARGS, arch=a, init_seed=0)
        m.set_grad_checkpointing(mode == "block")
        for name, p in m.named_parameters():
            p.requires_grad = A.param_group_of(name, a) >= 0
        te, ve, pred = m(_batch(a, 3, 4, 4, 5))
        loss = torch.nn.functional.cross_entropy(sim_matrix(te, ve) / 0.05, torch.arange(3, device=DEV)) + pred.square().mean()
        loss.backward()
        torch.cuda.synchronize()
        res[mode] = (float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, m.engine.recompute_count)
    assert res["none"][2] == 0 and res["block"][2] == LAYERS - 1
    assert res["none"][0] == res["block"][0] and res["none"][1].keys() == res["block"][1].keys() and len(res["none"][1]) > 10
    for n, g in res["none"][1].items():
        assert torch.equal(g, res["block"][1][n]), n
    assert any(float(g.abs().max()) > 0 for n, g in res["none"][1].items() if "resblocks.0.mlp" in n and "video" in n)


# ================================================================================================ 3. v1 pretrain step
@pytest.mark.parametrize("mode", ["mlp", "block"])
def test_v1_pretrain_step(K, mode):
    """small_arch_v1 with the text tower's training-mode dropout (0.1): the masks come from the same seed in both runs"""
    ref = _reference("v1", ())
    got = _trace("v1", mode, ())
    assert got[2].text_drop_p == 0.1 and got[2]._drop_active == 0.1
    for *_, count in got[0]:
        assert count == LAYERS - 1
    _same(got, ref, f"v1 {mode}")


# ================================================================================================ 4. v1 fine-tuning
TINY = dict(img_size=64, patch_size=16, embed_dim=128, depth=LAYERS, num_heads=2, num_frames=8, tubelet_size=2)
CLASSES = 5


def _finetune(mode, trainable, toggle=None, depth=LAYERS, calls=2):
    from tvts_amd.downstream.finetune_v1 import FinetuneStep, FusedTorchAdamW, param_groups
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    m = VisionTransformer(num_classes=CLASSES, drop_path_rate=0.2, init_seed=3, grad_checkpointing=mode, **dict(TINY, depth=depth))
    opt = FusedTorchAdamW(param_groups(m, 0.05, 0.75, trainable=trainable), m.store, lr=1e-3, model=m)
    for g in opt.param_groups:
        g["lr"] = 1e-3 * g["lr_scale"]
    step = FinetuneStep(m, opt, clip_grad=5.0, update_freq=2, trainable=trainable)
    gen = torch.Generator().manual_seed(11)
    outs, counts = [], []
    for i in range(calls):
        if toggle is not None:
            m.set_grad_checkpointing(toggle[i])
        clip = torch.randn(3, 3, 4, 64, 64, generator=gen)
        soft = torch.softmax(torch.randn(3, CLASSES, generator=gen), -1)
        r = step.step(clip, soft)
        torch.cuda.synchronize()
        outs.append((r["logits"].clone(), float(r["loss"]), None if r["grad_norm"] is None else float(r["grad_norm"])))
        counts.append(m.engine.recompute_count)
    return outs, counts, m.store.flat.clone(), m


@pytest.fixture(scope="module")
def ft_ref(K):
    return {t: _finetune("none", t)[:3] for t in ("all", "head")}


def _ft_same(got, ref, what):
    for i, ((lg, loss, gn), (lg0, loss0, gn0)) in enumerate(zip(got[0], ref[0])):
        assert torch.equal(lg, lg0) and loss == loss0 and gn == gn0, f"{what}: call {i}: {(loss, gn)} against {(loss0, gn0)}"
    assert got[0][0][2] is None and got[0][-1][2] is not None and got[0][-1][2] > 0  # (update_freq 2: the second call updates)
    assert torch.equal(got[2], ref[2]), f"{what}: parameters differ after the update"


@pytest.mark.parametrize("mode", ["mlp", "block", True])
def test_v1_finetune_step(K, ft_ref, mode):
    """FinetuneStep with drop-path 0.2, update_freq 2, clip_grad 5, soft targets, two calls: logits, loss, grad_norm and the
    parameters after the update"""
    assert ft_ref["all"][1] == [0, 0]
    got = _finetune(mode, "all")
    assert got[3].engine.recompute == ("block" if mode is True else mode)
    assert got[3].engine.buf["ft.dp_table"].shape == (2 * LAYERS, 3)  # (stochastic depth is on)
    assert got[1] == [LAYERS - 1] * 2, got[1]
    _ft_same(got, ft_ref["all"], f"finetune {mode}")


def test_v1_linear_probe_evaluates_nothing_again(K, ft_ref):
    got = _finetune("block", "head")
    assert got[1] == [0, 0]
    _ft_same(got, ft_ref["head"], "linear probe")


# ================================================================================================ 5. toggling
def test_toggling_between_steps(K):
    """set_grad_checkpointing(True), a step, False, a step, True, a step: each step is the step of a model that never toggled"""
    ref = _reference("small", ())
    got = _trace("small", None, (), toggle=(True, False, True))
    assert [c for *_, c in got[0]] == [LAYERS - 1, 0, LAYERS - 1]
    _same(got, ref, "toggled")
    ref = _finetune("none", "all", calls=3)
    got = _finetune(False, "all", toggle=("mlp", False, True), calls=3)
    assert got[1] == [LAYERS - 1, 0, LAYERS - 1]
    for (lg, loss, gn), (lg0, loss0, gn0) in zip(got[0], ref[0]):
        assert torch.equal(lg, lg0) and loss == loss0 and gn == gn0
    assert torch.equal(got[2], ref[2])


def test_constructors_read_the_config(K):
    """args.grad_checkpointing, the constructor keyword (an entry of the config's arch.args) and arch["recompute"], which wins"""
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.model.model_dist_TVTS import TVTS
    ns = types.SimpleNamespace
    a, a1 = _arch("small", layers=1, text_layers=1), _arch("v1", layers=1, text_layers=1)
    assert TVTSv2Base(ARGS, arch=a).engine.recompute == "none"
    assert TVTSv2Base(ns(local_rank=0, grad_checkpointing=True), arch=a).engine.recompute == "block"
    assert TVTSv2Base(ARGS, arch=a, grad_checkpointing="mlp").engine.recompute == "mlp"
    assert TVTSv2Base(ns(local_rank=0, grad_checkpointing=True), arch=dict(a, recompute="none")).engine.recompute == "none"
    assert TVTS(ARGS, arch=a1, grad_checkpointing=True).engine.recompute == "block"
    assert TVTS(ns(local_rank=0, grad_checkpointing="mlp"), arch=a1).engine.recompute == "mlp"
    m = VisionTransformer(num_classes=2, **dict(TINY, depth=1))
    assert m.engine.recompute == "none"
    m.set_grad_checkpointing()
    assert m.engine.recompute == "block"
    with pytest.raises(ValueError, match="fp8"):
        TVTSv2Base(ARGS, arch=dict(_arch("small_h", layers=1, text_layers=1), fp8=True), grad_checkpointing=True)
    with pytest.raises(ValueError, match="'everything'"):
        TVTSv2Base(ARGS, arch=a).set_grad_checkpointing("everything")


# ================================================================================================ 6. memory
def _growth(arch_name, mode, flags):
    """g(mode): what two more layers add to workspace_bytes() after one step"""
    out = []
    for layers in (LAYERS, LAYERS + 2):
        a = _arch(arch_name, layers=layers, recompute=mode, **dict(flags))
        m, run = _model(a)
        run.step(_batch(a, 3, 4, 4, 5))
        torch.cuda.synchronize()
        out.append(m.engine.workspace_bytes())
    return out[1] - out[0]


@pytest.mark.parametrize("arch_name,flags", [("small", ()), ("small_h", (("hybrid_stream", False),)), ("v1", ())])
def test_workspace_growth_per_layer(K, arch_name, flags):
    """Per block and row, in bf16 columns of the width: a v2 block saves 22 (hybrid stream; 24 with the fp32 stream), "block" keeps
    1 (2) of them -- the stream -- and "mlp" 14 (16); a v1 block 18, 2 and 10.  So two more layers may add at most 0.15 / 0.70 of what
    they add to the step that keeps everything."""
    g = {mode: _growth(arch_name, mode, flags) for mode in ("none", "mlp", "block")}
    print("workspace growth of two layers:", arch_name, flags, g)
    # one block's saved tensors at these shapes, against which per-layer index tables would have to be negligible: they are not
    # workspaces at all (the grouped plans live outside buf), so the growth IS the saved tensors
    assert g["none"] > 2 * 200_000
    assert g["none"] > 0
    assert g["block"] <= 0.15 * g["none"], g
    assert g["mlp"] <= 0.70 * g["none"], g
