"""The micro-batched pretraining step, StepRunner(micro_batches=n) (run with -m gpu): the exact full-batch contrastive
loss from n chunks of B / n clips -- embeddings of every chunk, one loss + dE over the whole batch, every chunk again for its backward.

Reference: the oracle's UNSPLIT step (tests/micro_batch_ref.py::unsplit_grads, O.train_step).  Gates, all taken from the existing
model-vs-oracle tests: |d loss| < 1e-2, check_grads of tests/test_model_gpu.py on EVERY trainable tensor (norm within 1 %, per-tensor
cosine > 0.995), parameters rel-L2 < 2e-2 (test_training_curve_tracks_oracle)."""
import math
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import micro_batch_ref as R  # noqa: E402
import train_guard_ref as G  # noqa: E402
from test_model_gpu import check_grads  # noqa: E402
from test_train_guard_gpu import bits, make, rel, same_bits, same_state, snapshot  # noqa: E402

from oracle import tvts_oracle as O  # noqa: E402  (checker only)

DEV = "cuda:0"
KEYS = ("pred_model.head.weight", "video_model.transformer.resblocks.1.timeattn.proj.weight")  # (test_training_curve_tracks_oracle's)


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import arch as A
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    return a, oarch, O.synth_params(oarch, seed=31)


@pytest.fixture(scope="module")
def b4(tiny):
    """three batches of 4 clips and the oracle's unsplit step on the first (computed once, read only)"""
    _, oarch, P = tiny
    batches = [O.synth_batch(oarch, B=4, T=2, seed=40 + i, caption_len=8) for i in range(3)]
    return batches, R.unsplit_grads(P, batches[0], oarch)


def grads_of(m, names):
    torch.cuda.synchronize()
    return {k: m.store.g(k).detach().cpu().clone() for k in names}


def margins(m, ref):
    tot, tot_ref, worst = check_grads(m.store, ref)
    return f"gradient norm {tot / tot_ref - 1:+.2e} (gate 1e-2), worst tensor cosine {worst[0][0]:.5f} {worst[0][1]} (gate 0.995)"


def test_micro_batches_1_is_todays_step(tiny, b4):
    a, oarch, P = tiny
    m0, opt0, r0 = make(a, P)
    m1, opt1, r1 = make(a, P, micro_batches=1)
    assert r0.micro_batches == r1.micro_batches == 1
    for b in b4[0]:
        o0, o1 = r0.step(b), r1.step(b)
        assert list(o0) == list(o1) == ["loss1", "loss2"]
        same_bits(o0["loss1"], o1["loss1"], "loss1")
        same_bits(o0["loss2"], o1["loss2"], "loss2")
    same_state(m1, snapshot(m0), "micro_batches=1 against no argument")
    assert opt0.global_step == opt1.global_step == 3


def test_second_forward_reproduces_the_cached_embeddings(tiny, b4):
    """the gradient is taken AT the cached point: every chunk's pass-2 embeddings are its rows of the two caches, bit for bit; and
    embeds_ready stays unarmed in every micro forward"""
    a, oarch, P = tiny
    m, opt, r = make(a, P, micro_batches=2)
    seen, armed = {}, []

    def observe(k, te, ve):
        seen[k] = (te.clone(), ve.clone())
        armed.append(m.engine.embeds_ready)
    r.micro_observer = observe
    r.step(b4[0][0])
    torch.cuda.synchronize()
    assert sorted(seen) == [0, 1] and armed == [None, None]
    t_cache, v_cache = r._emb_cache
    assert tuple(t_cache.shape) == tuple(v_cache.shape) == (4, a["embed"]) and t_cache.dtype == torch.float32
    for k, (te, ve) in seen.items():
        same_bits(te, t_cache[2 * k:2 * k + 2], f"text embeddings of chunk {k}")
        same_bits(ve, v_cache[2 * k:2 * k + 2], f"video embeddings of chunk {k}")
    assert not torch.equal(t_cache[:2], t_cache[2:]) and not torch.equal(v_cache[:2], v_cache[2:])


@pytest.mark.parametrize("B,n,seed", [(4, 2, 40), (4, 4, 43), (6, 3, 42)])
def test_one_step_against_the_unsplit_oracle(tiny, B, n, seed):
    """losses, the gradient of EVERY trainable tensor (store.grad is read behind the step: the update leaves it), the norm"""
    a, oarch, P = tiny
    batch = O.synth_batch(oarch, B=B, T=2, seed=seed, caption_len=8)
    l1, l2, ref = R.unsplit_grads(P, batch, oarch)
    mp, _, rp = make(a, P)
    op = rp.step(batch)
    plain = margins(mp, ref)
    m, opt, r = make(a, P, micro_batches=n, clip_grad=1e9)  # (max_norm 1e9: no clipping, the step reports its gradient norm)
    out = r.step(batch)
    torch.cuda.synchronize()
    g1, g2 = float(out["loss1"]), float(out["loss2"])
    ref_norm = float(R.flat(ref).norm())
    print(f"\n   [B {B} n {n}] loss1 {g1:.5f} (oracle {l1:.5f}, plain step {float(op['loss1']):.5f}) loss2 {g2:.5f} (oracle {l2:.5f}, plain "
          f"{float(op['loss2']):.5f})\n      micro: {margins(m, ref)}\n      plain: {plain}\n      grad_norm {float(out['grad_norm']):.6f} "
          f"oracle {ref_norm:.6f}; gradient rel-L2 micro vs plain {rel(m.store.grad, mp.store.grad):.2e}")
    assert abs(g1 - l1) < 1e-2 and abs(g2 - l2) < 1e-2, (g1, l1, g2, l2)
    assert len(ref) > 50 and all(m.engine.requires_grad[k] for k in ref)
    check_grads(m.store, ref)
    assert abs(float(out["grad_norm"]) - ref_norm) < 1e-2 * ref_norm
    # frozen tensors stay without a gradient, the update happened once
    frozen = [k for k in P if k not in ref]
    assert frozen and all(float(m.store.g(k).abs().max()) == 0.0 for k in frozen)
    assert opt.global_step == 1 and int(opt.state_dict()["state"][0]["step"]) == 1


def test_three_step_curve_tracks_the_oracle(tiny, b4):
    a, oarch, P = tiny
    Pr, state = {k: v.clone() for k, v in P.items()}, {}
    m, opt, r = make(a, P, micro_batches=2)
    mp, _, rp = make(a, P)
    for b in b4[0]:
        r1, r2, _ = O.train_step(Pr, b, oarch, state)
        out = r.step(b)
        rp.step(b)
        assert abs(float(out["loss1"]) - r1) < 1e-2 and abs(float(out["loss2"]) - r2) < 1e-2, (float(out["loss1"]), r1, float(out["loss2"]), r2)
    _, frozen = O.param_groups(list(P.keys()), oarch)
    every = max(rel(m.store.p(k), Pr[k]) for k in P if k not in frozen)
    mar, mar_p = max(rel(m.store.p(k), Pr[k]) for k in KEYS), max(rel(mp.store.p(k), Pr[k]) for k in KEYS)
    print(f"\n   [margins] parameters rel-L2 after three steps (gate 2e-2): micro {mar:.3e}, plain {mar_p:.3e}; worst of every trainable "
          f"tensor, micro {every:.3e}")
    assert mar < 2e-2 and every < 2e-2, (mar, every)


def test_device_drawn_masks_concatenate(tiny, b4):
    from tvts_amd.step import split_batch
    a, oarch, P = tiny
    data = {k: v for k, v in b4[0][1].items() if k != "keep_ind"}
    data.update(mask_seed=1234, sample_offset=96)
    m, opt, r = make(a, P, micro_batches=2)
    whole = m.engine.prepare_batch(data)["keep"]
    parts = [m.engine.prepare_batch(c)["keep"] for c in split_batch(data, 2)]
    same_bits(torch.cat(parts), whole, "the chunks' keep tables against the unsplit batch's")
    assert not torch.equal(parts[0], parts[1])
    m1, _, r1 = make(a, P)
    o1, o2 = r1.step(data), r.step(data)
    assert abs(float(o1["loss1"]) - float(o2["loss1"])) < 1e-2 and abs(float(o1["loss2"]) - float(o2["loss2"])) < 1e-2
    check_grads(m.store, grads_of(m1, [k for k in P if m1.engine.requires_grad[k]]))


def _short_captions(batch, oarch):
    """captions of different lengths (every other row cut to 5 tokens), so that the packed tower has something to pack"""
    t = batch["text"].clone()
    t[1::2, 4] = oarch["vocab"] - 1
    t[1::2, 5:] = 0
    return dict(batch, text=t)


def _u8(batch, oarch):
    g = torch.Generator().manual_seed(7)
    B, T, img = batch["video"].shape[0], batch["video"].shape[1], oarch["image"]
    return dict(batch, video=torch.randint(0, 256, (B, T, img + 6, img + 9, 3), generator=g, dtype=torch.uint8),
                crop=torch.stack([torch.arange(B) % 7, (3 * torch.arange(B)) % 10], 1))


@pytest.mark.parametrize("option", ["clip_grad", "recompute", "text_packed", "uint8"])
def test_options_against_the_same_option_unsplit(tiny, b4, option):
    """n = 2 beside n = 1 under the same option, at the oracle gates: |d loss| < 1e-2, check_grads over every trainable tensor with the
    n = 1 run's gradient as the reference"""
    from tvts_amd import arch as A
    a, oarch, P = tiny
    batch, kw = b4[0][0], {}
    if option == "clip_grad":
        norm = float(R.flat(b4[1][2]).norm())
        kw = dict(clip_grad=0.5 * norm)
        assert min(1.0, kw["clip_grad"] / (norm + 1e-6)) < 0.9  # the oracle's coefficient: clipping is active by construction
    elif option == "recompute":
        a = A.small_arch(recompute="block")
    elif option == "text_packed":
        a, batch = A.small_arch(text_packed=True), _short_captions(batch, oarch)
    else:
        batch = _u8(batch, oarch)
    m1, opt1, r1 = make(a, P, **kw)
    m2, opt2, r2 = make(a, P, micro_batches=2, **kw)
    o1, o2 = r1.step(batch), r2.step(batch)
    torch.cuda.synchronize()
    d1, d2 = abs(float(o1["loss1"]) - float(o2["loss1"])), abs(float(o1["loss2"]) - float(o2["loss2"]))
    names = [k for k in P if m1.engine.requires_grad[k]]
    print(f"\n   [{option}] |d loss1| {d1:.2e} |d loss2| {d2:.2e} (gate 1e-2); gradient rel-L2 n = 2 vs n = 1 {rel(m2.store.grad, m1.store.grad):.2e}; "
          f"parameters {max(rel(m2.store.p(k), m1.store.p(k)) for k in names):.2e} (gate 2e-2)")
    assert d1 < 1e-2 and d2 < 1e-2
    check_grads(m2.store, grads_of(m1, names))
    assert max(rel(m2.store.p(k), m1.store.p(k)) for k in names) < 2e-2
    if option == "clip_grad":
        n1, n2 = float(o1["grad_norm"]), float(o2["grad_norm"])
        assert abs(n2 - n1) < 1e-2 * n1 and float(r2.norm_coef[1]) < 0.9 and abs(float(r2.norm_coef[1]) - float(r1.norm_coef[1])) < 1e-2
        l1, l2, ref = b4[1]
        assert abs(n2 - float(R.flat(ref).norm())) < 1e-2 * float(R.flat(ref).norm())
    if option == "recompute":
        assert m2.engine.recompute == "block" and m2.engine.recompute_count > 0
    if option == "text_packed":
        assert m2.engine.text_packed


def test_overflow_in_the_last_chunk_skips_the_step(tiny, b4):
    """skip_nonfinite, the NaN pixel in the LAST clip: the bad value arrives with the last chunk only, after the other chunk's
    embeddings are cached -- every bit of the state is kept and `skipped` is 1; the next finite step updates"""
    a, oarch, P = tiny
    m, opt, r = make(a, P, micro_batches=2, skip_nonfinite=True)
    r.step(b4[0][0])
    snap = snapshot(m)
    assert int(r.skipped.item()) == 0 and int(opt.step_dev.item()) == 1
    out = r.step(G.nan_pixel(b4[0][1], oarch, sample=3))
    torch.cuda.synchronize()
    assert not math.isfinite(float(out["grad_norm"])) and int(r.skipped.item()) == 1 and int(opt.step_dev.item()) == 1
    same_state(m, snap, "after the bad step")
    r.step(b4[0][2])
    torch.cuda.synchronize()
    assert int(r.skipped.item()) == 1 and int(opt.step_dev.item()) == 2 and bool(torch.isfinite(m.store.flat).all())
    assert not torch.equal(bits(m.store.flat), bits(snap["flat"]))


def test_e4m3_weight_gradients(tiny):
    """small_h with e4m3 weight gradients, B = 4, n = 2, two steps (step 1 calibrates per token, step 2 runs per tensor).  The amax
    accumulators take a maximum, so the scales end_step forms are those of the n = 1 run bit for bit WHERE both runs start from the
    same weights: after step 1 at any learning rate, and after both steps at learning rate 0 (with an update in between the two
    runs' weights differ in their last bits -- the gradients are the same sums in another order -- and the step-2 maxima with them;
    that difference is printed).  Losses against the oracle at the e4m3 step tests' gate (3 % + 1e-2,
    test_training_curve_fp8_dgrad_tracks_oracle), parameters at 2e-2."""
    from tvts_amd import arch as A
    a = A.small_arch_h(width=640, heads=8, fp8_wgrad=True)
    oarch = O.tiny_arch(**a)
    P = O.synth_params(oarch, seed=33)
    batches = [O.synth_batch(oarch, B=4, T=2, seed=50 + i, caption_len=8) for i in range(2)]

    def two_steps(lr_mul, n):
        m, opt, r = make(a, P, lr_mul=lr_mul, micro_batches=n)
        scales, losses = [], []
        for b in batches:
            out = r.step(b)
            torch.cuda.synchronize()
            nn = len(m.engine._f8_ids)
            scales.append(m.engine._f8_scale[:nn].clone())
            losses.append((float(out["loss1"]), float(out["loss2"])))
        assert m.engine._f8_tensor_mode and nn == 12 * oarch["layers"] and float(m.engine._f8_amax.abs().max()) == 0.0
        return m, scales, losses
    m1, s1, l1 = two_steps(1.0, 1)
    m2, s2, l2 = two_steps(1.0, 2)
    same_bits(s2[0], s1[0], "the scales behind the calibration step")
    print(f"\n   [e4m3] scales after step 2 at lr > 0: rel diff n = 2 vs n = 1 {rel(s2[1], s1[1]):.2e}, equal {int((s2[1] == s1[1]).sum())} of {s1[1].numel()}")
    _, z1, _ = two_steps(0.0, 1)
    _, z2, _ = two_steps(0.0, 2)
    for i in range(2):
        same_bits(z2[i], z1[i], f"lr 0: the scales after step {i + 1}")
    assert bool((z2[1] > 0).all()) and bool(torch.isfinite(z2[1]).all())
    Pr, state = {k: v.clone() for k, v in P.items()}, {}
    _, frozen = O.param_groups(list(P.keys()), oarch)
    for i, b in enumerate(batches):
        r1, r2, _ = O.train_step(Pr, b, oarch, state)
        tot, ref = l2[i][0] + l2[i][1], r1 + r2
        print(f"   [e4m3] step {i + 1}: loss n = 2 {tot:.5f}, n = 1 {l1[i][0] + l1[i][1]:.5f}, oracle {ref:.5f}")
        assert abs(tot - ref) < 0.03 * abs(ref) + 1e-2, (tot, ref)
    worst = max(rel(m2.store.p(k), Pr[k]) for k in P if k not in frozen)
    print(f"   [e4m3] parameters rel-L2 against the oracle after two steps: n = 2 {worst:.3e}, n = 1 "
          f"{max(rel(m1.store.p(k), Pr[k]) for k in P if k not in frozen):.3e} (gate 2e-2)")
    assert worst < 2e-2


def test_named_refusals(tiny, b4):
    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.step import StepRunner
    from test_train_guard_gpu import ARGS
    a, oarch, P = tiny
    for bad in (0, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="micro_batches .* must be an int >= 1"):
            make(a, P, micro_batches=bad)
    with pytest.raises(RuntimeError, match=r"micro_batches=2\) cannot be combined with adamw_ranges / TVTS_ADAMW_RANGES=1"):
        make(A.small_arch(adamw_ranges=True), P, micro_batches=2)
    m = TVTSv2Base(ARGS, arch=a)
    m.load_state_dict(P, strict=True)
    with pytest.raises(RuntimeError, match=r"micro_batches=2\) needs the fused optimizer .* got AdamW"):
        StepRunner(m, torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4), micro_batches=2)
    _, _, r = make(a, P, micro_batches=3)
    with pytest.raises(ValueError, match="micro_batches 3 does not divide the batch of 4 clips"):
        r.step(b4[0][0])
    with pytest.raises(ValueError, match="prepares its chunks itself"):
        r.step(b4[0][0], pb=r.eng.prepare_batch(b4[0][0]))
    make(A.small_arch(adamw_ranges=True), P, micro_batches=1)[2].step(b4[0][0])  # n = 1 refuses nothing


def test_v1_engine_is_refused():
    """n > 1 on the v1 engine: not built (its text dropout seed advances per forward, it has no forward-only encoders)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd.step import StepRunner
    eng = types.SimpleNamespace(arch=dict(family="v1"), grad_ready=None)
    store = types.SimpleNamespace(device=torch.device(DEV), grad=torch.zeros(8, device=DEV))
    model = types.SimpleNamespace(engine=eng, store=store)
    opt = types.SimpleNamespace(chunk_group=None, begin_ranges=None)
    with pytest.raises(NotImplementedError, match="not built for the v1 engine"):
        StepRunner(model, opt, micro_batches=2)
    assert StepRunner(model, opt, micro_batches=1).micro_batches == 1


def test_trainer_config_key(tiny, tmp_path):
    """config['trainer']['micro_batches'] = 2 reaches the runner; one epoch over the two alternating loaders (YT-Temporal with the
    sorting loss, WebVid without) takes the plain trainer's number of updates and stays finite.  The distance to the plain trainer's
    parameters is PRINTED, not gated: this trainer fixture runs at 30 x the learning rate, where Adam's first updates are close to
    lr * sign(g) and an element whose gradient is rounding noise moves by a whole step in either direction -- measured 2.9e-2 rel-L2
    on the worst tensor after six updates, with per-step gradients that agree to 1e-7 (test_options_against_the_same_option_unsplit);
    the step's parity gates are the tests above, at the reference's learning rates."""
    from test_train_guard_gpu import build_trainer
    for d in ("m", "p"):
        (tmp_path / d).mkdir()
    tr_m, m_m = build_trainer(tmp_path / "m", 1, keys=dict(micro_batches=2))
    tr_p, m_p = build_trainer(tmp_path / "p", 1)
    assert tr_m.runner.micro_batches == 2 and not tr_m.replay.usable and tr_p.runner.micro_batches == 1
    tr_m.train(); tr_p.train()
    torch.cuda.synchronize()
    assert tr_m.optimizer.global_step == tr_p.optimizer.global_step > 0 and bool(torch.isfinite(m_m.store.flat).all())
    names = [k for k in m_p.engine.requires_grad if m_p.engine.requires_grad[k]]
    worst = max(rel(m_m.store.p(k), m_p.store.p(k)) for k in names)
    print(f"\n   [trainer] parameters rel-L2 micro_batches = 2 against the plain trainer after one epoch, worst tensor: {worst:.3e}")


def test_graph_replay_steps_eagerly(tiny, b4, monkeypatch):
    from tvts_amd.step import GraphReplay
    monkeypatch.setenv("TVTS_TRAINER_GRAPH", "1")
    a, oarch, P = tiny
    m, opt, r = make(a, P, micro_batches=2)
    me, opte, re_ = make(a, P, micro_batches=2)
    rep = GraphReplay(r)
    for _ in range(3):
        o, oe = rep.step(b4[0][0]), re_.step(b4[0][0])
        same_bits(o["loss1"], oe["loss1"], "loss1")
    assert not rep.usable and rep.eager == 3 and rep.captures == 0 and rep.replays == 0
    same_state(m, snapshot(me), "GraphReplay over a micro-batched runner against the runner")
    assert opt.global_step == 3
    assert GraphReplay(make(a, P)[2]).usable  # (n = 1 with the switch on still captures)
