"""The v1 forward-only path (run with -m gpu): its kernels per element (first-row query attention, the uint8 / channel-major tubelet
gathers, the label-matched video-to-video ranks), the encoders TVTS.encode_video / encode_text against the v1 oracle and against the
eval-mode training forward, their isolation from the training step (buffers and the dropout seed), and the downstream
VisionTransformer against the outputs of the reference's own classes (tests/golden/v1_downstream.npz,
tests/golden/make_golden_v1_downstream.py)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
import v1_downstream_synth as S  # noqa: E402
from v1_gather_ref import MEAN, STD, im2col_ref as _im2col_ref, normalise_u8  # noqa: E402
from oracle import tvts_v1_oracle as V  # noqa: E402  (checker only)

DEV = "cuda:0"
ARGS = types.SimpleNamespace(local_rank=0, rank=0, world_size=1)
HEADS = 3  # an odd count: a wrong head-column stride cannot land on another head's slice of the same row
BF16 = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def min_cos(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float(torch.nn.functional.cosine_similarity(a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1), dim=1).min())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ------------------------------------------------------------------------------------------------ 1. first-row query attention
def _first_row_case(K, S, dh, kv):
    """one call with lse2 and one without on NaN-filled outputs -> the worst (row, head) error of the B query rows"""
    B = 2 if kv is None else len(kv)
    W = HEADS * dh
    g = torch.Generator().manual_seed(7000 + 10 * S + dh + (0 if kv is None else 1))
    qkv = torch.randn(B * S, 3 * W, generator=g).bfloat16().to(DEV)
    kvd = None if kv is None else torch.tensor(kv, dtype=torch.int32, device=DEV)
    what = f"first[S {S}, dh {dh}, kv_len {kv}]"
    obuf, out = KB.guarded(B * S, W, BF16, DEV)
    lse = torch.full((B * S, HEADS), NAN, device=DEV)
    before = bits(out).clone()
    K.attn_fwd_first(qkv, kvd, out, lse, B=B, heads=HEADS, S=S, head_dim=dh)
    obuf2, out2 = KB.guarded(B * S, W, BF16, DEV)
    K.attn_fwd_first(qkv, kvd, out2, None, B=B, heads=HEADS, S=S, head_dim=dh)
    torch.cuda.synchronize()
    KB.check_guards(obuf, B * S, W, what + " out"); KB.check_guards(obuf2, B * S, W, what + " out (no lse2)")
    rows = torch.zeros(B * S, dtype=torch.bool, device=DEV)
    rows[torch.arange(B, device=DEV) * S] = True
    assert torch.equal(bits(out)[~rows], before[~rows]), f"{what}: out was written outside the rows b * S"
    assert torch.isnan(lse[~rows]).all(), f"{what}: lse2 was written outside the rows b * S"
    assert torch.equal(bits(out2), bits(out)), f"{what}: lse2 = NULL changes the output bits"
    ro, rl, _ = KB.attn_fwd_ref(qkv.view(B, S, 3 * W), HEADS, dh, kv_len=kvd)
    ro, rl = ro.reshape(B * S, W), rl.reshape(B * S, HEADS)
    got = torch.where(rows[:, None], out.double(), ro)  # (the other rows take the reference's values: a failure names the token row)
    w, wc = KB.rows_check(got, ro, KB.ATTN_ROW_TOL["out"], HEADS, B, S, what + " out")
    KB.assert_within(lse[rows], rl[rows], KB.LSE2_TOL, what + " lse2")
    return max(w, wc)


@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("S", [1, 16, 17, 63, 64, 65, 130])
def test_first_row_attention_per_row(K, S, dh):
    """tvts_attn_fwd_first: one query per sequence at token row 0.  One key tile or fewer (S <= 64) leaves three of the block's
    four waves without work, 64 / 65 is the four-tile boundary of the first round, 130 a partial third tile.  Key counts: all S
    keys; one sequence per kv_len in {1, 2, 16, 17, 63, 64, 65, S} (capped at S), one entry above S and one of 0 (the clamp)."""
    worst = _first_row_case(K, S, dh, None)
    lens = sorted({min(v, S) for v in (1, 2, 16, 17, 63, 64, 65, S)})
    worst = max(worst, _first_row_case(K, S, dh, lens + [S + 7, 0]))
    KB.bound_line(f"v1_infer first-row attention[S {S}, dh {dh}] out (per-row rel)", worst)


@pytest.mark.parametrize("S", [1, 17, 64, 65, 130])
def test_attn_fwd_len_without_lse_gives_the_same_bits(K, S):
    """the forward-only DistilBERT blocks call tvts_attn_fwd_len with lse2 = NULL: fwd_impl is shared with tvts_attn_fwd, whose
    kernels skip the store -- the output bits are those of the call with lse2"""
    lens = sorted({min(v, S) for v in (1, 2, 16, 17, 63, 64, 65, S)}) + [0]
    B, W = len(lens), HEADS * 64
    g = torch.Generator().manual_seed(7500 + S)
    qkv = torch.randn(B * S, 3 * W, generator=g).bfloat16().to(DEV)
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o1, o2 = (torch.full((B * S, W), NAN, dtype=BF16, device=DEV) for _ in range(2))
    lse = torch.full((B * S, HEADS), NAN, device=DEV)
    K.attn_fwd_len(qkv, kv, o1, lse, B=B, heads=HEADS, S=S)
    K.attn_fwd_len(qkv, kv, o2, None, B=B, heads=HEADS, S=S)
    torch.cuda.synchronize()
    assert torch.isfinite(o1.float()).all() and torch.equal(bits(o1), bits(o2))


# ------------------------------------------------------------------------------------------------ 2. tubelet gathers
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("p", [16, 8])
def test_tube_gathers_bit_exact(K, p, full):
    """tvts_patch_gather_tube_u8 and tvts_patch_gather_tube_cm against the host and against the existing fp32 kernel, bit for bit.
    37 x 39 frames: centre-crop margins 5 and 7, whose halves 2.5 and 3.5 round half-to-even to 2 and 4."""
    B, tubes, tb, img, H0, W0 = 2, 3, 2, 32, 37, 39
    T, ppf = tubes * tb, (img // p) ** 2
    n = ppf if full else (3 if p == 16 else 5)
    g = torch.Generator().manual_seed(8000 + p + int(full))
    frames = torch.randint(0, 256, (B, T, H0, W0, 3), generator=g, dtype=torch.uint8)
    keep = torch.stack([torch.stack([torch.randperm(ppf, generator=g)[:n] for _ in range(tubes)]) for _ in range(B)])
    assert n == 1 or any(not torch.equal(keep[b, t], keep[b, t].sort().values) for b in range(B) for t in range(tubes))
    keep_d = keep.to(torch.int32).to(DEV)
    Kc, M = 3 * tb * p * p, B * tubes * n
    for name, crop in (("centre", None), ("corners", [[0, 0], [H0 - img, W0 - img]])):
        offs = [[2, 4]] * B if crop is None else crop
        cut = torch.stack([frames[b, :, y:y + img, x:x + img] for b, (y, x) in enumerate(offs)])
        video = normalise_u8(cut).permute(0, 1, 4, 2, 3).contiguous()  # ClipToTensor + Normalize, [B, T, 3, H, W]
        want = _im2col_ref(video, keep, tb, p).bfloat16()
        what = f"tube gather[p {p}, n {n}, crop {name}]"
        crop_d = None if crop is None else torch.tensor(crop, dtype=torch.int32, device=DEV)
        ubuf, u = KB.guarded(M, Kc, BF16, DEV)
        K.patch_gather_tube_u8(frames.to(DEV), keep_d, u, B=B, tubes=tubes, tubelet=tb, n=n, img=img, patch=p, crop=crop_d)
        f = torch.full((M, Kc), NAN, dtype=BF16, device=DEV)
        K.patch_gather_tube(video.to(DEV), keep_d, f, B=B, tubes=tubes, tubelet=tb, n=n, img=img, patch=p)
        cbuf, c = KB.guarded(M, Kc, BF16, DEV)
        K.patch_gather_tube(video.permute(0, 2, 1, 3, 4).contiguous().to(DEV), keep_d, c, B=B, tubes=tubes, tubelet=tb, n=n, img=img,
                            patch=p, channel_major=True)
        torch.cuda.synchronize()
        KB.check_guards(ubuf, M, Kc, what + " u8"); KB.check_guards(cbuf, M, Kc, what + " channel-major")
        assert torch.equal(u.cpu(), want), what + ": uint8 kernel against the host"
        assert torch.equal(bits(u), bits(f)), what + ": uint8 kernel against the fp32 kernel on host-normalised frames"
        assert torch.equal(bits(c), bits(f)), what + ": channel-major kernel against the fp32 kernel"


# ------------------------------------------------------------------------------------------------ 3. video-to-video ranks
def _labels(N, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, 4, (N,), generator=g)
    lab[int(torch.randint(0, N, (1,), generator=g))] = 9  # a class with a single member: its query's best is its own -1000
    return lab


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("N", [1, 2, 10, 11, 257, 1000])
def test_v2v_ranks_exact(K, N, ties):
    """tvts_v2v_ranks == numpy on the similarities the kernel read: whole matrix in one call and in chunks of 96 query rows (q0 != 0,
    a ragged last chunk), ld > N, the input unchanged, nothing written past the nq ranks.  ties: scores on a grid of 1/4, so that
    equal scores are common and the strict > of the definition is exercised."""
    g = torch.Generator().manual_seed(9000 + N + int(ties))
    lab = _labels(N, 9100 + N)
    full = torch.randn(N, N + 5, generator=g)
    if ties:
        full = torch.round(full * 4) / 4
    s = full[:, :N].numpy().copy()
    np.fill_diagonal(s, -1000)
    want = S.defined_ranks(s, lab.numpy())
    assert want[int((lab == 9).nonzero()[0])] == N - 1  # the singleton's query: every other video scores above -1000
    lab_d = lab.to(torch.int32).to(DEV)
    for chunk in sorted({N, min(N, 96)}):
        got = torch.full((N + 2,), NAN, device=DEV)
        for q0 in range(0, N, chunk):
            nq = min(chunk, N - q0)
            sims = full[q0:q0 + nq].to(DEV)
            keep = sims.clone()
            K.v2v_ranks(sims, q0, lab_d, got[q0:q0 + nq], N=N)
            assert torch.equal(bits(sims), bits(keep)), "tvts_v2v_ranks modified its input"
        torch.cuda.synchronize()
        assert torch.isnan(got[N:]).all()
        assert np.array_equal(got[:N].cpu().numpy().astype(np.float64), want), (N, chunk, ties)


def test_v2v_protocol_reproduces_the_fixture(K, golden):
    from tvts_amd.downstream import zero_shot as Z
    f = golden("v1_downstream")
    feats, labels = S.v2v_data(int(f["v2v_seed"]))
    for chunk in (2048, 16):
        ranks = Z.v2v_ranks(feats.to(DEV), labels.to(DEV), chunk=chunk).cpu()
        assert Z.recall_at(ranks) == [float(v) for v in f["v2v_recall"]], chunk
        hit = f["v2v_ranks"] < 10
        assert np.array_equal(ranks.numpy()[hit], f["v2v_ranks"][hit]) and bool((ranks.numpy()[~hit] >= 10).all())


# ------------------------------------------------------------------------------------------------ 4. encoders against the oracle
def small():
    """the small() pairing of tests/test_v1_gpu.py: the engine's reduced v1 architecture and the oracle's arch dict of the same sizes"""
    from tvts_amd import arch as A
    a = A.small_arch_v1()
    return a, V.tiny_arch(**{k: a[k] for k in V.tiny_arch() if k in a and k != "name"})


def build(a, P, dropout=0.0):
    from tvts_amd.model.model_dist_TVTS import TVTS
    m = TVTS(ARGS, arch=dict(a, text_dropout=dropout))
    m.load_state_dict(P, strict=True)
    return m


def captions(oa, lens, seed):
    """right-padded captions of the given lengths, [CLS] first and [SEP] last (V.synth_batch's format)"""
    g = torch.Generator().manual_seed(seed)
    N, L = len(lens), max(lens)
    ids, mask = torch.zeros(N, L, dtype=torch.int64), torch.zeros(N, L, dtype=torch.int64)
    for r, n in enumerate(lens):
        ids[r, 0], ids[r, n - 1] = oa["vocab"] - 2, oa["vocab"] - 1
        ids[r, 1:n - 1] = torch.randint(1, oa["vocab"] - 2, (n - 2,), generator=g)
        mask[r, :n] = 1
    return {"input_ids": ids, "attention_mask": mask}


@pytest.fixture(scope="module")
def small_model(K):
    a, oa = small()
    P = V.synth_params(oa, seed=5)
    return build(a, P).eval(), a, oa, P


def _gates(got, train, ref, what):
    """the project's gates for this model (tests/test_v1_gpu.py:244-245) and the encoder-against-training-forward rule of
    tests/test_infer_gpu.py:83: the encoder may not be further from the oracle than 1.25 x the training forward + 1e-4"""
    e, e_train, c = rel(got, ref), rel(train, ref), min_cos(got, ref)
    print(f"\n   [{what}] rel {e:.3e} (training forward {e_train:.3e}), worst-row cosine {c:.7f}")
    assert e < 0.02 and c > 0.9995, (what, e, c)
    assert e <= 1.25 * e_train + 1e-4, (what, e, e_train)


@pytest.mark.parametrize("masked", [False, True])
def test_encode_video_against_the_oracle(small_model, masked):
    m, a, oa, P = small_model
    B, T, tubes, ppf = 3, 8, 4, 16
    g = torch.Generator().manual_seed(41 + int(masked))
    video = torch.randn(B, T, 3, a["image"], a["image"], generator=g)
    if masked:  # one mask per tube, n = 8: S = 33
        keep = torch.stack([torch.stack([torch.randperm(ppf, generator=g)[:8] for _ in range(tubes)]) for _ in range(B)])
        arg = keep
    else:       # every patch of every tube: S = 65
        keep, arg = torch.arange(ppf).view(1, 1, ppf).expand(B, tubes, ppf), None
    rtok, remb = V.compute_video(P, video, keep, oa)
    ttok, temb = m.compute_video(video, keep)
    emb = m.encode_video(video, arg)
    feat = m.encode_video(video, arg, project=False)
    assert emb.shape == (B, a["embed"]) and feat.shape == (B, a["width"])
    _gates(emb, temb, remb, f"encode_video S {1 + tubes * keep.shape[2]}")
    _gates(feat, ttok[:, 0], rtok[:, 0], f"encode_video(project=False) S {1 + tubes * keep.shape[2]}")
    if masked:  # [tubes, n]: one mask for every clip
        one = m.encode_video(video, keep[1])
        assert torch.equal(bits(one[1]), bits(emb[1]))


def test_encode_video_uint8_is_the_fp32_path_bit_for_bit(small_model):
    m, a, oa, P = small_model
    B, T, img, H0, W0 = 3, 8, a["image"], a["image"] + 3, a["image"] + 6   # margins 3 and 6: centre-crop offsets 2 (1.5 -> 2) and 3
    g = torch.Generator().manual_seed(43)
    frames = torch.randint(0, 256, (B, T, H0, W0, 3), generator=g, dtype=torch.uint8)
    mean, std = torch.tensor(MEAN).view(1, 1, 1, 1, 3), torch.tensor(STD).view(1, 1, 1, 1, 3)
    video = ((frames[:, :, 2:2 + img, 3:3 + img].float() / 255 - mean) / std).permute(0, 1, 4, 2, 3).contiguous()
    for project in (True, False):
        assert torch.equal(bits(m.encode_video(frames, project=project)), bits(m.encode_video(video, project=project)))


def test_encode_text_against_the_oracle(small_model):
    m, a, oa, P = small_model
    text = captions(oa, [3, 7, 13], seed=44)
    rb, rt = V.compute_text(P, text, oa)
    tb, tt = m.compute_text(text)
    got = m.encode_text(text)
    assert got.shape == (3, a["embed"])
    _gates(got, tt, rt, "encode_text lengths 3 / 7 / 13")
    # the padding behind the longest caption is cut, as prepare_batch does
    wide = {k: torch.cat([v, torch.zeros(3, 4, dtype=v.dtype)], 1) for k, v in text.items()}
    assert torch.equal(bits(m.encode_text(wide)), bits(got))


def test_encoder_argument_checks(small_model):
    m, a, oa, P = small_model
    img = a["image"]
    with pytest.raises(ValueError):
        m.encode_video(torch.zeros(1, 3, 3, img, img))                       # T is not a multiple of the tubelet
    with pytest.raises(ValueError):
        m.encode_video(torch.zeros(1, a["num_frames"] + 2, 3, img, img))     # T > num_frames
    with pytest.raises(ValueError):
        m.encode_video(torch.zeros(1, 3, 4, img, img))                       # channel-major where [B, T, 3, H, W] is expected
    with pytest.raises(ValueError):
        m.encode_video(torch.zeros(1, 4, 3, img, img, dtype=torch.uint8))    # uint8 must be [B, T, H, W, 3]
    with pytest.raises(ValueError):
        m.encode_video(torch.zeros(1, 4, 3, img, img), torch.zeros(3, 4, dtype=torch.int64))  # 3 masks for 2 tubes
    with pytest.raises(IndexError):
        m.encode_video(torch.zeros(1, 4, 3, img, img), torch.full((2, 4), 16))
    with pytest.raises(ValueError):
        m.encode_text({"input_ids": torch.ones(1, 4, dtype=torch.int64), "attention_mask": torch.tensor([[1, 0, 1, 0]])})
    with pytest.raises(IndexError):
        m.encode_text({"input_ids": torch.full((1, 4), a["vocab"]), "attention_mask": torch.ones(1, 4, dtype=torch.int64)})
    with pytest.raises(NotImplementedError):
        m.engine.encode_text_packed(None, None, 1, 4)


# ------------------------------------------------------------------------------------------------ 5. isolation, the seed rule
def test_encoders_leave_the_training_step_and_the_seed_alone(K):
    """the construction of tests/test_infer_gpu.py::test_encoders_leave_the_training_step_alone with the training-mode text tower
    (dropout 0.1): encoder calls of other shapes between construction and a training step change neither the step's losses nor one
    bit of its flat gradient -- which they would if they touched a buffer of the step or advanced the mask seed"""
    from tvts_amd.engine import LossHead
    a, oa = small()
    P = V.synth_params(oa, seed=7)
    batch = V.synth_batch(oa, B=4, T=6, seed=8, caption_len=13)

    def step(m):
        m._fresh_shadows(); m._sync_requires_grad()
        eng = m.engine
        pb = eng.prepare_batch(batch)
        m.store.grad.zero_()
        te, ve, pred = eng.forward(pb)
        head = LossHead(m.store.device)
        l1, dv, dt = head.contrastive(ve, te)
        l2, dp = head.sorting(pred, batch["label"].reshape(-1).to(torch.int32).to(DEV))
        eng.backward(dt, dv, dp)
        torch.cuda.synchronize()
        return l1.clone(), l2.clone(), m.store.grad.clone()

    used = build(a, P, dropout=0.1)
    assert used.training and used.engine.text_drop_p == 0.1
    text = captions(oa, [5, 9, 4, 11, 3], seed=45)
    seed0 = used.engine.drop_seed.clone()
    t_train = used.encode_text(text)
    used.eval()
    t_eval = used.encode_text(text)
    used.train()
    assert torch.equal(bits(t_train), bits(t_eval)), "encode_text applied dropout in train() mode"
    e1 = used.encode_video(batch["video"][:3, :4])
    used.encode_video(batch["video"][:2], batch["keep_ind"][:2])
    assert torch.isfinite(e1).all() and e1.shape == (3, a["embed"])
    assert torch.equal(used.engine.drop_seed, seed0), "an encoder call advanced the dropout seed"
    assert not used.engine.buf, "an encoder call created a buffer of the training step"
    got = step(used)
    fresh = build(a, P, dropout=0.1)
    want = step(fresh)
    assert not torch.equal(used.engine.drop_seed, seed0)  # (the step itself does advance it)
    for g_, w_, what in zip(got, want, ("loss1", "loss2", "gradients")):
        assert torch.equal(bits(g_), bits(w_)), what


# ------------------------------------------------------------------------------------------------ 6. the downstream class
def test_downstream_class_against_the_reference_fixture(K, golden):
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    f = golden("v1_downstream")
    C = int(f["classes_tiny"])
    sd = S.synth_state(S.TINY, int(f["seed_tiny"]), C)
    m = VisionTransformer(num_classes=C, **S.TINY)
    keys = [str(k) for k in f["keys"]]
    assert list(m.state_dict().keys()) == keys
    assert [str(tuple(v.shape)) for v in m.state_dict().values()] == [str(s) for s in f["shapes_tiny"]]
    assert not any(p.requires_grad for p in m.parameters())
    assert not [k for k in keys if k.startswith(("text_model", "pred_model", "txt_proj", "vid_proj"))]
    m.load_state_dict(sd, strict=True)
    x = S.synth_clip(S.TINY, int(f["B_tiny"]), int(f["T_tiny"]), int(f["clip_seed_tiny"]))
    feat = m.forward_features(x)
    e, c = rel(feat, f["feats_tiny"]), min_cos(feat, f["feats_tiny"])
    print(f"\n   [downstream tiny] features against the reference class: rel {e:.3e}, worst-clip cosine {c:.7f}")
    assert feat.shape == (int(f["B_tiny"]), S.TINY["embed_dim"]) and e < 0.02 and c > 0.9995, (e, c)
    logits = m(x)
    assert rel(logits, f["logits_tiny"]) < 0.02
    # the head alone: logits against a float64 head on the features the model returned.  tvts_gemm_small_f32 multiplies fp32 by
    # fp32, so a term costs up to two roundings (product and addition; one where the compiler fuses them): the any-order
    # summation bound of KB.gemm_bound with 2 K roundings
    W = S.TINY["embed_dim"]
    ref, Sabs = KB.gemm_ref(feat.cpu(), sd["head.weight"], bias=sd["head.bias"])
    worst = KB.assert_within(logits.cpu(), ref, KB.gemm_bound(ref, Sabs, 2 * W, torch.float32), "downstream head")
    KB.bound_line("v1_infer downstream head (|err| / bound)", worst)
    # the zero-shot class (no head) returns the features; a pretrain checkpoint loads through the script's key filter
    pre = {"module.video_model." + k: v for k, v in sd.items() if not k.startswith("head.")}
    pre["module.text_model.embeddings.LayerNorm.weight"] = torch.ones(4)
    pre["module.vid_proj.0.weight"] = torch.ones(4, 4)
    z = VisionTransformer.from_pretrain({"state_dict": pre}, **S.TINY)
    assert list(z.state_dict().keys()) == keys[:-2]
    assert torch.equal(bits(z(x)), bits(feat))
    missing = z.load_state_dict(sd, strict=False)  # as run_class_zero.py:340 loads
    assert not missing.missing_keys and sorted(missing.unexpected_keys) == ["head.bias", "head.weight"]
    for kw in (dict(qkv_bias=False), dict(representation_size=64), dict(embed_dim=128, num_heads=4), dict(embed_dim=160, num_heads=2)):
        with pytest.raises((ValueError, NotImplementedError)):
            VisionTransformer(**dict(S.TINY, **kw))
    with pytest.raises(ValueError):
        m.forward_features(x.permute(0, 2, 1, 3, 4).contiguous())  # [B, T, 3, H, W] is the pretrain model's layout, not this class's


# ------------------------------------------------------------------------------------------------ 7. real size, once
def _peak(fn, B, v):
    fn(v[:B])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn(v[:B])
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def test_real_size_once(K, golden):
    """dim 768, depth 12, 16 frames of 224 x 224, every patch: S = 1569.  The downstream class against the reference class's
    features; TVTS.encode_video against the eval-mode training forward on the same weights; memory per clip of both."""
    from tvts_amd import arch as A
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    from tvts_amd.model.model_dist_TVTS import TVTS
    f = golden("v1_downstream")
    B, T = int(f["B_real"]), int(f["T_real"])
    sd = S.synth_state(S.REAL, int(f["seed_real"]), int(f["classes_real"]))
    x4 = S.synth_clip(S.REAL, 4, T, int(f["clip_seed_real"]))
    x = S.synth_clip(S.REAL, B, T, int(f["clip_seed_real"]))
    # the pretrain model with the same video tower (a short text tower and sort head: they take no part here)
    m = TVTS(ARGS, arch=dict(A.ARCH_V1, text_layers=1, vocab=64, max_pos=16, sort_depth=1)).eval()
    miss = m.load_state_dict({S.PREFIX + k: v for k, v in sd.items() if not k.startswith("head.")}, strict=False)
    assert not miss.unexpected_keys and not [k for k in miss.missing_keys if k.startswith(S.PREFIX)]
    ppf = 196
    keep = torch.arange(ppf).view(1, 1, ppf).expand(B, T // 2, ppf)
    v = x.permute(0, 2, 1, 3, 4).contiguous()
    ttok, temb = m.compute_video(v, keep)
    emb = m.encode_video(v)
    c = min_cos(emb, temb)
    print(f"\n   [v1 T=16 S=1569] worst per-clip cosine encode_video vs eval-mode training forward: {c:.7f}")
    assert c >= 0.9999, c
    d = VisionTransformer(num_classes=int(f["classes_real"]), **S.REAL)
    d.load_state_dict(sd, strict=True)
    feat = d.forward_features(x)
    _gates(feat, ttok[:, 0], f["feats_real"], "downstream real size, features against the reference class")
    assert rel(d(x), f["logits_real"]) < 0.02
    del d
    # memory per clip, B = 2 -> 4 (workspaces only grow: both measurements start from none)
    eng = m.engine
    v4 = x4.permute(0, 2, 1, 3, 4).contiguous().to(DEV)
    keep4 = keep[:1].expand(4, -1, -1)
    eng._inf.clear(); eng.buf.clear(); eng._back.clear(); eng._seen.clear()
    torch.cuda.empty_cache()
    p2 = _peak(lambda t: m.encode_video(t), 2, v4)
    enc = (_peak(lambda t: m.encode_video(t), 4, v4) - p2) / 2 / 1e6
    eng._inf.clear()
    torch.cuda.empty_cache()

    def train(t):
        with torch.no_grad():
            m.compute_video(t, keep4[:t.shape[0]])
    q2 = _peak(train, 2, v4)
    tr = (_peak(train, 4, v4) - q2) / 2 / 1e6
    print(f"\n   [v1 T=16 S=1569] encode_video peak growth {enc:.1f} MB per clip, eval-mode training forward {tr:.1f} MB per clip")
    assert enc <= tr / 8, (enc, tr)
