"""The forward-only encoders on the e4m3 architectures: the few-rows e4m3 linear kernel (tvts_rows_linear_fp8) against exact
arithmetic, the tail's quantised rows, encode_video against the oracle's e4m3 emulation and against the training forward of the same
model, the untouched text tower, the isolation from the training step (per-token and per-tensor regimes) and the multiple-choice
forward.  Shapes as in tests/test_model_gpu.py::test_fp8_forward_path*: every quantised K is a multiple of 128."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
from oracle import tvts_oracle as O  # noqa: E402  (checker only)

DEV = "cuda:0"
ARGS = types.SimpleNamespace(local_rank=0, rank=0, world_size=1)


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def cos_rows(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return torch.nn.functional.cosine_similarity(a, b, dim=-1)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def _arch(kind, **over):
    from tvts_amd import arch as A
    return A.small_arch(**over) if kind == "b" else A.small_arch_h(width=640, heads=8, **over)


def _model(a, seed):
    """(TVTSv2Base on the architecture `a`, its oracle architecture, the synthetic parameters both carry)"""
    from tvts_amd.model._common import TVTSv2Base
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    oarch = O.tiny_arch(**a)
    P = O.synth_params(oarch, seed=seed)
    m = TVTSv2Base(ARGS, arch=dict(a))
    m.load_state_dict(P, strict=True)
    return m, oarch, P


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("N", [64, 200])
@pytest.mark.parametrize("Kd", [64, 128, 512, 640])  # 64: the smallest K; 512: exactly one 512-deep chunk of the decoded rows
@pytest.mark.parametrize("R", [1, 3, 17])
def test_rows_linear_fp8_against_exact_arithmetic(K, R, Kd, N):
    """out = residual + bias + row_scale[r] * w_scale * (a8 @ w8^T): both operands decoded on the host, the product in float64, every
    element inside kernel_bounds.gemm_bound (e4m3-decoded operands with scales, bias and residual).  R = 17 takes two row tiles,
    N = 200 a ragged column tile (guard rows / columns stay untouched), K = 640 the four-steps-in-flight loop and its remainder;
    a8 is a strided row view (row stride 5 K); one row is all zeros under scale 0; bias / residual present and absent; two calls
    give the same bits."""
    g = torch.Generator(device=DEV).manual_seed(1000 * R + Kd + N)
    x = (torch.randn(R, 5 * Kd, generator=g, device=DEV) * 1.7).bfloat16()
    q_full = torch.full((R, 5 * Kd), 0x7F, dtype=torch.uint8, device=DEV)  # (e4m3 NaN bytes wherever the view does not reach)
    a8 = q_full[:, :Kd]
    _, rs = K.quantize_fp8_rows(x[:, :Kd], q=a8)
    w8, ws = K.quantize_fp8(torch.randn(N, Kd, generator=g, device=DEV) * 0.05)
    bias = torch.randn(N, generator=g, device=DEV)
    res = torch.randn(R, N, generator=g, device=DEV) * 2.0
    assert a8.stride(0) == 5 * Kd and bool((q_full[:, Kd:] == 0x7F).all())
    zero_rows = [None, R - 1] if R > 1 else [None, 0]
    worst = 0.0
    for z in zero_rows:
        if z is not None:
            a8[z].zero_()
            rs[z] = 0.0
        ad, wd = KB.decode_e4m3(a8.cpu().contiguous()), KB.decode_e4m3(w8.cpu())
        scale = rs[:R].double().cpu() * float(ws)
        for b, r in ((bias, res), (None, None), (bias, None), (None, res)):
            buf, out = KB.guarded(R, N, torch.float32, DEV)
            K.rows_linear_fp8(a8, rs, w8, ws, out, bias=b, residual=r)
            torch.cuda.synchronize()
            KB.check_guards(buf, R, N, "rows_linear_fp8")
            worst = max(worst, KB.check_gemm(out.cpu(), ad, wd, scale=scale, bias=None if b is None else b.cpu(),
                                             residual=None if r is None else r.cpu(),
                                             what=f"rows_linear_fp8 R={R} K={Kd} N={N} zero_row={z} bias={b is not None} res={r is not None}"))
            if z is not None:
                want = (0.0 if b is None else b) + (torch.zeros(N, device=DEV) if r is None else r[z])
                KB.assert_equal_bits(out[z].contiguous(), want.contiguous().float(), "the all-zero row under scale 0")
            buf2, out2 = KB.guarded(R, N, torch.float32, DEV)
            K.rows_linear_fp8(a8, rs, w8, ws, out2, bias=b, residual=r)
            KB.assert_equal_bits(out2.contiguous(), out.contiguous(), "second call")
    print(f"BOUND rows_linear_fp8[{R},{N},{Kd}] {worst:.4g} acc {KB.pop_acc_worst():.4g}")


def test_rows_linear_fp8_refuses_what_it_cannot_load(K):
    """K in whole 64-byte steps and 16-byte aligned rows, or an error: never a partial load"""
    a8 = torch.zeros(4, 192, dtype=torch.uint8, device=DEV)
    w8 = torch.zeros(32, 192, dtype=torch.uint8, device=DEV)
    rs, ws, out = torch.ones(4, device=DEV), torch.ones(1, device=DEV), torch.zeros(4, 32, device=DEV)
    K.rows_linear_fp8(a8, rs, w8, ws, out)
    with pytest.raises(K.HipError):
        K.rows_linear_fp8(a8[:, :96], rs, w8[:, :96].contiguous(), ws, out)     # K % 64
    with pytest.raises(K.HipError):
        K.rows_linear_fp8(a8[:, 8:136], rs, w8[:, :128].contiguous(), ws, out)  # rows that start off a 16-byte boundary


# ------------------------------------------------------------------------------------------------ shared models
@pytest.fixture(scope="module")
def small_fp8():
    return _model(_arch("b", fp8=True), seed=3)


@pytest.fixture(scope="module")
def h_fp8():
    return _model(_arch("h", fp8=True), seed=4)


# ------------------------------------------------------------------------------------------------ 2. the tail's e4m3 rows
def test_tail_rows_are_quantize_fp8_rows_of_the_cls_view(K, small_fp8):
    """The e4m3 rows the tail multiplies are tvts_quant_fp8_rows of the same bf16 rows: on the strided CLS view of a [B * S, W]
    operand (one row per clip, row stride S * W) the kernel writes the bytes and scales it writes for a contiguous copy of those
    rows; and what Engine.encode_video leaves in its workspaces agrees -- the e4m3 rows c_proj's tail multiplied are the
    quantisation of the bf16 rows c_fc wrote."""
    B, S, W = 5, 33, 256
    g = torch.Generator(device=DEV).manual_seed(11)
    x = (torch.randn(B * S, W, generator=g, device=DEV) * 3.0).bfloat16()
    x[2 * S].zero_()  # one all-zero CLS row
    view = x.view(B, S * W)[:, :W]
    q1, s1 = K.quantize_fp8_rows(view)
    q2, s2 = K.quantize_fp8_rows(view.contiguous())
    KB.assert_equal_bits(q1, q2, "bytes of the strided CLS rows")
    KB.assert_equal_bits(s1, s2, "scales of the strided CLS rows")
    m, oarch, P = small_fp8
    a = m.arch
    batch = O.synth_batch(oarch, B=3, T=3, seed=5, caption_len=11)
    m.encode_video(batch["video"])
    eng, Wd = m.engine, a["width"]
    h_c = eng._ib("hc", (3, 4 * Wd))                      # the bf16 rows c_fc wrote for the three CLS rows
    q_c = eng._ib("q8.%d" % (4 * Wd), (3, 4 * Wd), torch.uint8)
    rs_c = eng._ib("q8.row_scale", (3,), torch.float32)
    q3, s3 = K.quantize_fp8_rows(h_c.clone())
    KB.assert_equal_bits(q_c.clone(), q3, "bytes the c_proj tail multiplied")
    KB.assert_equal_bits(rs_c.clone(), s3, "scales the c_proj tail multiplied")
    assert float(s3.min()) > 0.0


# ------------------------------------------------------------------------------------------------ 3. against the oracle
@pytest.mark.parametrize("kind", ["b", "h"])
def test_encode_video_against_the_oracle_e4m3_emulation(kind, request):
    """encode_video at mask 0 (every patch kept) against the oracle's video embedding under fp8=True (quantise -> dequantise
    emulation of the six linear layers of every block, every row), with the e4m3 gates of test_fp8_forward_path: minimum row cosine
    > 0.999 and rel-L2 < 0.04; against the unquantised oracle cosine > 0.995."""
    m, oarch, P = request.getfixturevalue("small_fp8" if kind == "b" else "h_fp8")
    assert len(m.store.w8) == 0 or len(m.store.w8) == 6 * m.arch["layers"]
    batch = O.synth_batch(oarch, B=3, T=3, seed=5, caption_len=11)
    keep = torch.arange(O.patches_per_frame(oarch)).unsqueeze(0)
    with torch.no_grad():
        want, _ = O.video_tower(P, batch["video"], keep, oarch)
        want32, _ = O.video_tower(P, batch["video"], keep, dict(oarch, fp8=False))
    got = m.encode_video(batch["video"])
    assert len(m.store.w8) == 6 * m.arch["layers"]
    c, e, c32 = float(cos_rows(got, want).min()), rel(got, want), float(cos_rows(got, want32).min())
    print(f"\n   [margins, {m.arch['name']}] encode_video vs e4m3 oracle: min cosine {c:.6f} (gate 0.999), rel {e:.4f} (gate 0.04); "
          f"vs unquantised oracle: min cosine {c32:.6f} (gate 0.995)")
    assert c > 0.999 and e < 0.04, (c, e)
    assert c32 > 0.995, c32
    again = m.encode_video(batch["video"], keep)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 4. against the training forward
@pytest.mark.parametrize("kind,over,B,T", [("h", dict(image=224), 2, 2), ("b", {}, 3, 3)])
def test_encode_video_against_the_training_forward_of_the_same_model(kind, over, B, T):
    """encode_video against compute_video (the training forward under no_grad) of the SAME e4m3 model, per-clip cosine.  The H
    structure at 224 pixels has 256 patches per frame (112 < n + 1 <= 272): the full-frame SPACE kernel and its CLS merge run in
    front of the quantisers; the B-style model's 16 patches stay below that range.  The two passes differ by design in the last
    block's CLS rows: the encoder multiplies the e4m3 copies of attn.proj / mlp.c_proj there (what the oracle's emulation does for
    every row), the training step's hybrid stream carries its fp32 CLS rows through the bf16 shadows (Engine._cls_lin).
    Gate: the project's e4m3 cosine, 0.999.
    The measured worst per-clip cosines belong in the comment at the assertion (`pytest -s` prints the current ones)."""
    a8, a16 = _arch(kind, fp8=True, **over), _arch(kind, **over)
    keep = None
    worst = {}
    for name, a in (("e4m3", a8), ("bf16 twin", a16)):
        m, oarch, P = _model(a, seed=7)
        n = O.patches_per_frame(oarch)
        keep = torch.arange(n).unsqueeze(0)
        v = O.synth_batch(oarch, B=B, T=T, seed=21, n_trans=1)["video"]
        got = m.encode_video(v, keep)
        with torch.no_grad():
            _, want = m.compute_video(v, keep.expand(B, -1))
        worst[name] = float(cos_rows(got, want).min())
        del m
        torch.cuda.empty_cache()
    print(f"\n   [{a8['name']} T={T} n={n}] worst per-clip cosine encode_video vs training forward: e4m3 {worst['e4m3']:.7f}, "
          f"bf16 twin {worst['bf16 twin']:.7f}")
    # NOT YET MEASURED on an MI355X (H structure n = 256 T = 2, B-style n = 16 T = 3; e4m3 and bf16 twin): the values belong here
    assert worst["e4m3"] >= 0.999, worst
    assert worst["bf16 twin"] >= 0.999, worst


# ------------------------------------------------------------------------------------------------ 5. the text tower
def test_text_is_untouched(small_fp8):
    """the text tower is never quantised: on an e4m3 architecture encode_text has the bits of compute_text, and the packed pass
    agrees with it within the tolerance of tests/test_text_packed_gpu.py (rel-L2 < 0.02, row cosine > 0.9995)"""
    m, oarch, P = small_fp8
    ids = O.synth_batch(oarch, B=2, T=2, seed=9, caption_len=12)["text"].clone()
    for r, n in enumerate((3, 12, 7, 2, 9, 12, 5, 8)):
        ids[r, n - 1] = oarch["vocab"] - 1
        ids[r, n:] = 0
    want, _ = m.compute_text(ids)
    got = m.encode_text(ids)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    packed = m.encode_text(ids, packed=True)
    e, c = rel(packed, want), float(cos_rows(packed, want).min())
    print(f"\n   encode_text(packed=True) vs compute_text on the e4m3 architecture: rel {e:.3e}, min cosine {c:.7f}")
    assert e < 0.02 and c > 0.9995, (e, c)


# ------------------------------------------------------------------------------------------------ 6. isolation
@pytest.mark.parametrize("flag", ["fp8", "fp8_wgrad"])
def test_e4m3_encoders_leave_the_training_step_alone(flag):
    """training step, encoder calls, training step -- against the same two training steps without the encoder calls: identical
    losses, gradients, e4m3 scale table and maxima; the encoder calls move no training workspace and touch nothing the backward
    recorded.  fp8_wgrad: the first step is the calibration step, so the encoder calls run with _f8_tensor_mode on (and still per
    token) and the second step runs per tensor."""
    from tvts_amd.engine import LossHead
    a = _arch("b", **{flag: True})
    oarch = O.tiny_arch(**a)
    batch = O.synth_batch(oarch, B=4, T=3, seed=5, caption_len=11)

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
        eng.end_step()
        torch.cuda.synchronize()
        return l1.clone(), l2.clone(), m.store.grad.clone()

    def table(eng):
        return (None if eng._f8_scale is None else eng._f8_scale.clone(), None if eng._f8_amax is None else eng._f8_amax.clone(),
                dict(eng._f8_ids), eng._f8_tensor_mode)

    def same_table(x, y):
        return all((p is None and q is None) or torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x[:2], y[:2])) \
            and x[2:] == y[2:]

    used, _, P = _model(a, seed=3)
    first = step(used)
    eng = used.engine
    assert eng._f8_tensor_mode == (flag == "fp8_wgrad")
    ptrs = {k: t.data_ptr() for k, t in eng.buf.items()}
    backs = {k: (t.data_ptr(), t.numel()) for k, t in eng._back.items()}
    book = (dict(eng._x8), dict(eng._x8_ready), set(eng._x8_only), dict(eng._dy8_ready))
    tab = table(eng)
    e1 = used.encode_video(batch["video"])
    used.encode_text(batch["text"])
    used.encode_text(batch["text"], packed=True)
    e2 = used.encode_video(batch["video"][:2, :2], batch["keep_ind"][:2])
    assert torch.isfinite(e1).all() and e1.shape == (4, a["embed"]) and torch.isfinite(e2).all()
    assert {k: t.data_ptr() for k, t in eng.buf.items()} == ptrs
    assert {k: (t.data_ptr(), t.numel()) for k, t in eng._back.items()} == backs
    now = (dict(eng._x8), dict(eng._x8_ready), set(eng._x8_only), dict(eng._dy8_ready))
    assert all(p.keys() == q.keys() if isinstance(p, dict) else p == q for p, q in zip(book, now))
    assert all(now[0][k][0].data_ptr() == book[0][k][0].data_ptr() for k in book[0])
    assert same_table(table(eng), tab)
    second = step(used)
    fresh, _, _ = _model(a, seed=3)
    want_first, want_second = step(fresh), step(fresh)
    for got, want, which in ((first, want_first, "first step"), (second, want_second, "second step")):
        for g, w, what in zip(got, want, ("loss1", "loss2", "gradients")):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (which, what)
    assert same_table(table(eng), table(fresh.engine))
    if flag == "fp8_wgrad":
        assert eng._f8_tensor_mode and len(eng._f8_ids) == 12 * a["layers"]


# ------------------------------------------------------------------------------------------------ 7. multiple choice
def test_multiple_choice_on_the_e4m3_architecture():
    """an _mc-style model (MCBase with arch=) on the small e4m3 architecture: 2 clips x 3 candidate captions of different lengths ->
    [C, B, E] and [B, E]; its mc_logits are those of the encoders called separately"""
    from tvts_amd.downstream import zero_shot as Z
    from tvts_amd.downstream._common import MCBase
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    a = _arch("b", fp8=True)
    m = MCBase(load_checkpoint=None, arch=a)
    oarch = O.tiny_arch(**dict(a, mask_ratio=0.0, sort_head=False))
    P = O.synth_params(oarch, seed=0)
    assert list(m.state_dict().keys()) == list(P.keys())
    m.load_state_dict(P, strict=True)
    assert len(m.store.w8) == 0 or len(m.store.w8) == 6 * a["layers"]
    B, T, C = 2, 2, 3
    video = O.synth_batch(oarch, B=B, T=T, seed=8, n_trans=1)["video"]
    g = torch.Generator().manual_seed(9)
    text = torch.zeros(C * B, a["context"], dtype=torch.int32)
    for r, ln in enumerate((4, 16, 9, 2, 13, 7)):
        text[r, 0] = a["vocab"] - 2
        text[r, 1:ln - 1] = torch.randint(1, a["vocab"] - 2, (max(ln - 2, 0),), generator=g, dtype=torch.int32)
        text[r, ln - 1] = a["vocab"] - 1
    te, ve = m({"text": text, "video": video})
    assert te.shape == (C, B, a["embed"]) and ve.shape == (B, a["embed"])
    assert bool(torch.isfinite(te).all()) and bool(torch.isfinite(ve).all())
    logits = Z.mc_logits(te, ve)
    assert logits.shape == (B, C)
    sep_t, sep_v = m.encode_text(text, packed=True).view(C, B, -1), m.encode_video(video)
    assert torch.equal(Z.mc_logits(sep_t, sep_v).view(torch.int32), logits.view(torch.int32))
    # and the scores of the rectangular text pass, in float64 (the packed pass differs from it by bf16 rounding only)
    td, vd = m.encode_text(text).view(C, B, -1).double(), sep_v.double()
    want = 100.0 * torch.einsum("be,cbe->bc", vd / vd.norm(dim=-1, keepdim=True), td / td.norm(dim=-1, keepdim=True))
    assert float((logits.double() - want).abs().max()) < 0.5, (logits, want)
