"""Parity ON the path bench.py times (run with -m gpu): the pipelined 256x256 NT kernel in bf16 with every epilogue
template at the step's own sizes, one ViT-B/16 T=8 mask-0.5 engine step large enough for the dispatcher to pick that
kernel, and the hipGraph-replayed step against eager launches and against the CPU oracle.

Tolerances: kernel level = the ones of tests/test_kernels_gpu.py (bf16 output 4e-3 rel-L2, fp32 output 2e-5, activation
outputs 5e-3); model level = SURVEY.md 8d (row cosine >= 0.9995, rel-L2 <= 2 %, |d loss| <= 1e-2, grad-norm 1 %)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tvts_oracle as O  # noqa: E402  (checker only)
import kernel_bounds as KB  # noqa: E402  (per-element bounds against float64)

DEV = "cuda:0"


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


@pytest.fixture(scope="module")
def lib(K):
    from tvts_amd import _lib
    return _lib.load()


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def operands(M, N, Kd, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(M, Kd, generator=g, device=DEV).bfloat16()
    b = (torch.randn(N, Kd, generator=g, device=DEV) * Kd ** -0.5).bfloat16()
    bias = torch.randn(N, generator=g, device=DEV)
    return a, b, bias


def ref_product(a, b, bias):
    """fp32 torch product of the bf16-rounded operands (exact products, fp32 accumulation) + bias, spot-checked in
    float64 on the CPU over rows that include both tile edges and the ragged tail."""
    ref = a.float() @ b.float().t() + bias
    M = a.shape[0]
    rows = sorted({0, 1, 255, 256, 257, M // 2, (M // 256) * 256 - 1, (M // 256) * 256, M - 2, M - 1} & set(range(M)))
    r64 = a[rows].double().cpu() @ b.double().cpu().t() + bias.double().cpu()
    assert rel(ref[rows].cpu(), r64) < 2e-6
    return ref


def guard_out(M, N, dtype):
    """output with 3 guard rows behind it: a kernel that writes past row M-1 of a ragged last tile is caught"""
    buf = torch.full((M + 3, N), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[:M]


def check_guard(buf, M):
    assert torch.isnan(buf[M:].float()).all(), "rows past M were written"


def bound(name, v):
    """the worst |err| / bound of a per-element check (kernel_bounds.py) and the worst used share of its accumulation term,
    printed for the record"""
    print(f"BOUND {name} {v:.4g} acc {KB.pop_acc_worst():.4g}")
    return v


# ------------------------------------------------------------------------------------------------ (a) the kernel
PLAIN = [(40000, 512, 768), (150720, 2304, 768), (150720, 768, 3072), (40000, 3840, 1280), (40000, 5120, 1280),
         (40000, 3072, 256)]


@pytest.mark.parametrize("M,N,Kd", PLAIN)
def test_nt256p_bf16_plain_outputs(K, lib, M, N, Kd):
    """gemm_nt256p_kernel<0,0,false>: bf16 and fp32 outputs, ragged last row tile (40000 = 156 x 256 + 64, 150720 =
    588 x 256 + 192), row-major walk (N = 512 / 768 / 2304) and the column-group walk (N = 3072: gc 6, 3840 / 5120: gc 5)."""
    assert K.gemm_nt_select(M, N) == 256
    a, b, bias = operands(M, N, Kd, seed=100 + N)
    ref = ref_product(a, b, bias)
    for dt, tol in ((torch.bfloat16, 4e-3), (torch.float32, 2e-5)):
        buf, out = guard_out(M, N, dt)
        K.gemm_nt(a, b, out, bias=bias)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()
        assert rel(out.float(), ref) < tol, (dt, rel(out.float(), ref))
        check_guard(buf, M)
        bound(f"nt256p plain {M},{N},{Kd} {dt}", KB.check_gemm(out, a, b, bias=bias, what=f"nt256p plain {dt}"))
    # the 128x128 kernel on the same operands: the two tilings agree to fp32 summation-order noise
    assert K.gemm_nt_select(M, N, tile=128) == 128
    o128 = torch.empty(M, N, dtype=torch.float32, device=DEV)
    K.gemm_nt(a, b, o128, bias=bias, tile=128)
    assert rel(o128, out.float()) < 2e-6


@pytest.mark.parametrize("M,N,Kd", [(150720, 768, 768), (150720, 2304, 768), (40000, 512, 768), (40000, 3840, 1280), (1000, 768, 128),
                                    (24576, 1536, 512), (150720, 768, 3072)])
def test_nt256p_bf16_first_patch_gives_the_bits_of_the_fp32_patch(K, lib, M, N, Kd):
    """Round 6: plain bf16 results leave the 256 x 256 kernel through the bf16-FIRST patch (the tile is rounded in the accumulator layout
    and crosses the LDS patch as bf16, two 16-row slabs per 4 KiB patch) -- generic epilogue (N = 512 / 768 / 1536) and the
    hand-scheduled one (N >= 2304), whole and ragged row tiles (40000 = 156 x 256 + 64; 1000 rows: three whole tiles and one of 232),
    with and without bias.  One rounding of the same fp32 value either way: the bits of the fp32 patch (TVTS_GEMM_F32_PATCH), no row
    past M written; fp32 results take the fp32 patch inside the same kernel and are unchanged as well."""
    a, b, bias = operands(M, N, Kd, seed=7 + N + Kd)
    for bi in (bias, None):
        for dt in (torch.bfloat16, torch.float32):
            buf, out = guard_out(M, N, dt)
            K.gemm_nt(a, b, out, bias=bi, tile=256)
            with K.options(nt_f32_patch=True):
                buf0, out0 = guard_out(M, N, dt)
                K.gemm_nt(a, b, out0, bias=bi, tile=256)
            torch.cuda.synchronize()
            assert torch.isfinite(out.float()).all()
            assert torch.equal(out, out0), (dt, bi is not None, float((out.float() - out0.float()).abs().max()))
            check_guard(buf, M); check_guard(buf0, M)
    ref = ref_product(a, b, bias)
    buf, out = guard_out(M, N, torch.bfloat16)
    K.gemm_nt(a, b, out, bias=bias, tile=256)
    assert rel(out.float(), ref) < 4e-3
    bound(f"nt256p bf16-first {M},{N},{Kd}", KB.check_gemm(out, a, b, bias=bias, what="nt256p bf16-first patch"))


@pytest.mark.parametrize("M,N,Kd,odt", [(150720, 768, 768, torch.float32), (150720, 768, 768, torch.bfloat16),
                                        (40000, 3072, 256, torch.float32), (150720, 768, 3072, torch.float32)])
def test_nt256p_bf16_residual_epilogue(K, lib, M, N, Kd, odt):
    """fp32 residual added in the epilogue (attention / MLP output projections: s_res, x_{l+1} fp32; t_res bf16)."""
    assert K.gemm_nt_select(M, N) == 256
    a, b, bias = operands(M, N, Kd, seed=200 + N + Kd)
    res = torch.randn(M, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    ref = ref_product(a, b, bias) + res
    buf, out = guard_out(M, N, odt)
    K.gemm_nt(a, b, out, bias=bias, residual=res)
    assert rel(out.float(), ref) < (2e-5 if odt == torch.float32 else 4e-3)
    check_guard(buf, M)
    w = KB.check_gemm(out, a, b, bias=bias, residual=res, what=f"nt256p residual {odt}")
    gbuf, gout = KB.guarded(M, N, odt, DEV)  # guard rows AND columns (leading dimension N + 8)
    K.gemm_nt(a, b, gout, bias=bias, residual=res)
    KB.check_guards(gbuf, M, N, "nt256p residual")
    KB.assert_equal_bits(gout, out, "nt256p residual, wider leading dimension")
    bound(f"nt256p residual {M},{N},{Kd} {odt}", w)


@pytest.mark.parametrize("M,N,Kd,act", [(150720, 3072, 768, "quick_gelu"), (40000, 5120, 1280, "gelu"),
                                        (40000, 512, 128, "quick_gelu"), (40000, 2304, 64, "gelu")])
def test_nt256p_bf16_activation_epilogue(K, lib, M, N, Kd, act):
    """<1,0> QuickGELU and <2,0> erf-GELU with the pre-activation side output (MLP c_fc forward)."""
    assert K.gemm_nt_select(M, N) == 256
    a, b, bias = operands(M, N, Kd, seed=300 + N)
    pre_ref = ref_product(a, b, bias)
    fn = O.quick_gelu if act == "quick_gelu" else O.gelu_erf
    buf, out = guard_out(M, N, torch.bfloat16)
    pbuf, pre = guard_out(M, N, torch.bfloat16)
    K.gemm_nt(a, b, out, bias=bias, act=act, preact=pre)
    assert rel(pre.float(), pre_ref) < 4e-3 and rel(out.float(), fn(pre_ref)) < 5e-3
    check_guard(buf, M); check_guard(pbuf, M)
    w = KB.check_gemm(out, a, b, bias=bias, act=act, preact=pre, what=f"nt256p {act}")
    gbuf, gout = KB.guarded(M, N, torch.bfloat16, DEV)
    gpbuf, gpre = KB.guarded(M, N, torch.bfloat16, DEV)
    K.gemm_nt(a, b, gout, bias=bias, act=act, preact=gpre)
    KB.check_guards(gbuf, M, N, "nt256p act out"); KB.check_guards(gpbuf, M, N, "nt256p act preact")
    KB.assert_equal_bits(gout, out, "nt256p act, wider ld"); KB.assert_equal_bits(gpre, pre, "nt256p preact, wider ld")
    # fp32 output of the same template
    out32 = torch.empty(M, N, dtype=torch.float32, device=DEV)
    K.gemm_nt(a, b, out32, bias=bias, act=act, preact=pre)
    assert rel(out32, fn(pre_ref)) < 5e-5
    w = max(w, KB.check_gemm(out32, a, b, bias=bias, act=act, what=f"nt256p {act} fp32"))
    bound(f"nt256p {act} {M},{N},{Kd}", w)


@pytest.mark.parametrize("M,N,Kd,act", [(150720, 3072, 768, "quick_gelu"), (40000, 3840, 640, "gelu"),
                                        (40000, 768, 3072, "quick_gelu")])
def test_nt256p_bf16_gate_epilogue(K, lib, M, N, Kd, act):
    """<0,1> / <0,2>: dgrad of c_proj with the activation-gradient gate act'(h) fused (MLP backward)."""
    assert K.gemm_nt_select(M, N) == 256
    a, b, _ = operands(M, N, Kd, seed=400 + N)
    h = (torch.randn(M, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)) * 1.5).bfloat16()
    x = h.float().clone().requires_grad_(True)
    (O.quick_gelu(x) if act == "quick_gelu" else O.gelu_erf(x)).sum().backward()
    ref = ref_product(a, b, torch.zeros(N, device=DEV)) * x.grad
    buf, out = guard_out(M, N, torch.bfloat16)
    K.gemm_nt(a, b, out, gate_h=h, gate_act=act)
    assert rel(out.float(), ref) < 5e-3, rel(out.float(), ref)
    check_guard(buf, M)
    w = KB.check_gemm(out, a, b, gate_h=h, gate_act=act, what=f"nt256p gate {act}")
    gbuf, gout = KB.guarded(M, N, torch.bfloat16, DEV)
    K.gemm_nt(a, b, gout, gate_h=h, gate_act=act)
    KB.check_guards(gbuf, M, N, "nt256p gate")
    KB.assert_equal_bits(gout, out, "nt256p gate, wider ld")
    bound(f"nt256p gate {act} {M},{N},{Kd}", w)


def test_nt256p_strided_views_and_forced_small_shapes(K, lib):
    """leading dimensions wider than the matrices (the engine's packed buffers) and, with the tile forced, outputs smaller
    than one tile / one XCD round (grid < 256 blocks)."""
    with K.options(nt_tile=256):
        for (M, N, Kd) in [(100, 256, 64), (257, 512, 128), (3140, 768, 768), (1570, 2304, 768), (3000, 72, 64)]:
            assert K.gemm_nt_select(M, N) == 256
            g = torch.Generator(device=DEV).manual_seed(M)
            abig = torch.randn(M, Kd + 64, generator=g, device=DEV).bfloat16()
            bbig = (torch.randn(N, Kd + 128, generator=g, device=DEV) * Kd ** -0.5).bfloat16()
            obig = torch.full((M, N + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
            a, b, out = abig[:, 64:], bbig[:, :Kd], obig[:, :N]
            K.gemm_nt(a, b, out)
            ref = a.float() @ b.float().t()
            assert rel(out.float(), ref) < 4e-3, (M, N, Kd, rel(out.float(), ref))
            assert torch.isnan(obig[:, N:].float()).all()
            bound(f"nt256p strided {M},{N},{Kd}", KB.check_gemm(out, a, b, what=f"nt256p strided {M},{N},{Kd}"))


# ------------------------------------------------------------------------------------------------ (b) the engine step
ARGS = types.SimpleNamespace(local_rank=0, rank=0, world_size=1)


def min_cos(a, b):
    a, b = a.detach().double().cpu().reshape(a.shape[0], -1), b.detach().double().cpu().reshape(b.shape[0], -1)
    return float(torch.nn.functional.cosine_similarity(a, b, dim=1).min())


def test_b16_step_at_bench_dispatch_against_oracle(K, lib):
    """ViT-B/16, 8 frames, tube mask 0.5, 4 x 32-token captions, 24 pairs: M = 18 840 rows -> 222 / 666 / 888 tiles of 256x256,
    so the ViT blocks' qkv / proj / MLP GEMMs (forward and dgrad, every epilogue) take gemm_nt256p_kernel exactly as in
    the 192-pair bench step.  Forward + losses + hand-written backward against the fp32 CPU oracle."""
    _step_against_oracle(lib, "B_16", 24, 8, big_tile=True)


def test_b32_t8_step_against_oracle(K, lib):
    """BASELINE.json configs[1]: ViT-B/32, 8 frames of 224^2, no mask (49 patches per frame, S = 393), 4 x 32-token captions, at the
    reference's own per-GPU batch of 24 pairs (configs/..b-32.json:21; M = 9 432 token rows): the same gates."""
    _step_against_oracle(lib, "B_32", 24, 8, big_tile=False)


def _step_against_oracle(lib, arch_name, B, T, big_tile):
    import psutil
    if psutil.virtual_memory().available < 80 * 2 ** 30:
        pytest.skip("the fp32 CPU oracle's autograd graph at 24 pairs needs ~40 GB of host memory")
    from tvts_amd import arch as A
    from tvts_amd.engine import LossHead
    from tvts_amd.model._common import TVTSv2Base
    a = A.ARCHS[arch_name]
    S = 1 + T * A.n_keep(a)
    if big_tile:
        from tvts_amd import hip as K
        assert K.gemm_nt_select(B * S, 768) == 256 and K.gemm_nt_select(B * S, 2304) == 256
    oarch = O.ARCHS[arch_name]
    P = O.synth_params(oarch, seed=11)
    m = TVTSv2Base(ARGS, arch=a)
    m.load_state_dict(P, strict=True)
    batch = O.synth_batch(oarch, B=B, T=T, seed=12, caption_len=32)
    # oracle
    torch.set_num_threads(min(64, torch.get_num_threads()))
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    r1, r2, rte, rve, rpred = O.step_losses(leaves, batch, oarch)
    (r1 + r2).backward()
    grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    gn_ref = sum(float(g.double().norm()) ** 2 for g in grads.values()) ** 0.5
    # engine
    m._fresh_shadows(); m._sync_requires_grad()
    pb = m.engine.prepare_batch(batch)
    m.store.grad.zero_()
    te, ve, pred = m.engine.forward(pb)
    head = LossHead(m.store.device)
    loss1, dv, dt = head.contrastive(ve, te)
    loss2, dpred = head.sorting(pred, batch["label"].reshape(-1).to(torch.int32).to(DEV))
    m.engine.backward(dt, dv, dpred)
    torch.cuda.synchronize()
    assert min_cos(te, rte) > 0.9995 and rel(te.cpu(), rte.detach()) < 0.02
    assert min_cos(ve, rve) > 0.9995 and rel(ve.cpu(), rve.detach()) < 0.02, (min_cos(ve, rve), rel(ve.cpu(), rve.detach()))
    r1, r2 = r1.detach(), r2.detach()
    assert abs(float(loss1) - float(r1)) < 1e-2 and abs(float(loss2) - float(r2)) < 1e-2, (float(loss1), float(r1), float(loss2), float(r2))
    gn = 0.0
    worst = []
    for k, g in grads.items():
        mine = m.store.g(k).detach().cpu()
        assert torch.isfinite(mine).all(), k
        gn += float(mine.double().norm()) ** 2
        if float(g.norm()) > 1e-3 * gn_ref:
            worst.append((float(torch.nn.functional.cosine_similarity(mine.double().flatten(), g.double().flatten(), dim=0)), k))
    gn = gn ** 0.5
    worst.sort()
    assert abs(gn - gn_ref) < 0.01 * gn_ref, (gn, gn_ref, worst[:5])
    assert worst[0][0] > 0.995, worst[:8]
    # the same step with every NT GEMM that can take it on the stream-K walk (K-stage work split, ordered sum of the partial tiles in
    # the last-arriving block) and every split weight gradient reduced inside its kernel: the same gates against the oracle, and
    # two such steps leave the same bits (the sums are ordered whoever arrives last)
    from tvts_amd import hip as K2
    g_default = m.store.grad.clone()

    def forced_step():
        m.store.grad.zero_()
        te_, ve_, pred_ = m.engine.forward(pb)
        l1_, dv_, dt_ = head.contrastive(ve_, te_)
        l2_, dp_ = head.sorting(pred_, batch["label"].reshape(-1).to(torch.int32).to(DEV))
        m.engine.backward(dt_, dv_, dp_)
        torch.cuda.synchronize()
        return float(l1_), float(l2_), te_.clone(), ve_.clone(), m.store.grad.clone()
    with K2.options(nt_streamk=True, tn_streamk=True):
        n0 = K2.STREAMK_TAKEN[0]
        s1, s2, te_s, ve_s, g_s = forced_step()
        taken = K2.STREAMK_TAKEN[0] - n0
        _, _, _, _, g_s2 = forced_step()
    assert taken >= 200, taken                      # the ViT blocks' GEMMs did take the forced paths
    assert torch.equal(g_s, g_s2)
    assert min_cos(ve_s, rve) > 0.9995 and rel(ve_s.cpu(), rve.detach()) < 0.02
    assert abs(s1 - float(r1)) < 1e-2 and abs(s2 - float(r2)) < 1e-2
    gn_s = float(g_s.double().norm())
    assert abs(gn_s - gn_ref) < 0.01 * gn_ref and not torch.equal(g_s, g_default)
    cos = float(torch.nn.functional.cosine_similarity(g_s.double().flatten(), g_default.double().flatten(), dim=0))
    assert cos > 0.9999, cos


def _sub_batch(batch, idx, NT):
    """the samples `idx` of a clip-major batch dict (text rows are i * B + b; v1: the tokenizer's dict of such matrices)"""
    B = batch["video"].shape[0]
    rows = lambda t: t.reshape(NT, B, -1)[:, idx].reshape(NT * len(idx), -1)  # noqa: E731
    out = {"video": batch["video"][idx], "keep_ind": batch["keep_ind"][idx],
           "text": {k: rows(v) for k, v in batch["text"].items()} if isinstance(batch["text"], dict) else rows(batch["text"])}
    if "label" in batch:
        out["label"] = batch["label"][idx]
    return out


@pytest.mark.parametrize("arch_name,B,T,nsub", [("B_16", 192, 8, 24), ("B_32", 384, 8, 24), ("H_14", 48, 16, 4), ("v1", 256, 4, 16)])
def test_full_size_step_properties(K, lib, arch_name, B, T, nsub):
    """The workloads bench.py times -- the headline ViT-B/16, 8 frames, mask 0.5, 4 x 32-token captions, 192 pairs (BASELINE.json's
    metric configuration; M = 150 720 token rows), configs[1] (B/32, 384 pairs), H/14 with 16 frames and the v1 step (dropout off:
    its masks are drawn per element of the batch) -- are out of the CPU oracle's reach, so the full-size step is tied to the
    oracle-checked sizes (test_b16_step_at_bench_dispatch_against_oracle: 24 pairs, same kernels and dispatch; tests/test_model_gpu.py,
    tests/test_v1_gpu.py) by properties that do not depend on the size: (1) run twice it gives the same bits; (2) a sample's embeddings and sort logits do not depend on the other samples of the
    batch: the first `nsub` samples run alone give the rows the full batch gives (different tile counts and kernels for the text
    tower: equal to bf16 rounding, not bit for bit); (3) rotating the batch rotates the embeddings, leaves both losses where they were
    and the parameter gradient too -- up to bf16 rounding noise (see the assertion)."""
    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch, synth_batch_v1
    from tvts_amd.engine import LossHead
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.model.model_dist_TVTS import TVTS
    a = dict(A.ARCHS[arch_name])
    a["num_frames"] = max(a["num_frames"], T)
    v1 = a.get("family") == "v1"
    NT = a["n_trans"]
    m = (TVTS if v1 else TVTSv2Base)(ARGS, arch=a, init_seed=0)
    m._fresh_shadows(); m._sync_requires_grad()
    if v1:
        m.engine.training = False
    head = LossHead(m.store.device)
    batch = (synth_batch_v1 if v1 else synth_batch)(a, B, T, seed=31, caption_len=32)

    def run(bt):
        pb = m.engine.prepare_batch(bt)
        m.store.grad.zero_()
        te, ve, pred = m.engine.forward(pb)
        loss1, dv, dt = head.contrastive(ve, te)
        loss2, dpred = head.sorting(pred, bt["label"].reshape(-1).to(torch.int32).to(DEV))
        m.engine.backward(dt, dv, dpred)
        torch.cuda.synchronize()
        return te.clone(), ve.clone(), pred.reshape(te.shape[0], -1).clone(), float(loss1), float(loss2), m.store.grad.clone()

    te, ve, pred, l1, l2, g = run(batch)
    assert all(torch.isfinite(t).all() for t in (te, ve, pred, g)) and np.isfinite(l1) and np.isfinite(l2)
    # (1) reproducible to the bit
    te2, ve2, pred2, l1b, l2b, g2 = run(batch)
    assert torch.equal(te, te2) and torch.equal(ve, ve2) and torch.equal(pred, pred2) and (l1, l2) == (l1b, l2b) and torch.equal(g, g2)
    del te2, ve2, pred2, g2
    # (2) the oracle-checked size is a sub-batch of this one
    idx = torch.arange(nsub)
    tes, ves, preds, _, _, _ = run(_sub_batch(batch, idx, NT))
    for full, sub in ((te[:nsub], tes), (ve[:nsub], ves), (pred[:nsub], preds)):
        assert min_cos(full, sub) > 0.9999 and rel(full, sub) < 6e-3, (min_cos(full, sub), rel(full, sub))
    # (3) rotation of the batch
    perm = torch.roll(torch.arange(B), 37)
    tep, vep, predp, l1p, l2p, gp = run(_sub_batch(batch, perm, NT))
    permd = perm.to(DEV)
    gn, gnp = float(g.double().norm()), float(gp.double().norm())
    stats = dict(te=rel(tep, te[permd]), ve=rel(vep, ve[permd]), pred=rel(predp, pred[permd]), dl1=l1p - l1, dl2=l2p - l2,
                 g=rel(gp, g), gn=(gnp - gn) / gn)
    print("rotation:", arch_name, stats)
    # (not bit for bit: a GEMM row's fp32 summation order depends on its place in the 256-row tile -- the bias joins the accumulators
    # before the last k-step of one half of the wave tile -- and a last-bit difference flips bf16 roundings downstream)
    # measured on B/16: te 1.0e-3, ve 3.0e-3, pred 1.9e-3, losses 2e-4 / 5e-5, gradient 3.0e-3, its norm 1e-4 (the step's distance
    # from the fp32 oracle is 4-5e-3 on the embeddings: the same bf16 rounding noise)
    assert stats["te"] < 6e-3 and stats["ve"] < 6e-3 and stats["pred"] < 1e-2, stats
    assert min_cos(tep, te[permd]) > 0.9999 and min_cos(vep, ve[permd]) > 0.9999
    assert abs(stats["dl1"]) < 2e-3 and abs(stats["dl2"]) < 2e-3, stats
    assert stats["g"] < 2e-2 and abs(stats["gn"]) < 2e-3, stats


@pytest.mark.parametrize("arch_name,B,T,flags", [("B_16", 48, 8, ()), ("B_32", 48, 8, ()), ("H_14", 8, 16, ()), ("H_14", 8, 16, ("fp8", "fp8_dgrad")),
                                                 ("B_16", 48, 8, ("bf16_residual",)), ("B_16", 48, 8, ("hybrid_stream=False",)),
                                                 ("H_14", 8, 16, ("hybrid_stream=False",)), ("v1", 48, 4, ())])
def test_every_gradient_is_bit_reproducible(K, lib, arch_name, B, T, flags):
    """Two identical steps (the training step's parameter groups, v1 with its dropout masks pinned) leave the same bits in EVERY
    parameter gradient and both losses: all reductions of the step are ordered sums -- none is a scatter of fp32 atomics whose
    last-bit noise could, through Adam, flip a bf16 rounding of the next forward (experiments/dbg/bench_repro.py runs
    the same check at the bench's sizes)."""
    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch, synth_batch_v1
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.model.model_dist_TVTS import TVTS
    a = dict(A.ARCHS[arch_name])
    a["num_frames"] = max(a["num_frames"], T)
    for f in flags:
        a[f.split("=")[0]] = not f.endswith("=False")
    v1 = a.get("family") == "v1"
    m = (TVTS if v1 else TVTSv2Base)(ARGS, arch=a, init_seed=0)
    for name, p in m.named_parameters():
        p.requires_grad = A.param_group_of(name, a) >= 0
    _, _, run = _runner_of(m, a)
    eng = m.engine
    if hasattr(eng, "training"):
        eng.training = True
    batch = (synth_batch_v1 if v1 else synth_batch)(a, B, T, seed=5, caption_len=32)
    m._fresh_shadows(); m._sync_requires_grad()
    pb = eng.prepare_batch(batch)
    lab = batch["label"].reshape(-1).to(torch.int32).to(DEV)
    seed0 = eng.drop_seed.clone() if hasattr(eng, "drop_seed") else None

    def grads():
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
        return m.store.grad.clone(), float(l1), float(l2)

    g0, l1, l2 = grads()
    assert torch.isfinite(g0).all() and float(g0.abs().max()) > 0
    for _ in range(2):
        g1, l1b, l2b = grads()
        if not torch.equal(g0, g1):
            diff = (g0 - g1).abs()
            raise AssertionError(f"gradients differ between identical steps: max |d| {float(diff.max()):.3e} in {int((diff > 0).sum())} elements")
        assert (l1, l2) == (l1b, l2b)

@pytest.mark.parametrize("arch_name,B,T,NT", [("B_16", 12, 8, 4), ("B_16", 6, 4, 1), ("H_14", 2, 16, 4)])
def test_text_tower_on_its_own_stream_gives_the_same_bits(K, lib, arch_name, B, T, NT):
    """arch["text_side"] (the default): the text tower's forward and backward run on a second stream beside the ViT -- one fork and one
    join per direction, scratch buffers of their own (hip.lane).  The towers share nothing until the loss, so every embedding, both
    losses and every gradient have the bits of the in-line order, eagerly and through a captured hipGraph (whose replays keep the
    two chains side by side)."""
    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch
    from tvts_amd.model._common import TVTSv2Base
    res = {}
    for side in (False, True):
        a = dict(A.ARCHS[arch_name], text_side=side)
        a["num_frames"] = max(a["num_frames"], T)
        m = TVTSv2Base(ARGS, arch=a, init_seed=0)
        for name, p in m.named_parameters():
            p.requires_grad = A.param_group_of(name, a) >= 0
        _, _, run = _runner_of(m, a)
        eng = m.engine
        assert eng.text_side == side
        batch = synth_batch(a, B, T, seed=5, caption_len=32, n_trans=NT)
        m._fresh_shadows(); m._sync_requires_grad()
        pb = eng.prepare_batch(batch)
        lab = batch["label"].reshape(-1).to(torch.int32).to(DEV) if NT != 1 else None
        out = {}

        def grads():
            m.store.grad.zero_()
            eng.embeds_ready = run.gather.start
            try:
                te, ve, pred = eng.forward(pb)
            finally:
                eng.embeds_ready = None
            l1, l2, dte, dve, dpred = run.losses_and_grads(pb, te, ve, pred, lab)
            eng.backward(dte, dve, dpred)
            out.update(te=te, ve=ve, l1=l1)
        grads(); grads()
        torch.cuda.synchronize()
        eager = (m.store.grad.clone(), out["te"].clone(), out["ve"].clone(), out["l1"].clone())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            grads()
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(eager[0], m.store.grad), f"captured step differs from the eager one (text_side {side})"
        assert torch.equal(eager[1], out["te"]) and torch.equal(eager[3], out["l1"])
        res[side] = eager
        del g, m
    assert float(res[True][0].abs().max()) > 0
    for x, y in zip(res[False], res[True]):
        assert torch.equal(x, y)


def test_cu_reservation_gives_the_same_bits(K, lib):
    """dist.auto_cu_reservation reserves 8 CUs for the RCCL kernels at 24 ... 72 pairs per GPU when world > 1: the persistent 256 x 256
    NT grids then run on 248 CUs (hip.set_default(nt_cus=248)).  A smaller grid changes which block walks which tile, never a tile's
    arithmetic: embeddings, losses and every gradient of the 24-pair step keep their bits."""
    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch
    from tvts_amd.dist import auto_cu_reservation
    from tvts_amd.model._common import TVTSv2Base
    B, T, NT = 24, 8, 4
    a = dict(A.ARCHS["B_16"])
    keep = auto_cu_reservation(B * (T * 98 + 1), 8)
    assert keep == 8
    res = {}
    for cus in (0, 256 - keep):
        m = TVTSv2Base(ARGS, arch=a, init_seed=0)
        for name, p in m.named_parameters():
            p.requires_grad = A.param_group_of(name, a) >= 0
        _, _, run = _runner_of(m, a)
        eng = m.engine
        batch = synth_batch(a, B, T, seed=5, caption_len=32, n_trans=NT)
        m._fresh_shadows(); m._sync_requires_grad()
        pb = eng.prepare_batch(batch)
        lab = batch["label"].reshape(-1).to(torch.int32).to(DEV)
        with K.options(nt_cus=cus):
            m.store.grad.zero_()
            eng.embeds_ready = run.gather.start
            try:
                te, ve, pred = eng.forward(pb)
            finally:
                eng.embeds_ready = None
            l1, l2, dte, dve, dpred = run.losses_and_grads(pb, te, ve, pred, lab)
            eng.backward(dte, dve, dpred)
            torch.cuda.synchronize()
        res[cus] = (m.store.grad.clone(), te.clone(), ve.clone(), l1.clone(), l2.clone())
        del m
    assert float(res[0][0].abs().max()) > 0
    for x, y in zip(res[0], res[248]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("arch_name,B,T", [("B_16", 12, 8), ("B_32", 24, 8), ("H_14", 2, 16)])
def test_wgrad_side_stream_gives_the_same_bits(K, lib, arch_name, B, T):
    """The reference's own per-GPU batches (v2/configs/dist-yt-web-pt-vit-b-16.json:21 = 12, ...b-32.json:21 = 24, ...h-14.json:21 = 2):
    the weight gradients of the ViT blocks launched on the engine's side stream (arch["wgrad_stream"], the automatic choice at these
    sizes) leave the same bits in every gradient as the single-stream backward -- the same kernels write the same tensors, only
    beside the input-gradient chain instead of inside it -- eagerly and through a captured hipGraph."""
    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch
    from tvts_amd.model._common import TVTSv2Base
    res = {}
    for side in (False, True):
        a = dict(A.ARCHS[arch_name], wgrad_stream=side, tn_grouped=False)  # (grouping re-plans the contraction ranges: other bits)
        a["num_frames"] = max(a["num_frames"], T)
        m = TVTSv2Base(ARGS, arch=a, init_seed=0)
        for name, p in m.named_parameters():
            p.requires_grad = A.param_group_of(name, a) >= 0
        _, _, run = _runner_of(m, a)
        eng = m.engine
        batch = synth_batch(a, B, T, seed=5, caption_len=32)
        m._fresh_shadows(); m._sync_requires_grad()
        pb = eng.prepare_batch(batch)
        lab = batch["label"].reshape(-1).to(torch.int32).to(DEV)

        def grads():
            m.store.grad.zero_()
            eng.embeds_ready = run.gather.start
            try:
                te, ve, pred = eng.forward(pb)
            finally:
                eng.embeds_ready = None
            l1, l2, dte, dve, dpred = run.losses_and_grads(pb, te, ve, pred, lab)
            eng.backward(dte, dve, dpred)
            return l1, l2
        grads(); grads()
        torch.cuda.synchronize()
        eager = m.store.grad.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            grads()
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(eager, m.store.grad), f"captured backward differs from the eager one (side stream {side})"
        res[side] = eager
        del g, m
    assert float(res[True].abs().max()) > 0 and torch.equal(res[False], res[True])


@pytest.mark.parametrize("arch_name,B,T", [("B_16", 2, 8), ("B_16", 12, 8), ("B_32", 24, 8)])
def test_ring_kernels_leave_the_bits_of_the_old_small_batch_kernel(K, lib, arch_name, B, T):
    """The reference's per-GPU batches once more: with the ring forms of the 128-column NT kernel (the dispatcher's choice for the text
    tower at these sizes and for every GEMM of the 2-pair step) the step's losses and EVERY gradient are the bits of the step that
    forbids them (TVTS_GEMM_NO_RING through the engine's options: the double-buffered 128 kernel) -- same tile walk, k order and
    epilogue arithmetic -- and the captured step replays them."""
    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch
    from tvts_amd.model._common import TVTSv2Base
    assert K.gemm_nt_select(B * 4 * 32, 512) in (1128, 1192) and K.gemm_nt_select(B * 4 * 32, 512, tile="noring") in (128, 256)
    res = {}
    for tile in ("noring", None):
        a = dict(A.ARCHS[arch_name])
        a["num_frames"] = max(a["num_frames"], T)
        m = TVTSv2Base(ARGS, arch=a, init_seed=0)
        for name, p in m.named_parameters():
            p.requires_grad = A.param_group_of(name, a) >= 0
        _, _, run = _runner_of(m, a)
        eng = m.engine
        batch = synth_batch(a, B, T, seed=5, caption_len=32)
        m._fresh_shadows(); m._sync_requires_grad()
        pb = eng.prepare_batch(batch)
        lab = batch["label"].reshape(-1).to(torch.int32).to(DEV)

        def grads():
            m.store.grad.zero_()
            eng.embeds_ready = run.gather.start
            try:
                te, ve, pred = eng.forward(pb)
            finally:
                eng.embeds_ready = None
            l1, l2, dte, dve, dpred = run.losses_and_grads(pb, te, ve, pred, lab)
            eng.backward(dte, dve, dpred)
            return l1, l2
        with K.options(nt_tile=tile):
            grads()
            l1, l2 = grads()
            torch.cuda.synchronize()
            eager = m.store.grad.clone()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                grads()
            for _ in range(2):
                g.replay()
            torch.cuda.synchronize()
        assert torch.equal(eager, m.store.grad), f"captured backward differs from the eager one (nt_tile {tile})"
        res[tile] = (eager, float(l1), float(l2))
        del g, m
    assert float(res[None][0].abs().max()) > 0 and torch.equal(res["noring"][0], res[None][0]) and res["noring"][1:] == res[None][1:]


def test_grouped_weight_gradients_match_the_single_launches(K, lib):
    """At the reference's per-GPU batch (B/16, 12 pairs: M = 9 420) the six weight gradients of a ViT block leave in one grouped launch
    (arch["tn_grouped"], the automatic choice up to 12 000 token rows).  Same products, same ordered partial sums per problem -- only the
    number of contraction ranges differs from the one-by-one plan, i.e. fp32 summation order: every gradient within 1e-5 relative,
    run-to-run bit-reproducible, and capturable."""
    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch
    from tvts_amd.model._common import TVTSv2Base
    res = {}
    for grouped in (False, True):
        a = dict(A.ARCHS["B_16"], tn_grouped=grouped)
        m = TVTSv2Base(ARGS, arch=a, init_seed=0)
        for name, p in m.named_parameters():
            p.requires_grad = A.param_group_of(name, a) >= 0
        _, _, run = _runner_of(m, a)
        eng = m.engine
        batch = synth_batch(a, 12, 8, seed=5, caption_len=32)
        m._fresh_shadows(); m._sync_requires_grad()
        pb = eng.prepare_batch(batch)
        lab = batch["label"].reshape(-1).to(torch.int32).to(DEV)

        def step():
            m.store.grad.zero_()
            eng.embeds_ready = run.gather.start
            try:
                te, ve, pred = eng.forward(pb)
            finally:
                eng.embeds_ready = None
            l1, l2, dte, dve, dpred = run.losses_and_grads(pb, te, ve, pred, lab)
            eng.backward(dte, dve, dpred)
        step(); step()
        torch.cuda.synchronize()
        g1 = m.store.grad.clone()
        step()
        torch.cuda.synchronize()
        assert torch.equal(g1, m.store.grad)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        gr.replay(); gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(g1, m.store.grad), f"captured backward differs (grouped {grouped})"
        assert (len(eng._tn_groups) == a["layers"]) == grouped
        res[grouped] = (g1, m.store)
        del gr
        if grouped:
            # the reference's loop alternates two loaders of different clip lengths: a block keeps ONE plan per problem signature
            # instead of rebuilding (and re-uploading) it at every step, and going back to the first loader re-uses its plan
            pb_first = pb
            pb = eng.prepare_batch(synth_batch(a, 12, 4, seed=6, caption_len=32))
            step()
            plans_mid = {k: list(v.values()) for k, v in eng._tn_groups.items()}
            pb = pb_first
            step()
            torch.cuda.synchronize()
            assert torch.equal(g1, m.store.grad)
            assert all(len(v) == 2 for v in eng._tn_groups.values())
            assert all(list(v.values())[:len(plans_mid[k])] == plans_mid[k] for k, v in eng._tn_groups.items())  # nothing was rebuilt
    g0, g1 = res[False][0], res[True][0]
    assert not torch.equal(g0, g1)
    st = res[True][1]
    for name in st.shapes:
        if "resblocks" in name and name.startswith("video_model") and float(res[False][1].g(name).abs().max()) > 0:
            a_, b_ = res[False][1].g(name).double(), st.g(name).double()
            assert float((a_ - b_).norm() / b_.norm().clamp_min(1e-30)) < 1e-5, name


# ------------------------------------------------------------------------------------------------ (c) hipGraph replay
def _runner(a, P, lr_mul=1.0):
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
                        for i in range(4)], m.store, model=m)
    return m, opt, StepRunner(m, opt)


def _runner_of(m, a):
    from tvts_amd import arch as A
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner
    hp = ((1e-4, 0.0),) * 4 if a.get("family") == "v1" else A.GROUP_HPARAMS
    groups = [[], [], [], []]
    for name, p in m.named_parameters():
        gi = A.param_group_of(name, a)
        if gi >= 0:
            groups[gi].append(p)
    opt = FusedHFAdamW([dict(params=groups[i], lr=hp[i][0], weight_decay=hp[i][1]) for i in range(4) if groups[i]], m.store, model=m)
    return m, opt, StepRunner(m, opt)


def _three_steps(a, P, batch, mode):
    """mode: 'eager' (device-side step counter, plain launches) or 'graph' (captured once, replayed)."""
    m, opt, run = _runner(a, P)
    pb = m.engine.prepare_batch(batch)
    lab = batch["label"].reshape(-1).to(torch.int32).to(DEV)
    m._fresh_shadows(); m._sync_requires_grad()
    losses, gnorm = [], []
    if mode == "eager":
        for _ in range(3):
            out = run.run(pb, lab, device_step=True)
            torch.cuda.synchronize()
            losses.append(float(out["loss1"]) + float(out["loss2"])); gnorm.append(float(m.store.grad.double().norm()))
        return m, opt, losses, gnorm
    opt.sync_hyper()
    # one eager step warms the workspaces (capture must not allocate); its effect on the state is rolled back
    snap = {k: t.clone() for k, t in (("flat", m.store.flat), ("m", m.store.m), ("v", m.store.v))}
    run.run(pb, lab, device_step=True)
    torch.cuda.synchronize()
    m.store.flat.copy_(snap["flat"]); m.store.m.copy_(snap["m"]); m.store.v.copy_(snap["v"])
    opt.step_dev.zero_(); opt.global_step = 0
    m.store.refresh_shadows()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run.run(pb, lab, device_step=True)
    torch.cuda.synchronize()
    assert torch.equal(m.store.flat, snap["flat"]) and int(opt.step_dev.item()) == 0  # capture does not execute
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        losses.append(float(out["loss1"]) + float(out["loss2"])); gnorm.append(float(m.store.grad.double().norm()))
    assert int(opt.step_dev.item()) == 3
    assert opt.state_dict()["state"][0]["step"] == 3  # host counters re-read from the device counter
    return m, opt, losses, gnorm


def test_graph_replay_is_the_eager_step_on_a_deterministic_model(K, lib):
    """bench.py at world 1 captures the whole step (zero_grad ... fused AdamW, step counter in device memory) into a hipGraph
    and replays it.  On the small architecture the step is run-to-run reproducible (losses bit for bit), so three replays must
    leave the state three plain launches leave (round 2 found the captured step wrong from its second replay on: a
    hipMemsetAsync node did not zero the CLS-gradient accumulators on replay; the zeroing is a kernel now)."""
    from tvts_amd import arch as A
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    P = O.synth_params(oarch, seed=21)
    batch = O.synth_batch(oarch, B=4, T=2, seed=22, caption_len=9)
    me, _, le, ge = _three_steps(a, P, batch, "eager")
    mg, _, lg, gg = _three_steps(a, P, batch, "graph")
    assert lg == le and gg == ge, (lg, le, gg, ge)  # losses and gradient norms bit for bit: every reduction has a fixed order
    assert torch.equal(mg.store.flat, me.store.flat) and torch.equal(mg.store.m, me.store.m) and torch.equal(mg.store.v, me.store.v)


def test_graph_replayed_steps_match_eager_steps_and_the_oracle(K, lib):
    """The same on the headline architecture with the 256x256 kernel forced (so the replay exercises the benchmarked GEMM
    kernel at this small size).  History of this test: round 2 asserted 1e-5 on the first gradient norm and failed on the driver's
    box.  The cause was not reordering noise but a BIFURCATION: the type-embedding gradient (one of the lr 1e-4 parameters) was a
    sum of fp32 atomics, its 1e-8 noise moved the type embedding's master weights by an ulp after the first Adam step, and in
    ~12 % of the runs that flipped one bf16 rounding in the next forward -- a discrete alternative trajectory, 7e-5 away in the
    third loss (experiments/dbg/step_repro2.py found it: 36 of 300 steps).  Since round 3 every reduction of the step has a fixed order
    (loss scalars, bias gradients, CLS shares, LayerNorm sums, type / temporal / class embeddings and -- last -- the rows of the
    embedding tables): 300 of 300 repeated steps and graph replays end in the same losses bit for bit
    (profiles/r03_step_repro_spread_b16.txt).  Graph vs eager: losses, gradient norms and the parameters after three steps equal
    bit for bit; both against the oracle's train_step within the 2 % gate."""
    from tvts_amd import arch as A
    a = A.ARCHS["B_16"]
    oarch = O.ARCHS["B_16"]
    P = O.synth_params(oarch, seed=21)
    batch = O.synth_batch(oarch, B=4, T=8, seed=22, caption_len=32)
    with K.options(nt_tile=256):
        me, _, le, ge = _three_steps(a, P, batch, "eager")
        mg, _, lg, gg = _three_steps(a, P, batch, "graph")
    assert lg == le and gg == ge, (lg, le, gg, ge)  # (gradient norms of every replay: garbage would show here first)
    assert torch.equal(mg.store.flat, me.store.flat)
    Pr = {k: v.clone() for k, v in P.items()}
    state, curve = {}, []
    for _ in range(3):
        r1, r2, _ = O.train_step(Pr, batch, oarch, state)
        curve.append(r1 + r2)
    assert np.all(np.abs(np.array(lg) - np.array(curve)) < 0.02 * np.abs(np.array(curve)) + 1e-2), (lg, curve)
    for k in ("pred_model.head.weight", "video_model.transformer.resblocks.11.timeattn.proj.weight", "video_model.proj"):
        assert rel(mg.store.p(k).cpu(), Pr[k]) < 2e-2, k


def test_full_size_graph_replay_is_the_eager_step(K, lib):
    """... and at the size bench.py replays it: ViT-B/16, 8 frames, 192 pairs.  Three replays of the captured step leave the losses,
    the gradient norms and every parameter / Adam moment three plain launches leave, bit for bit -- the number the bench reports is
    measured on the same arithmetic the oracle-checked eager step does (test_full_size_step_properties ties that one to the oracle)."""
    from tvts_amd import arch as A
    a, oarch = A.ARCHS["B_16"], O.ARCHS["B_16"]
    P = O.synth_params(oarch, seed=21)
    batch = O.synth_batch(oarch, B=192, T=8, seed=23, caption_len=32)
    me, _, le, ge = _three_steps(a, P, batch, "eager")
    flat_e, m_e, v_e = me.store.flat.clone(), me.store.m.clone(), me.store.v.clone()
    del me
    mg, _, lg, gg = _three_steps(a, P, batch, "graph")
    assert all(np.isfinite(x) for x in le + ge) and le[2] < le[0]  # it trains
    assert lg == le and gg == ge, (lg, le, gg, ge)
    assert torch.equal(mg.store.flat, flat_e) and torch.equal(mg.store.m, m_e) and torch.equal(mg.store.v, v_e)


@pytest.mark.parametrize("arch_name", ["B_16", "H_14"])
def test_fused_adamw_on_the_whole_parameter_set(K, lib, arch_name):
    """the optimizer at its real size (H/14: one flat buffer of a billion fp32 parameters, offsets past 2^31 bytes): two fused
    steps over random gradients against the per-tensor HF-AdamW restatement run tensor by tensor -- every trainable parameter
    and both moments, the frozen ones bit for bit where they were, the bf16 shadows the rounded master weights"""
    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base
    a = A.ARCHS[arch_name]
    m = TVTSv2Base(ARGS, arch=a, init_seed=0)
    for name, p in m.named_parameters():
        p.requires_grad = A.param_group_of(name, a) >= 0
    _, opt, _ = _runner_of(m, a)
    m._fresh_shadows(); m._sync_requires_grad()
    st = m.store
    gen = torch.Generator(device=DEV).manual_seed(5)
    names = [n for n, _ in m.named_parameters()]
    init = {n: st.p(n).clone() for n in names}
    ref = {n: (init[n].clone(), torch.zeros_like(init[n]), torch.zeros_like(init[n])) for n in names}
    for step in (1, 2):
        st.grad.normal_(generator=gen).mul_(1e-2 * step)
        g = {n: st.g(n).clone() for n in names}
        opt.step()
        for n, (pr, mr, vr) in ref.items():
            gi = A.param_group_of(n, a)
            if gi >= 0:
                O.hf_adamw_step(pr, g[n], mr, vr, step, A.GROUP_HPARAMS[gi][0], A.GROUP_HPARAMS[gi][1])
    torch.cuda.synchronize()
    moved = 0
    for n, (pr, mr, vr) in ref.items():
        if A.param_group_of(n, a) < 0:
            assert torch.equal(st.p(n), init[n]), n  # frozen: bit for bit where it was
            continue
        # the update is lr-sized (1e-4 ... 1e-7 of a parameter): compare the MOVE, not the value
        move = float((pr - init[n]).abs().max())
        assert move > 0, n
        tol = 1e-4 * move + 2.4e-7 * float(pr.abs().max())  # (+ the last bit of the value: the kernel fuses multiply-adds)
        assert float((st.p(n) - pr).abs().max()) <= tol, (n, float((st.p(n) - pr).abs().max()), move)
        moved += 1
    assert moved > 100
    assert int(st.flat.numel()) * 4 > 2 ** 31 or arch_name != "H_14"  # (H/14: the flat buffer does reach past 2^31 bytes)


def test_captured_step_follows_the_learning_rate_schedule(K, lib):
    """lr / weight decay live in a device table that sync_hyper() refreshes: a replayed graph applies the new learning
    rate without being captured again (the epoch-end x0.1 of trainer.py:402-417)."""
    from tvts_amd import arch as A
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    P = O.synth_params(oarch, seed=3)
    batch = O.synth_batch(oarch, B=4, T=2, seed=4, caption_len=9)
    m, opt, run = _runner(a, P, lr_mul=10.0)
    pb = m.engine.prepare_batch(batch)
    lab = batch["label"].reshape(-1).to(torch.int32).to(DEV)
    m._fresh_shadows(); m._sync_requires_grad()
    run.run(pb, lab, device_step=True)  # eager warm-up (allocates workspaces, uploads the table)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run.run(pb, lab, device_step=True)
    key = "pred_model.head.weight"
    w0 = m.store.p(key).clone()
    g.replay(); torch.cuda.synchronize()
    d1 = float((m.store.p(key) - w0).abs().mean())
    for grp in opt.param_groups:
        grp["lr"] = 0.0
        grp["weight_decay"] = 0.0
    opt.sync_hyper()
    w1 = m.store.p(key).clone()
    g.replay(); torch.cuda.synchronize()
    assert d1 > 0 and torch.equal(m.store.p(key), w1)


def test_range_wise_adamw_gives_the_bits_of_the_single_launch(K, lib):
    """arch["adamw_ranges"] (opt-in, measured slower): the fused AdamW launched range by range on its own stream as the backward
    finishes each parameter range, the rest by step() -- three steps leave the parameters, both moments and the transposed shadows
    of the single launch behind the backward, bit for bit, eagerly and replayed."""
    from tvts_amd import arch as A
    oarch = O.tiny_arch(**A.small_arch())
    P = O.synth_params(oarch, seed=21)
    batch = O.synth_batch(oarch, B=4, T=3, seed=22, caption_len=9)
    res = {}
    for ranged in (False, True):
        a = dict(A.small_arch(), adamw_ranges=ranged)
        for mode in ("eager", "graph"):
            m, opt, losses, gn = _three_steps(a, P, batch, mode)
            res[(ranged, mode)] = (m.store.flat.clone(), m.store.m.clone(), m.store.v.clone(), m.store.shadow_t.clone(), losses)
    ref = res[(False, "eager")]
    for k, v in res.items():
        for x, y in zip(ref[:4], v[:4]):
            assert torch.equal(x, y), k
        assert v[4] == ref[4], k
