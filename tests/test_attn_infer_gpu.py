"""Forward-only attention calls (lse2 = None): the fused SPACE kernel for full-frame groups (112 < n + 1 <= 272) against float64
torch per (row, head), and the geometries that keep today's kernels bit for bit against the call that stores the log-sum-exp."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
from oracle import tvts_oracle as O  # noqa: E402  (checker only)

DEV = "cuda:0"
OUT_TOL = 7e-3  # test_kernels_gpu.py ATTN_ROW_TOL["out"]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def _qkv(rows, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(rows, 3 * W, generator=g, device=DEV).bfloat16()


def _ws(B, heads, T, n, dh):
    return torch.full((B * heads * max(T, -(-n // 28)) * (dh + 2),), float("nan"), device=DEV)


GEOS = [(n, T, B, 64) for n in (112, 150, 196, 256) for T in (1, 3, 12) for B in (1, 2)] + \
       [(n, T, B, 80) for n in (196, 256) for T in (1, 3, 12) for B in (1, 2)]


@pytest.mark.parametrize("n,T,B,dh", GEOS)
def test_full_frame_space_forward(K, n, T, B, dh):
    heads = 2
    S, W = 1 + T * n, heads * dh
    qkv = _qkv(B * S, W, seed=n + 7 * T + B + dh)
    ref = O.divided_attention_core(qkv.view(B, S, 3 * W).double(), heads, "space", T, n).reshape(B * S, W)
    outs = []
    for _ in range(2):
        buf, out = KB.guarded(B * S, W, torch.bfloat16, DEV)
        K.attn_fwd_divided("space", qkv, out, None, _ws(B, heads, T, n, dh), B=B, heads=heads, S=S, T=T, n=n, head_dim=dh)
        torch.cuda.synchronize()
        KB.check_guards(buf, B * S, W, "full-frame space out")
        outs.append(out)
    what = f"space fwd-only n={n} T={T} B={B} dh={dh}"
    KB.assert_rows_within(outs[0], ref, OUT_TOL, groups=heads, what=what, out_dtype=torch.bfloat16)
    cls = torch.arange(B, device=DEV) * S
    KB.assert_rows_within(outs[0][cls], ref[cls], OUT_TOL, groups=heads, what=what + " (CLS rows)", out_dtype=torch.bfloat16)
    KB.assert_equal_bits(outs[1], outs[0], what + ": second run")


def _pair(run):
    """run(out, lse) once with an lse buffer and once with None -> the two outputs"""
    a, b = run(True), run(False)
    torch.cuda.synchronize()
    return a, b


@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("mode,B,T,n,fused", [("space", 2, 4, 98, True), ("space", 1, 12, 49, True), ("time", 2, 12, 196, True),
                                              ("time", 1, 16, 76, True), ("space", 2, 3, 196, False),
                                              ("space", 2, 3, 16, True), ("time", 2, 20, 29, True), ("time", 2, 31, 3, True)])
def test_divided_forward_only_keeps_the_bits(K, mode, B, T, n, fused, dh):
    """fused SPACE (n + 1 <= 112) and TIME: the same kernels with the LSE store skipped; the split SPACE path (fused=False at
    n = 196: the streaming kernel + the CLS-query pass) likewise.  The last three: a SPACE tile with one live row, the last size of
    the TIME <2, 20> class with a one-position last chunk, the largest TIME tile with waves that own no group"""
    heads = 2
    S, W = 1 + T * n, heads * dh
    qkv = _qkv(B * S, W, seed=3 * n + T)

    def run(with_lse):
        out = torch.zeros(B * S, W, dtype=torch.bfloat16, device=DEV)
        lse = torch.empty(B * S, heads, device=DEV) if with_lse else None
        # (calls with lse2 take today's kernels whatever the fused option; the forward-only one follows it)
        K.attn_fwd_divided(mode, qkv, out, lse, _ws(B, heads, T, n, dh), B=B, heads=heads, S=S, T=T, n=n, head_dim=dh,
                           fused=True if with_lse else fused)
        return out
    a, b = _pair(run)
    KB.assert_equal_bits(b, a, f"{mode} n={n} T={T} forward-only")


@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("B,S,causal", [(6, 32, True), (3, 77, True), (2, 150, False)])
def test_full_attention_forward_only_keeps_the_bits(K, B, S, causal, dh):
    heads = 2
    W = heads * dh
    qkv = _qkv(B * S, W, seed=S + B)

    def run(with_lse):
        out = torch.zeros(B * S, W, dtype=torch.bfloat16, device=DEV)
        K.attn_fwd("full", qkv, out, torch.empty(B * S, heads, device=DEV) if with_lse else None, B=B, heads=heads, S=S,
                   causal=causal, head_dim=dh)
        return out
    a, b = _pair(run)
    KB.assert_equal_bits(b, a, f"full S={S} forward-only")


@pytest.mark.parametrize("dh", [64, 80])
def test_rowq_and_cls_forward_only_keep_the_bits(K, dh):
    heads, B, L = 2, 5, 29
    W = heads * dh
    qkv = _qkv(B * L, W, seed=11)
    pos = torch.tensor([3, 28, 0, 17, 9], dtype=torch.int32, device=DEV)

    def rowq(with_lse):
        out = torch.zeros(B * L, W, dtype=torch.bfloat16, device=DEV)
        K.attn_fwd_rowq(qkv, pos, out, torch.empty(B * L, heads, device=DEV) if with_lse else None, B=B, heads=heads, S=L, head_dim=dh)
        return out
    a, b = _pair(rowq)
    KB.assert_equal_bits(b, a, "rowq forward-only")
    Bv, T, n = 2, 12, 196
    S = 1 + T * n
    qv = _qkv(Bv * S, W, seed=12)

    def cls(with_lse):
        out = torch.zeros(Bv * S, W, dtype=torch.bfloat16, device=DEV)
        K.attn_fwd("cls", qv, out, torch.empty(Bv * S, heads, device=DEV) if with_lse else None, B=Bv, heads=heads, S=S, T=T, n=n,
                   head_dim=dh)
        return out
    a, b = _pair(cls)
    KB.assert_equal_bits(b, a, "CLS query forward-only")
