"""CPU self-test of tests/kernel_bounds.py: the per-element GEMM bound is SOUND (the same product summed in fp32 in other orders
passes it) and SHARP (each seeded corruption of an output tensor fails it, where the whole-tensor rel-L2 gate of the kernel tests
lets the same corruption through).  Only output tensors are corrupted; no kernel is involved."""
import math

import torch

import kernel_bounds as KB

torch.set_num_threads(min(8, torch.get_num_threads()))


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def operands(M, N, Kd, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, Kd, generator=g).bfloat16()
    b = (torch.randn(N, Kd, generator=g) * Kd ** -0.5).bfloat16()
    bias = torch.randn(N, generator=g)
    return a, b, bias


def check(got, a, b, **kw):
    """check_gemm; -> the worst used share of the bound's accumulation term (the total ratio of a correctly rounded bf16 result
    reaches ~1 through its rounding term alone)"""
    KB.pop_acc_worst()
    KB.check_gemm(got, a, b, what="product", **kw)
    return KB.pop_acc_worst()


def fails(fn, *words):
    try:
        fn()
    except AssertionError as e:
        msg = str(e)
        for w in words:
            assert w in msg, (w, msg)
        return msg
    raise AssertionError("the corruption passed the check")


# ------------------------------------------------------------------------------------------------ sound
def sums_in_other_orders(a, b, bias):
    """the same fp32 product summed in four orders: 32-wide K chunks, reversed K, pairwise, the bias before the last chunk"""
    af, bf = a.float(), b.float()
    Kd = a.shape[1]
    P = af[:, None, :] * bf[None, :, :]          # exact products (bf16 x bf16 fits in fp32)
    out = {}
    acc = torch.zeros(a.shape[0], b.shape[0])
    for k0 in range(0, Kd, 32):
        acc = acc + P[..., k0:k0 + 32].sum(-1)  # a chunk's own sum, then the running one: an MFMA K-step chain
    out["chunked"] = acc + bias
    acc = bias.expand(a.shape[0], -1).clone()
    for k in range(Kd - 1, -1, -1):
        acc = acc + P[..., k]
    out["reversed"] = acc
    t = P
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = torch.cat([t, torch.zeros_like(t[..., :1])], -1)
        t = t[..., 0::2] + t[..., 1::2]
    out["pairwise"] = t[..., 0] + bias
    acc = torch.zeros(a.shape[0], b.shape[0])
    last = max(0, Kd - 64)
    for k0 in range(0, last, 64):
        acc = acc + P[..., k0:k0 + 64].sum(-1)
    out["bias_before_last_chunk"] = (acc + bias) + P[..., last:].sum(-1)
    return out


def test_bound_holds_for_every_summation_order():
    worst = {}
    for (M, N, Kd) in ((40, 24, 64), (24, 16, 768), (12, 8, 3072)):
        a, b, bias = operands(M, N, Kd, seed=Kd)
        for name, v in sums_in_other_orders(a, b, bias).items():
            for dt in (torch.float32, torch.bfloat16):
                worst[(Kd, name, str(dt))] = check(v.to(dt), a, b, bias=bias)
    assert max(worst.values()) <= 0.5, max(worst.items(), key=lambda kv: kv[1])
    # the fp32 orders really differ from one another: the bound is not passing one value against itself
    a, b, bias = operands(12, 8, 3072, seed=3072)
    o = sums_in_other_orders(a, b, bias)
    assert not torch.equal(o["chunked"], o["reversed"]) and not torch.equal(o["pairwise"], o["bias_before_last_chunk"])


def test_bound_holds_for_fp8_decoded_operands_with_scales_and_residual():
    g = torch.Generator().manual_seed(5)
    M, N, Kd = 32, 24, 512
    a8 = (torch.randn(M, Kd, generator=g) * 60).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    b8 = (torch.randn(N, Kd, generator=g) * 60).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    sa = torch.rand(M, generator=g, dtype=torch.float64) * 1e-3 + 1e-4  # one scale per row
    sb = 3.1e-3
    res = torch.randn(M, N, generator=g)
    ad, bd = KB.decode_e4m3(a8).float(), KB.decode_e4m3(b8).float()
    acc = torch.zeros(M, N)
    for k0 in range(Kd - 128, -1, -128):                             # K = 128 blocks, last block first
        acc = acc + ad[:, k0:k0 + 128] @ bd[:, k0:k0 + 128].t()
    v = (acc * (sa.float()[:, None] * sb)) + res
    for dt in (torch.float32, torch.bfloat16):
        assert check(v.to(dt), KB.decode_e4m3(a8), KB.decode_e4m3(b8), scale=sa * sb, residual=res) <= 0.5


def test_activation_and_gate_bounds_hold_for_fp32_evaluations():
    a, b, bias = operands(64, 48, 768, seed=11)
    pre = a.float() @ b.float().t() + bias
    h = (torch.randn(64, 48, generator=torch.Generator().manual_seed(2)) * 2).bfloat16()
    z = a.float() @ b.float().t()
    for act in ("quick_gelu", "gelu"):
        y = KB.act_ref(pre.double(), act).float()
        assert check(y.bfloat16(), a, b, bias=bias, act=act, preact=pre.bfloat16()) <= 0.5
        assert check(y, a, b, bias=bias, act=act) <= 0.5
        gz = z * KB.act_deriv_ref(h.double(), act).float()
        assert check(gz.bfloat16(), a, b, gate_h=h, gate_act=act) <= 0.5
        d = KB.act_deriv_ref(pre.double(), act).float()
        assert check(y.bfloat16(), a, b, bias=bias, act=act, preact=d.bfloat16(), deriv=True) <= 0.5
        assert check((z * h.float()).bfloat16(), a, b, gate_h=h, gate_act=act, deriv=True) <= 0.5
        # a wrong activation (the tanh approximation of GELU / QuickGELU swapped) fails at fp32 output
        other = "gelu" if act == "quick_gelu" else "quick_gelu"
        fails(lambda: check(KB.act_ref(pre.double(), other).float(), a, b, bias=bias, act=act), "outside the bound")


# ------------------------------------------------------------------------------------------------ sharp
def test_seeded_corruptions_fail_the_bound_but_pass_the_rel_gate():
    """the headline projection's shape (M = 150 720 rows = 588 tiles of 256 + a ragged tile of 192, N = 768); K is cut to 64:
    the bf16 rounding noise a rel gate sees does not depend on K (1.6e-3 here as at K = 768)"""
    M, N, Kd = 150720, 768, 64
    a, b, bias = operands(M, N, Kd, seed=1)
    ref = a.float() @ b.float().t() + bias
    clean = ref.bfloat16()
    noise = rel(clean.float(), ref)
    assert 1.4e-3 < noise < 1.9e-3, noise
    assert check(clean, a, b, bias=bias, chunk=16384) <= 0.5

    def corrupt(fn):
        x = clean.clone()
        fn(x)
        return x

    cases = {
        "last row = the row above": (corrupt(lambda x: x[-1].copy_(x[-2])), (M - 1, None)),
        "one 16x16 block transposed": (corrupt(lambda x: x[4096:4112, 512:528].copy_(x[4096:4112, 512:528].t().clone())), None),
        "one value negated": (corrupt(lambda x: x[77777, 300].neg_()), (77777, 300)),
        # one 16 x 16 fragment of the ragged last tile (rows 150 528 .. 150 719) written one 16-row slab too low
        "ragged-tail fragment shifted by one slab": (corrupt(lambda x: x[M - 176:M - 160, 48:64].copy_(x[M - 192:M - 176, 48:64].clone())),
                                                     (M - 176, 48)),
    }
    # a kernel that truncates its fp32 results to bf16 instead of rounding them to nearest: up to a whole ulp off
    trunc = (ref.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    assert rel(trunc.float(), ref) < 4e-3, rel(trunc.float(), ref)
    fails(lambda: check(trunc, a, b, bias=bias, chunk=16384), "outside the bound")
    for name, (got, where) in cases.items():
        assert rel(got.float(), ref) < 4e-3, (name, rel(got.float(), ref))  # the old gate: passes
        msg = fails(lambda: check(got, a, b, bias=bias, chunk=16384), "outside the bound", "tile", "slab")
        if where is not None:
            r, c = where
            assert f"(row {r}, col {c if c is not None else ''}" in msg, (name, msg)


def test_sixteen_zeroed_values_of_one_row_fail_at_k3072():
    M, N, Kd = 9420, 768, 3072
    a, b, _ = operands(M, N, Kd, seed=2)
    ref = a.float() @ b.float().t()
    got = ref.bfloat16()
    got[5000, 256:272] = 0
    assert rel(got.float(), ref) < 4e-3
    msg = fails(lambda: check(got, a, b), "16 of", "(row 5000, col 256)", "tile (19, 1)", "column group 16")
    assert "slab 8 of that tile" in msg, msg


def test_fp32_outputs_catch_a_single_wrong_element():
    a, b, bias = operands(2000, 256, 768, seed=4)
    ref = a.float() @ b.float().t() + bias
    got = ref.clone()
    got[1234, 200] = float(torch.nextafter(got[1234, 200], torch.tensor(math.inf)))  # 1 ulp: still within the bound
    assert check(got, a, b, bias=bias) < 0.5
    got[1234, 200] *= 1.01                                                           # 1 % off in one element of 512 000
    assert rel(got, ref) < 2e-5                                                      # the whole-tensor fp32 gate: passes
    fails(lambda: check(got, a, b, bias=bias), "1 of", "(row 1234, col 200)")
    got[1234, 200] = float("nan")
    fails(lambda: check(got, a, b, bias=bias), "1 non-finite")


def test_rows_within_catches_one_attention_row_and_one_head_slice():
    g = torch.Generator().manual_seed(9)
    R, heads, dh = 8192, 8, 64
    ref = torch.randn(R, heads * dh, generator=g, dtype=torch.float64)
    got = (ref + 2e-3 * torch.randn(R, heads * dh, generator=g, dtype=torch.float64)).float()
    worst = KB.assert_rows_within(got, ref, 8e-3, groups=heads)
    assert worst < 4e-3
    row = got.clone()
    row[1000] = row[1001]                                   # one attention row replaced by its neighbour
    assert rel(row, ref) < 2e-2                             # the attention backward gate: passes
    fails(lambda: KB.assert_rows_within(row, ref, 8e-3, groups=heads), "8 of", "[1000, 0]")
    head = got.clone()
    head[3000, 5 * dh:6 * dh] = head[3000, 4 * dh:5 * dh]   # one head slice replaced by the neighbouring head
    assert rel(head, ref) < 8e-3                            # the attention forward gate: passes
    fails(lambda: KB.assert_rows_within(head, ref, 8e-3, groups=heads), "1 of", "[3000, 5]")
    # per-column vectors (dgamma / dbeta): one column off by 1 % fails, the whole-vector rel stays under 1e-4 at W = 1280
    dg = torch.randn(1280, generator=g, dtype=torch.float64)
    bad = dg.clone()
    bad[700] *= 1.01
    assert rel(bad, dg) < 1e-3
    fails(lambda: KB.assert_rows_within(bad, dg, 1e-3), "[700, 0]")


def test_guards_and_exact_bits():
    buf, out = KB.guarded(10, 12, torch.bfloat16, "cpu")
    out.fill_(1.0)
    KB.check_guards(buf, 10, 12)
    assert out.stride(0) == 20
    buf[3, 12] = 0
    fails(lambda: KB.check_guards(buf, 10, 12), "columns past 12")
    buf[3, 12] = float("nan")
    buf[10, 0] = 0
    fails(lambda: KB.check_guards(buf, 10, 12), "rows past 10")
    qb, q = KB.guarded(4, 16, torch.uint8, "cpu")
    q.zero_()
    KB.check_guards(qb, 4, 16)
    x = torch.randn(300, 40).bfloat16()
    KB.assert_equal_bits(x, x.clone())
    y = x.clone()
    y[299, 39] = -y[299, 39]
    fails(lambda: KB.assert_equal_bits(y, x), "1 of", "(row 299, col 39)", "tile (1, 0)")


def test_layernorm_bounds_hold_for_fp32_torch_and_catch_a_wrong_row():
    g = torch.Generator().manual_seed(12)
    M, W = 3001, 768
    x = torch.randn(M, W, generator=g) * 2 + 0.3
    gamma, beta = 1 + 0.1 * torch.randn(W, generator=g), 0.1 * torch.randn(W, generator=g)
    y, mean, rstd = torch.native_layer_norm(x, [W], gamma, beta, 1e-5)
    mean, rstd = mean[:, 0], rstd[:, 0]
    KB.pop_acc_worst()
    assert KB.ln_fwd_check(x, gamma, beta, 1e-5, y, mean, rstd, what="ln fwd") <= 1.0
    assert KB.ln_fwd_check(x, gamma, beta, 1e-5, y.bfloat16(), what="ln fwd bf16") <= 1.0
    assert KB.pop_acc_worst() <= 0.5
    bad = y.bfloat16()
    bad[2999] = bad[3000]                                            # a ragged-tail row from its neighbour
    fails(lambda: KB.ln_fwd_check(x, gamma, beta, 1e-5, bad, what="ln fwd"), "(row 2999")
    dy = torch.randn(M, W, generator=g).bfloat16()
    res1 = torch.randn(M, W, generator=g)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, [W], gr, br, 1e-5).backward(dy.float())
    dx = xr.grad + res1
    kw = dict(res1=res1, what="ln bwd", col_tol=1e-4)
    cw = {}
    assert KB.ln_bwd_check(dy, x, mean, rstd, gamma, dx=dx, dx_bf16=dx.bfloat16(), dgamma=gr.grad, dbeta=br.grad, col_worst=cw, **kw) <= 1.0
    assert KB.pop_acc_worst() <= 0.5
    assert max(cw.values()) < 1e-4 / 3, cw
    bad = dx.clone()
    bad[1500, 17] += 1e-3
    fails(lambda: KB.ln_bwd_check(dy, x, mean, rstd, gamma, dx=bad, **kw), "(row 1500, col 17)")
    dg = gr.grad.clone()
    dg[100] *= 1.001                                                 # one column 0.1 % off: the whole-vector gate 1e-4 passes it
    assert rel(dg, gr.grad) < 1e-4
    fails(lambda: KB.ln_bwd_check(dy, x, mean, rstd, gamma, dgamma=dg, **kw), "dgamma", "[100, 0]")


# ------------------------------------------------------------------------------------------------ attention references
from oracle import tvts_oracle as O  # noqa: E402
from oracle import tvts_v1_oracle as V  # noqa: E402

TOL = KB.ATTN_ROW_TOL


def attn_inputs(B, S, heads, dh, seed):
    """bf16-valued qkv [B, S, 3W] and dO [B, S, W] in float64"""
    g = torch.Generator().manual_seed(seed)
    W = heads * dh
    return torch.randn(B, S, 3 * W, generator=g).bfloat16().double(), torch.randn(B, S, W, generator=g).bfloat16().double()


def _identity(qkv, dO, heads, dh, q_rows=None, **kw):
    """attn_bwd_same_inputs on the exact float64 output and log-sum-exp against float64 autograd of the same restriction"""
    dOz = dO if q_rows is None else dO * q_rows[..., None]
    out, ref = KB.attn_autograd(qkv, dOz, heads, dh, **kw)
    _, lse2, _ = KB.attn_fwd_ref(qkv, heads, dh, **kw)
    if q_rows is not None:  # what a query-subset kernel leaves in the rows it does not own must not matter
        nanrow = ~q_rows[..., None]
        dO = dO.masked_fill(nanrow, float("nan"))
        out, lse2 = out.masked_fill(nanrow, float("nan")), lse2.masked_fill(nanrow, float("nan"))
    got = KB.attn_bwd_same_inputs(qkv, dO, out, lse2, heads, dh, q_rows=q_rows, **kw)
    assert torch.isfinite(got).all()
    assert rel(got, ref) < 1e-10, rel(got, ref)
    W = heads * dh
    for i in range(3):
        assert rel(got[..., i * W:(i + 1) * W], ref[..., i * W:(i + 1) * W]) < 1e-10
    return ref


def test_attention_same_inputs_reference_is_autograd_on_exact_inputs():
    heads, dh = 3, 16
    qkv, dO = attn_inputs(3, 37, heads, dh, seed=21)
    B, S = 3, 37
    _identity(qkv, dO, heads, dh)
    _identity(qkv, dO, heads, dh, causal=True)
    lens = torch.tensor([0, 17, 37])                      # 0 is clamped to 1
    ref = _identity(qkv, dO * (torch.arange(S)[None, :] < lens.clamp(1)[:, None])[..., None], heads, dh, kv_len=lens)
    assert (ref[1, 17:, heads * dh:] == 0).all() and (ref[0, 1:, heads * dh:] == 0).all()  # padded keys: no dK / dV
    mask = V.drop_mask(77, 3, (B, heads, S, S), 0.25)
    _identity(qkv, dO, heads, dh, kv_len=lens, drop_mask=mask, p=0.25)
    out_d, _, P = KB.attn_fwd_ref(qkv, heads, dh, drop_mask=mask, p=0.25)
    v = qkv[..., 2 * heads * dh:].reshape(B, S, heads, dh).permute(0, 2, 1, 3)
    assert rel(out_d, ((P * mask.double()) @ v).permute(0, 2, 1, 3).reshape(B, S, -1)) < 1e-7  # the oracle's mask carries 1/(1-p), in fp32
    tail = torch.zeros(B, S, dtype=torch.bool)
    tail[:, S - 4:] = True
    _identity(qkv, dO, heads, dh, q_rows=tail)
    rowq = torch.zeros(B, S, dtype=torch.bool)
    qpos = torch.tensor([0, 16, 36])
    rowq[torch.arange(B), qpos] = True
    ref = _identity(qkv, dO, heads, dh, q_rows=rowq, causal=True)
    assert (ref[1, 17:, heads * dh:] == 0).all()          # keys behind the query: no dK / dV
    # the forward reference against the whole-tensor tests' formulation
    s = (qkv[..., :48].reshape(B, S, heads, dh).permute(0, 2, 1, 3) * dh ** -0.5) @ \
        qkv[..., 48:96].reshape(B, S, heads, dh).permute(0, 2, 3, 1)
    out, lse2, _ = KB.attn_fwd_ref(qkv, heads, dh)
    assert rel(out, (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, S, -1)) < 1e-14
    assert rel(lse2, (torch.logsumexp(s, -1) * KB.LOG2E).permute(0, 2, 1)) < 1e-14


def test_divided_same_inputs_reference_is_autograd_of_the_oracle():
    heads, dh, B = 3, 16, 2
    for mode, T, n in (("space", 3, 5), ("time", 4, 3)):
        S = 1 + T * n
        al = KB.divided_allowed(mode, T, n)
        assert al[0].all() and al[:, 0].all() and int(al[1:, 1:].sum()) == T * n * (n if mode == "space" else T)
        qkv, dO = attn_inputs(B, S, heads, dh, seed=31)
        x = qkv.clone().requires_grad_(True)
        ro = O.divided_attention_core(x, heads, mode, T, n)
        ro.backward(dO)
        out, lse2, _ = KB.divided_fwd_ref(qkv, heads, dh, mode, T, n)
        assert rel(out, ro.detach()) < 1e-14
        got = KB.divided_bwd_same_inputs(qkv, dO, out, lse2, heads, dh, mode, T, n)
        assert rel(got, x.grad) < 1e-10, (mode, rel(got, x.grad))
        assert rel(got[:, 0], x.grad[:, 0]) < 1e-10


def test_delta_from_the_bf16_output_limits_dq_where_a_query_has_few_keys():
    """The recorded answer to the split divided backward's "time-mode dQ reaches 0.105 in a few slices of B/16": no kernel is
    involved.  B/16 time geometry (9 keys per patch query), bf16-valued randn inputs: dQ formed with delta = rowsum(dO o bf16(O))
    against dQ with the exact delta is off by > 0.05 in its worst (row, head) slice (0.117 measured, 45 of 18 816 patch slices
    above 1.2e-2), because dP - delta cancels and the rounding of O shows through; FULL attention over 200 keys stays < 4e-3."""
    c = KB.DIVIDED["B16"]
    B, T, n, heads, dh = 2, c["T"], c["n"], c["heads"], c["dh"]
    S = 1 + T * n
    qkv, dO = attn_inputs(B, S, heads, dh, seed=5)
    e = KB.attn_conditioning(qkv, dO, heads, dh, allowed=KB.divided_allowed("time", T, n))
    patch = e["dq"].reshape(B, S, heads)[:, 1:]
    worst, above = float(patch.max()), int((patch > TOL["dq"]).sum())
    print(f"CONDITIONING time B/16 dq worst {worst:.4g}, {above} of {patch.numel()} patch slices above {TOL['dq']:g}; "
          f"dk {float(e['dk'].max()):.4g} dv {float(e['dv'].max()):.4g}")
    assert worst > 0.05 and above > 0, (worst, above)
    assert float(e["dv"].max()) < 1e-12                    # dV does not read delta
    qkv, dO = attn_inputs(2, 200, 3, 64, seed=5)
    e = KB.attn_conditioning(qkv, dO, 3, 64)
    full = max(float(v.max()) for v in e.values())
    print(f"CONDITIONING full S=200 worst {full:.4g}")
    assert full < 4e-3, full


def _thirds(t, W):
    return {"dq": t[..., :W], "dk": t[..., W:2 * W], "dv": t[..., 2 * W:]}


def _gate_passes_rows_fail(got, ref, heads, tol, gate, where):
    """the corruption passes the whole-tensor gate and fails assert_rows_within, which names the (row, head) slice"""
    W = ref.shape[-1]
    g2, r2 = got.reshape(-1, W), ref.reshape(-1, W)
    assert rel(g2, r2) < gate, rel(g2, r2)
    fails(lambda: KB.assert_rows_within(g2, r2, tol, groups=heads), f"[{where[0]}, ")


def test_seeded_attention_corruptions_fail_per_row_but_pass_the_whole_tensor_gates():
    """each corruption is an off-by-one a tiled kernel can make; `got` is float64-derived (the reference recomputed with the
    fault), the clean result passes at ATTN_ROW_TOL / 100"""
    heads, dh = 3, 64
    W = heads * dh
    # ---- one causal row that also sees key qi + 1 (a per-wave causal key limit one too high)
    B, S = 2, 129
    qkv, dO = attn_inputs(B, S, heads, dh, seed=41)
    out, _, _ = KB.attn_fwd_ref(qkv, heads, dh, causal=True)
    al = torch.ones(S, S, dtype=torch.bool).tril().repeat(B, 1, 1, 1)
    al[1, 0, 63, 64] = True
    bad, _, _ = KB.attn_fwd_ref(qkv, heads, dh, allowed=al)
    KB.assert_rows_within(out.reshape(-1, W), out.reshape(-1, W), TOL["out"] / 100, groups=heads)
    _gate_passes_rows_fail(bad, out, heads, TOL["out"], 8e-3, (S + 63,))
    # ---- key 64 missing from the softmax of a single row at S = 65 (the last key tile holds one key)
    B, S = 16, 65
    qkv, dO = attn_inputs(B, S, heads, dh, seed=42)
    out, _, _ = KB.attn_fwd_ref(qkv, heads, dh)
    al = torch.ones(B, 1, S, S, dtype=torch.bool)
    al[0, 0, 40, 64] = False
    bad, _, _ = KB.attn_fwd_ref(qkv, heads, dh, allowed=al)
    _gate_passes_rows_fail(bad, out, heads, TOL["out"], 8e-3, (40,))
    # ---- kv_len off by one for one sequence of 512 (the GPU test's lengths, 64 times over: the one extra key changes every row
    # of its sequence by ~ 1 / sqrt(length), which the whole-tensor gates pass once the batch has ~ 16 000 rows)
    B, S, h1 = 512, 130, 1
    lens = torch.tensor([1, 2, 63, 64, 65, 128, 129, 130]).repeat(64)
    qkv, dO = attn_inputs(B, S, h1, dh, seed=43)
    qkv = qkv * 0.5                                        # the scale test_full_attention_with_padded_keys draws its inputs at
    dO = dO * (torch.arange(S)[None, :] < lens[:, None])[..., None]
    out, ref = KB.attn_autograd(qkv, dO, h1, dh, kv_len=lens)
    off = lens.clone()
    off[3] = 65
    bout, bad = KB.attn_autograd(qkv, dO, h1, dh, kv_len=off)
    valid = (torch.arange(S)[None, :] < lens[:, None])
    _gate_passes_rows_fail(bout[valid], out[valid], h1, TOL["out"], 8e-3, (66,))  # first valid row of sequence 3
    for nm in ("dq", "dk", "dv"):
        _gate_passes_rows_fail(_thirds(bad, dh)[nm], _thirds(ref, dh)[nm], h1, TOL[nm], 2e-2, (3 * S,))
    # ---- the one-row form's query of one sequence taken at qpos + 1.  The form has ONE output row per sequence and the wrong
    # row is wrong altogether (relative error ~ 1.4), so the forward gate passes it only from ~ 30 000 sequences on
    B, S = 32768, 20
    g = torch.Generator().manual_seed(44)
    qpos = torch.randint(0, S - 1, (B,), generator=g)
    qkv, dO = attn_inputs(B, S, h1, dh, seed=44)
    rows = torch.zeros(B, S, dtype=torch.bool)
    rows[torch.arange(B), qpos] = True
    out, ref = KB.attn_autograd(qkv, dO * rows[..., None], h1, dh, causal=True)
    wrong = rows.clone()
    wrong[4, qpos[4]], wrong[4, qpos[4] + 1] = False, True
    dO2 = dO.clone()
    dO2[4, qpos[4] + 1] = dO[4, qpos[4]]                   # the upstream gradient is the query row's
    bout, bad = KB.attn_autograd(qkv, dO2 * wrong[..., None], h1, dh, causal=True)
    got_out = out[rows].clone()
    got_out[4] = bout[4, qpos[4] + 1]                      # the row the kernel would have stored at the query's place
    _gate_passes_rows_fail(got_out, out[rows], h1, TOL["out"], 8e-3, (4,))
    bad = bad.clone()
    bad[4, qpos[4], :dh], bad[4, qpos[4] + 1, :dh] = bad[4, qpos[4] + 1, :dh].clone(), 0.0   # its dQ lands in the query's row
    for nm in ("dq", "dk", "dv"):
        _gate_passes_rows_fail(_thirds(bad, dh)[nm], _thirds(ref, dh)[nm], h1, TOL[nm], 2e-2, (4 * S + (int(qpos[4]) if nm == "dq" else 0),))
    # ---- one tail query row swapped with its neighbour (two wrong rows: the forward gate passes them among ~ 130 000)
    B, S, nq = 8192, 24, 16
    qkv, dO = attn_inputs(B, S, h1, dh, seed=45)
    rows = torch.zeros(B, S, dtype=torch.bool)
    rows[:, S - nq:] = True
    out, ref = KB.attn_autograd(qkv, dO * rows[..., None], h1, dh)
    t_out, t_dq = out[:, S - nq:].clone(), ref[:, S - nq:, :dh].clone()
    t_out[1, [5, 6]], t_dq[1, [5, 6]] = t_out[1, [6, 5]], t_dq[1, [6, 5]]
    _gate_passes_rows_fail(t_out, out[:, S - nq:], h1, TOL["out"], 8e-3, (nq + 5,))
    _gate_passes_rows_fail(t_dq, ref[:, S - nq:, :dh], h1, TOL["dq"], 2e-2, (nq + 5,))
    # ---- one sequence's dK rows 32..63 zeroed (one 32-key half of one key tile never stored): 32 rows, passed among 131 072
    B, S = 2048, 64
    qkv, dO = attn_inputs(B, S, h1, dh, seed=46)
    _, ref = KB.attn_autograd(qkv, dO, h1, dh)
    bad = ref.clone()
    bad[5, 32:64, dh:2 * dh] = 0
    _gate_passes_rows_fail(_thirds(bad, dh)["dk"], _thirds(ref, dh)["dk"], h1, TOL["dk"], 2e-2, (5 * S + 32,))


def test_bf16_rounding_emulation_sits_inside_the_attention_tolerances():
    """The arbiter for a tolerance question: the references with the roundings the algorithm cannot avoid (`emulate`: P to bf16
    before P.V and P^T.dO, dS to bf16 before its two products, everything else float64) against the exact references on the same
    inputs.  Its worst (row, head) slice is 2.9e-3 .. 4.2e-3 over the geometries below -- the size of the kernels' own measured
    error -- and inside ATTN_ROW_TOL everywhere, so a kernel that misses the table is not explained by these roundings alone."""
    worst = {}
    for name, (B, S, heads, dh, kw) in {
            "full causal S 129": (2, 129, 3, 64, dict(causal=True)), "full S 197 dh 80": (2, 197, 3, 80, {}), "full S 33": (2, 33, 3, 64, {}),
            "time T 8 n 30": (2, 241, 3, 64, dict(allowed=KB.divided_allowed("time", 8, 30))),
            "space T 2 n 111 dh 80": (2, 223, 3, 80, dict(allowed=KB.divided_allowed("space", 2, 111)))}.items():
        W = heads * dh
        qkv, dO = attn_inputs(B, S, heads, dh, seed=len(name))
        out, lse2, _ = KB.attn_fwd_ref(qkv, heads, dh, **kw)
        e_out, e_lse2, _ = KB.attn_fwd_ref(qkv, heads, dh, emulate=True, **kw)
        assert torch.equal(lse2, e_lse2)                                     # the log-sum-exp is formed before any rounding
        O_read = out.bfloat16()
        exact = KB.attn_bwd_same_inputs(qkv, dO, O_read, lse2, heads, dh, **kw)
        emul = KB.attn_bwd_same_inputs(qkv, dO, O_read, lse2, heads, dh, emulate=True, **kw)
        w = {"out": float(KB.rows_rel(e_out.reshape(-1, W), out.reshape(-1, W), heads)[0].max())}
        for nm, a, b in zip(("dq", "dk", "dv"), _thirds(emul, W).values(), _thirds(exact, W).values()):
            w[nm] = float(KB.rows_rel(a.reshape(-1, W), b.reshape(-1, W), heads)[0].max())
        print("EMULATION", name, {k: f"{v:.3g}" for k, v in w.items()})
        for nm, v in w.items():
            assert TOL[nm] / 10 < v < TOL[nm], (name, nm, v)
            worst[nm] = max(worst.get(nm, 0.0), v)
    assert max(worst.values()) < 4.5e-3, worst


# ------------------------------------------------------------------------------------------------ embed / loss / AdamW helpers
def f32_sum_in_groups(parts, groups=16):
    """colsum_partials_kernel's order in fp32 torch: every group adds its partials p = g, g + 16, ... in order, the groups in order"""
    acc = torch.zeros(parts.shape[1])
    for g in range(groups):
        s = torch.zeros(parts.shape[1])
        for p in range(g, parts.shape[0], groups):
            s = s + parts[p]
        acc = acc + s
    return acc


def test_sum_bound_passes_fp32_orders_and_catches_a_missing_addend():
    """54 partials (18 clips x 3 slot groups) added into a non-zero output: three fp32 orders pass; the smallest addend missing from
    ONE column fails and the column is named"""
    g = torch.Generator().manual_seed(11)
    parts, init = torch.randn(54, 96, generator=g), torch.randn(96, generator=g)
    ref = parts.double().sum(0) + init.double()
    bound = KB.sum_bound(parts.double().abs().sum(0), 54, init=init)
    for got in (init + f32_sum_in_groups(parts), init + parts.sum(0), (init + parts.flip(0).cumsum(0)[-1])):
        assert KB.assert_within(got, ref, bound, "column sums") < 1.0
    col = 37
    k = int(parts[:, col].abs().argmin())  # the SMALLEST addend of that column
    bad = init + f32_sum_in_groups(parts)
    bad[col] -= parts[k, col]
    assert abs(float(parts[k, col])) < 0.05
    fails(lambda: KB.assert_within(bad, ref, bound, "column sums"), "row 37")  # (a 1-D output: its elements are the rows)
    # bf16 output form
    b16 = KB.sum_bound(parts.double().abs().sum(0), 54, torch.bfloat16, init=init, ref=ref)
    assert KB.assert_within((init + parts.sum(0)).bfloat16(), ref, b16, "bf16 column sums") <= 1.0


def test_bit_equality_catches_two_swapped_gathered_rows():
    g = torch.Generator().manual_seed(12)
    emb, pos = torch.randn(20, 32, generator=g), torch.randn(7, 32, generator=g)
    ids = torch.randint(0, 20, (3, 7), generator=g)
    want = (emb[ids] + pos).reshape(21, 32)
    KB.assert_equal_bits(want.clone(), want, "gather")
    bad = want.clone()
    bad[[4, 11]] = want[[11, 4]]
    assert rel(bad, want) > 0  # (a whole-tensor gate of 1e-6 sees this one too; the point is that the row is named)
    fails(lambda: KB.assert_equal_bits(bad, want, "gather"), "row 4")


def l2_standin(x, eps):
    e = torch.tensor(eps, dtype=torch.float32)
    nrm = (x * x).sum(1).sqrt()
    iv = 1.0 / torch.maximum(nrm, e)
    return x * iv[:, None], torch.where(nrm > e, iv, -iv)


def l2_bwd_standin(dxn, xn, inv):
    s = (xn * dxn).sum(1, keepdim=True)
    return torch.where((inv < 0)[:, None], -inv[:, None] * dxn, inv[:, None] * (dxn - xn * s))


def test_l2norm_checks_pass_fp32_and_catch_an_inverted_clamp_flag():
    g = torch.Generator().manual_seed(13)
    for E in (1, 64, 65, 512):
        x = torch.randn(9, E, generator=g)
        u = x[:5].double() / x[:5].double().norm(dim=1, keepdim=True)
        x[0] = 0.0
        x[1] = (u[1] * 1e-10).float()
        x[2] = 0.0
        x[2, E // 2] = KB.f32_const(1e-8)
        x[3], x[4] = (u[3] * 1e-3).float(), (u[4] * 1e3).float()
        xn, inv = l2_standin(x, 1e-8)
        assert KB.l2norm_check(x, 1e-8, xn, inv, what="l2norm") <= 1.0
        assert bool((inv[:3] < 0).all()) and bool((inv[3:] > 0).all())
        dxn = torch.randn(9, E, generator=g)
        assert KB.l2norm_bwd_check(dxn, xn, inv, l2_bwd_standin(dxn, xn, inv), what="l2norm_bwd") <= 1.0
        for row in (1, 4):  # a clamped row marked unclamped, an ordinary row marked clamped
            bad = inv.clone()
            bad[row] = -bad[row]
            fails(lambda: KB.l2norm_check(x, 1e-8, xn, bad, what="l2norm"), "clamp flag", f"row {row}")
        if E > 1:  # the backward follows the flag it reads: the other branch's values fail against it
            bad = inv.clone()
            bad[4] = -bad[4]
            fails(lambda: KB.l2norm_bwd_check(dxn, xn, bad, l2_bwd_standin(dxn, xn, inv), what="l2norm_bwd"), "row 4")


def infonce_standin(x, lse=None):
    G = x.shape[0]
    if lse is None:
        lse = torch.cat([torch.logsumexp(x, 1), torch.logsumexp(x, 0)])
    dx = (torch.exp(x - lse[:G, None]) + torch.exp(x - lse[None, G:]) - 2.0 * torch.eye(G)) / G
    loss = -(2.0 * x.diagonal() - lse[:G] - lse[G:]).sum() / G
    return lse, dx, loss


def test_infonce_check_passes_fp32_and_catches_one_column_lse_off_by_1e_5():
    """... which the old gates (rel < 1e-4 on dv / dt after the two GEMMs, 2e-5 on the loss) let through"""
    g = torch.Generator().manual_seed(14)
    G, E, temp = 65, 64, 0.05
    v, t = torch.randn(G, E, generator=g), torch.randn(G, E, generator=g)
    loss_ref, dv_ref, dt_ref, e_dv, e_dt = KB.contrastive_bound(v, t, temp, 1e-8)
    vn, vi = l2_standin(v, 1e-8)
    tn, ti = l2_standin(t, 1e-8)
    x = (vn @ tn.t()) * (1.0 / temp)
    lse, dx, loss = infonce_standin(x)
    res = KB.infonce_check(x, lse, dx, loss + 0.75, loss0=0.75, what="infonce")
    assert max(res.values()) <= 1.0, res

    def head(dx):
        dv = l2_bwd_standin((dx @ tn) * (1.0 / temp), vn, vi)
        return dv, l2_bwd_standin((dx.t() @ vn) * (1.0 / temp), tn, ti)
    dv, dt = head(dx)
    for got, ref, e in ((dv, dv_ref, e_dv), (dt, dt_ref, e_dt)):  # the composed bound holds for the fp32 chain, with room
        assert KB.assert_within(got, ref, e, "contrastive") < 0.5
    bad = lse.clone()
    bad[G + 17] += 1e-5
    _, dx_bad, loss_bad = infonce_standin(x, bad)
    dvb, dtb = head(dx_bad)
    assert rel(dvb, dv_ref) < 1e-4 and rel(dtb, dt_ref) < 1e-4 and abs(float(loss_bad) - loss_ref) < 2e-5 * max(1.0, abs(loss_ref))
    fails(lambda: KB.infonce_check(x, bad, None, None, what="infonce"), "infonce: lse", f"row {G + 17}")
    # (dx_bad itself stays inside its bound: that bound carries the lse bound, so the lse check is the one that sees the fault)
    KB.infonce_check(x, None, dx_bad, None, what="infonce")
    # small G and the edge values of the GPU test
    for G2 in (1, 2, 3, 5):
        x2 = torch.rand(G2, G2, generator=g) * 40.0 - 20.0
        x2[0, 0] = 21.0
        l2, d2, s2 = infonce_standin(x2)
        assert max(KB.infonce_check(x2, l2, d2, s2, what="infonce small").values()) <= 1.0


def test_ce_check_passes_fp32_and_catches_a_wrong_label_row():
    g = torch.Generator().manual_seed(15)
    for R, C in ((1, 1), (257, 4), (768, 7)):
        x = torch.randn(R, C, generator=g) * 3.0
        lab = torch.randint(0, C, (R,), generator=g, dtype=torch.int32)
        lse = torch.logsumexp(x, 1)
        onehot = torch.zeros(R, C).scatter_(1, lab.long()[:, None], 1.0)
        dl = 2.0 * (torch.exp(x - lse[:, None]) - onehot) / R
        loss = 0.25 + 2.0 * (lse - x.gather(1, lab.long()[:, None])[:, 0]).sum() / R
        assert max(KB.ce_check(x, lab, 2.0, dl, loss, loss0=0.25, what="ce").values()) <= 1.0
        if C > 1:
            bad = dl.clone()
            bad[R // 2] = 2.0 * (torch.exp(x[R // 2] - lse[R // 2]) - onehot[R // 2].roll(1)) / R
            fails(lambda: KB.ce_check(x, lab, 2.0, bad, None, what="ce"), f"row {R // 2}")
            fails(lambda: KB.ce_check(x, lab, 2.0, None, loss + 1e-3, loss0=0.25, what="ce"), "loss")


def adamw_standin(p, g, m, v, lr, wd, step, gs, beta1=0.9, beta2=0.999, eps=1e-6, m_beta=None):
    f = lambda z: torch.tensor(z, dtype=torch.float32)  # noqa: E731
    ss = f(float(f(lr)) * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step))
    gg = g * f(gs)
    m1 = f(beta1 if m_beta is None else m_beta) * m + f(1.0 - beta1) * gg
    v1 = f(beta2) * v + f(1.0 - beta2) * gg * gg
    p1 = p - ss * m1 / (v1.sqrt() + f(eps))
    if wd > 0:
        p1 = p1 - f(lr) * f(wd) * p1
    return p1, m1, v1, p1.bfloat16()


def test_adamw_check_passes_fp32_and_catches_m_updated_with_beta2():
    g = torch.Generator().manual_seed(16)
    n = 1024
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    m, v = torch.randn(n, generator=g) * 0.05, torch.rand(n, generator=g) * 1e-2
    gr[:8], m[:16], v[:16] = 0.0, 0.0, 0.0
    gr[8:16] = 1e-12
    p[16] = -1e4
    for step in (1, 2, 1000):
        for lr, wd in ((1e-2, 0.05), (1e-4, 0.0)):
            out = adamw_standin(p, gr, m, v, lr, wd, step, 0.5)
            assert KB.adamw_check(p, gr, m, v, *out, lr=lr, wd=wd, step=step, grad_scale=0.5, what="adamw") <= 1.0
            bad = adamw_standin(p, gr, m, v, lr, wd, step, 0.5, m_beta=0.999)
            fails(lambda: KB.adamw_check(p, gr, m, v, *bad, lr=lr, wd=wd, step=step, grad_scale=0.5, what="adamw"), "adamw: m")
    out = adamw_standin(p, gr, m, v, 1e-2, 0.05, 2, 0.5)
    sh = out[3].clone()
    sh[5] = sh[6]
    fails(lambda: KB.adamw_check(p, gr, m, v, out[0], out[1], out[2], sh, lr=1e-2, wd=0.05, step=2, grad_scale=0.5, what="adamw"), "bf16 shadow")


# ------------------------------------------------------------------------------------------------ GEMM edge shapes
# The smallest shapes of tests/test_gemm_edges_gpu.py: the checks those tests apply CAN fail there (every edge mistake a kernel can
# make is rejected) and a correct result cannot (the fp32 emulation passes every form's bound).
EDGE_NT = [(1, 4, 64), (129, 132, 64), (257, 264, 320)]  # (M, N, K)
EDGE_TN = [(1, 8, 8), (65, 120, 136)]                    # (M, Na, Nb)


def edge_tn_operands(M, Na, Nb, seed):
    g = torch.Generator().manual_seed(seed)
    p, q = torch.randn(M, Na, generator=g).bfloat16(), torch.randn(M, Nb, generator=g).bfloat16()
    return p, q, torch.randn(Na, Nb, generator=g), torch.randn(Na, generator=g)


def test_fp32_emulation_passes_every_forms_bound_at_the_edge_shapes():
    for (M, N, Kd) in EDGE_NT:
        a, b, bias = operands(M, N, Kd, seed=100 + M)
        g = torch.Generator().manual_seed(200 + M)
        res, h = torch.randn(M, N, generator=g), (torch.randn(M, N, generator=g) * 1.5).bfloat16()
        z = a.float() @ b.float().t()
        pre = z + bias
        check(z.bfloat16(), a, b)                                                # plain, no bias
        for dt in (torch.float32, torch.bfloat16):
            check(pre.to(dt), a, b, bias=bias)
            check((pre + res).to(dt), a, b, bias=bias, residual=res)
        check((pre + h.float()).bfloat16(), a, b, bias=bias, add_bf16=h)         # the bf16 residual stream
        for act in ("quick_gelu", "gelu"):
            y = KB.act_ref(pre.double(), act).float()
            d = KB.act_deriv_ref(pre.double(), act).float()
            check(y.bfloat16(), a, b, bias=bias, act=act, preact=pre.bfloat16())
            check(y.bfloat16(), a, b, bias=bias, act=act, preact=d.bfloat16(), deriv=True)
            check((z * KB.act_deriv_ref(h.double(), act).float()).bfloat16(), a, b, gate_h=h, gate_act=act)
            check((z * h.float()).bfloat16(), a, b, gate_h=h, gate_act=act, deriv=True)
    for (M, Na, Nb) in EDGE_TN:
        p, q, init, cs0 = edge_tn_operands(M, Na, Nb, seed=300 + M)
        out = p.float().t() @ q.float()
        check(out, p.t(), q.t(), K=M)
        check(init + out, p.t(), q.t(), residual=init, K=M)
        bound = KB.sum_bound(p.double().abs().sum(0), M, init=cs0)
        assert KB.assert_within(cs0 + p.float().sum(0), p.double().sum(0) + cs0.double(), bound, "colsum") <= 1.0


def test_edge_mistakes_are_rejected_at_every_edge_shape():
    """what a kernel gets wrong at a tile edge, applied to the correct result: the last 64-deep k stage left out, the last row
    computed from row M - 2 of a (a clamp one row short), the last four columns computed from the four before them (the N - 8
    clamp where N - 4 was meant); for TN a tail row m = M counted in with the values of row M - 1 (the clamped row not zeroed)
    and the column sum missing the last row.  Each must fail at each shape, for fp32 and bf16 results.  Two combinations do not
    exist: M = 1 has no row M - 2 and N = 4 no four columns before the last four (the kernels' clamps cannot go there either)."""
    done = set()
    for (M, N, Kd) in EDGE_NT:
        a, b, bias = operands(M, N, Kd, seed=100 + M)
        ok = a.float() @ b.float().t() + bias
        muts = {"last k stage left out": a[:, :Kd - 64].float() @ b[:, :Kd - 64].float().t() + bias}
        if M >= 2:
            x = ok.clone()
            x[-1] = a[M - 2].float() @ b.float().t() + bias
            muts["last row from row M - 2"] = x
        if N >= 8:
            x = ok.clone()
            x[:, N - 4:] = ok[:, N - 8:N - 4]
            muts["last four columns from the four before"] = x
        for name, x in muts.items():
            for dt in (torch.float32, torch.bfloat16):
                check(ok.to(dt), a, b, bias=bias)
                fails(lambda: check(x.to(dt), a, b, bias=bias), "outside the bound")
            done.add(name)
    assert len(done) == 3
    for (M, Na, Nb) in EDGE_TN:
        p, q, init, cs0 = edge_tn_operands(M, Na, Nb, seed=300 + M)
        ok = init + p.float().t() @ q.float()
        tail = ok + p[M - 1].float()[:, None] * q[M - 1].float()[None, :]
        fails(lambda: check(tail, p.t(), q.t(), residual=init, K=M), "outside the bound")
        fails(lambda: check(tail - init, p.t(), q.t(), K=M), "outside the bound")
        ref, bound = p.double().sum(0) + cs0.double(), KB.sum_bound(p.double().abs().sum(0), M, init=cs0)
        fails(lambda: KB.assert_within(cs0 + p[:M - 1].float().sum(0), ref, bound, "colsum"), "outside the bound")
        fails(lambda: KB.assert_within(cs0 + p.float().sum(0) + p[M - 1].float(), ref, bound, "colsum"), "outside the bound")  # ... or the tail row twice


# ------------------------------------------------------------------------------------------------ LayerNorm at width and row edges
import ln_cases as LC  # noqa: E402

LN_EDGE_W = (260, 1028)  # a 4-column tail behind one full column group and behind four (IT = 2, 5)


def test_layernorm_fp32_emulation_passes_the_edge_checks():
    """the checks of tests/test_layernorm_edges_gpu.py (ln_cases.fwd_case / bwd_case: ln_fwd_check, ln_bwd_check, the derived
    column bound ln_cols_check, the e4m3 references, guards, poison outside the listed rows) run on an fp32 torch emulation of
    the kernels -- two-pass mean / variance, fp32 accumulation -- with the special rows, and pass with every ratio <= 1"""
    K = LC.Emulation()
    for W in LN_EDGE_W:
        for name in ("f32_bf16", "f32_f32", "f32_q8rows", "f32_q8tensor", "bf16_4col", "cls_4col_q8rows"):
            f = LC.FWD_BY_NAME[name]
            assert LC.fwd_case(K, "cpu", f, 7, W, 4 if f["x"] == LC.F32 else 0, 0, seed=W, period=7 if f["cls"] else 0) <= 1.0
        assert LC.fwd_case(K, "cpu", LC.FWD_BY_NAME["f32_f32"], 6, W, 0, 4, seed=W, gathered=True, extra=3) <= 1.0
        assert LC.fwd_case(K, "cpu", LC.FWD_BY_NAME["f32_q8rows"], 5, W, 0, 4, seed=W, zero_beta=True) <= 1.0
        for f in LC.FORMS + [LC.FORM_F32_RES12, LC.FORM_ALL_BF16]:
            w, cols = LC.bwd_case(K, "cpu", f, 10, W, 0, 4, seed=W + 1, period=5 if f["cls"] else 0)
            assert w <= 1.0 and max(cols.values()) <= 1.0, (f["name"], w, cols)
        for M in LC.M_REDUCE[:4]:
            w, cols = LC.bwd_case(K, "cpu", LC.FORM_F32_RES12, M, 68, 0, 0, seed=M, workspace=False)
            assert w <= 1.0 and max(cols.values()) <= 1.0, (M, w, cols)


def test_layernorm_edge_mistakes_are_rejected():
    """what a kernel gets wrong at a width or row edge, built into the emulation: each is rejected by the check that is there for it,
    at both widths"""
    fwd, fwd_q, fwd_t = (LC.FWD_BY_NAME[n] for n in ("f32_bf16", "f32_q8rows", "f32_q8tensor"))
    bwd = LC.FORM_F32_RES12
    bwd_q, bwd_t = (LC.BWD_BY_NAME[f"bwd_fp8-x32-dy16-r1no-r2no-both-q8{m}"] for m in ("rows", "tensor"))
    for W in LN_EDGE_W:
        def f(form, mistake, **kw):
            return lambda: LC.fwd_case(LC.Emulation(mistake), "cpu", form, 7, W, 4, 0, seed=W, **kw)

        def b(form, mistake, **kw):
            return lambda: LC.bwd_case(LC.Emulation(mistake), "cpu", form, 7, W, 4, 0, seed=W, **kw)

        f(fwd, None)(); b(bwd, None)(); b(bwd_q, None)()                          # (the same calls without a mistake pass)
        fails(f(fwd, "var_tail"), "outside the bound", "(row 0")                   # the variance without the last four columns
        fails(f(fwd_q, "var_tail"), "outside the bound")
        fails(b(bwd, "c12_tail"), "dx", "outside the bound", "(row 0")             # c1 / c2 without them
        fails(f(fwd_q, "amax_tail"), "row scales")                                 # the amax without the tail group
        fails(f(fwd_t, "amax_tail"), "amax")
        fails(b(bwd_q, "amax_tail"), "row scales")
        fails(b(bwd_t, "amax_tail"), "amax")
        fails(b(bwd, "dgamma_tail"), "dgamma (per column)", f"(row {W - 4}, col 0)")   # dgamma missing the last block's tail
        fails(f(fwd, "row_late"), "outside the bound", "non-finite", "(row 6")     # a row's result one row late
        fails(f(fwd, "row_late", extra=2), "outside the bound", "(row 6")          # ... into a row past M (poison, not a guard)
        fails(b(bwd, "row_late"), "outside the bound", "(row 6")


# ------------------------------------------------------------------------------------------------ fused divided site kernels
import attn_fused_cases as FC  # noqa: E402


def test_fused_divided_reference_is_within_half_the_tolerance_of_autograd_at_the_tiny_geometries():
    """tests/test_attention_fused_rows_gpu.py holds the fused backward to float64 on what it read: the exact output in the patch
    rows, the bf16 output in the CLS rows (divided_mixed_o_read).  With 2 .. 4 keys per query dP - delta cancels, so that reference
    is first held to float64 autograd itself, with no kernel: at the sweep's smallest geometries, for the inputs the GPU test
    draws, every (row, head) slice of dq / dk / dv is within HALF of its ATTN_ROW_TOL entry (dv does not read delta: exact).
    The patch rows of the reference are autograd's up to the CLS query's share in dK; what is left comes from the bf16 rounding of
    the CLS output row, and seven (geometry, dh) pairs take a later draw for it (attn_fused_cases.SEED_SHIFT)."""
    worst = {}
    for mode, T, n in FC.TINY_CASES:
        for dh in (64, 80):
            S, W = 1 + T * n, FC.HEADS * dh
            qkv, dO = FC.plain_inputs(mode, T, n, dh)
            e = KB.attn_conditioning(qkv.double().view(FC.B, S, 3 * W), dO.double().view(FC.B, S, W), FC.HEADS, dh,
                                     allowed=KB.divided_allowed(mode, T, n), o_read=lambda o: KB.divided_mixed_o_read(o, o.bfloat16()))
            for nm, v in e.items():
                assert float(v.max()) <= TOL[nm] / 2, (mode, T, n, dh, nm, float(v.max()))
                worst[nm] = max(worst.get(nm, 0.0), float(v.max()))
            assert float(e["dq"].reshape(FC.B, S, FC.HEADS)[:, 1:].max()) < 1e-12   # patch queries: D from the exact output
    print("CONDITIONING fused mixed reference, tiny geometries:", {k: f"{v:.3g}" for k, v in worst.items()})
    # the first draw of one of the shifted geometries does exceed it: the shift is not decoration
    qkv, dO = FC.plain_inputs("space", 1, 1, 80, seed=FC.seed_of("space", 1, 1, 80) - 100000 * FC.SEED_SHIFT[("space", 1, 1, 80)])
    e = KB.attn_conditioning(qkv.double().view(FC.B, 2, -1), dO.double().view(FC.B, 2, -1), FC.HEADS, 80,
                             allowed=KB.divided_allowed("space", 1, 1), o_read=lambda o: KB.divided_mixed_o_read(o, o.bfloat16()))
    assert float(e["dq"].max()) > TOL["dq"], float(e["dq"].max())


def test_fused_divided_stress_inputs_have_a_finite_reference_and_the_stated_scores():
    """the second input family of the GPU sweep (attn_fused_cases.stress_inputs), no kernel: no reference slice is non-finite; in
    head 0 the CLS row puts all but 2^-24 of its weight on the one aligned key (so its group's partial dominates every other by more
    than 2^24) and some patch rows have one-key softmaxes; in head 1 lse2 = log2(keys) exactly and dq = dk = 0"""
    for mode, T, n in FC.STRESS_CASES:
        for dh in (64, 80):
            S, W = 1 + T * n, FC.HEADS * dh
            qkv, dO = FC.stress_inputs(mode, T, n, dh)
            qkv, dO = qkv.double(), dO.double()
            ro, rl = FC.forward_ref(qkv, mode, T, n, dh)
            rd = FC.backward_ref(qkv, dO, ro, ro.bfloat16(), rl, mode, T, n, dh)
            assert torch.isfinite(ro).all() and torch.isfinite(rl).all() and torch.isfinite(rd).all(), (mode, T, n, dh)
            P = KB.divided_fwd_ref(qkv.view(FC.B, S, 3 * W), FC.HEADS, dh, mode, T, n)[2]
            for b in range(FC.B):
                r = FC.stress_row(mode, T, n, b)
                assert r >= 1 and float(1.0 - P[b, 0, 0, r]) < 2.0 ** -24, (mode, T, n, dh, b, float(P[b, 0, 0, r]))
            assert int((P[:, 0, 1:].max(-1).values > 1 - 2.0 ** -9).sum()) >= 4, (mode, T, n, dh)
            keys = KB.divided_allowed(mode, T, n).sum(1).double()
            assert float((rl.view(FC.B, S, FC.HEADS)[:, :, 1] - torch.log2(keys)).abs().max()) < 1e-13, (mode, T, n, dh)
            z = rd.view(FC.B * S, 3, FC.HEADS, dh)
            assert (z[:, :2, 1] == 0).all() and (z[:, 2, 1] != 0).any()


def _site_refs(mode, T, n, dh):
    qkv, dO = FC.plain_inputs(mode, T, n, dh)
    qkv, dO = qkv.double(), dO.double()
    ro, rl = FC.forward_ref(qkv, mode, T, n, dh)
    return qkv, dO, ro, rl, FC.backward_ref(qkv, dO, ro, ro.bfloat16(), rl, mode, T, n, dh)


def _with_extra_keys(qkv, dO, mode, T, n, dh, edit=None):
    """(out, lse2, dqkv) of the site in float64 autograd with one edit (clip, query row, key rows, seen) of the key relation; key
    S is a padding row (q = k = v = 0: a key at score 0 with a zero value) that no query sees unless the edit says so"""
    S, W = 1 + T * n, FC.HEADS * dh
    pad = lambda t: torch.cat([t.view(FC.B, S, -1), torch.zeros(FC.B, 1, t.shape[-1], dtype=t.dtype)], 1)  # noqa: E731
    al = torch.zeros(FC.B, 1, S + 1, S + 1, dtype=torch.bool)
    al[:, 0, :S, :S] = KB.divided_allowed(mode, T, n)
    al[:, 0, S, S] = True
    if edit is not None:
        b, query, keys, seen = edit
        al[b, 0, query, keys] = seen
    out, dqkv = KB.attn_autograd(pad(qkv), pad(dO), FC.HEADS, dh, allowed=al)
    lse2 = KB.attn_fwd_ref(pad(qkv), FC.HEADS, dh, allowed=al)[1]
    return out[:, :S].reshape(FC.B * S, W), lse2[:, :S].reshape(FC.B * S, FC.HEADS), dqkv[:, :S].reshape(FC.B * S, 3 * W)


def test_fused_divided_gates_catch_single_faults_of_the_fused_kernels():
    """The gates of tests/test_attention_fused_rows_gpu.py (attn_fused_cases.gate_forward / gate_backward) on float64 results with
    ONE fault of the kind the fused kernels can make, SPACE (n = 16, T = 3: one live row in the last tile) and TIME (T = 19, n = 29:
    the <2, 20> tile, a one-position last chunk): each raises, and names the quantity.  The whole-tensor rel of
    test_attention_site_forward / _backward (8e-3 / 2e-2) is computed for the same fault alone."""
    dh = 64
    W = FC.HEADS * dh
    for mode, T, n in (("space", 3, 16), ("time", 19, 29)):
        S = 1 + T * n
        qkv, dO, ro, rl, rd = _site_refs(mode, T, n, dh)
        tag = f"fault[{mode}]"

        def gates(out=ro, lse=rl, dqkv=rd):
            FC.gate_forward(tag, out, lse, ro, rl, S)
            FC.gate_backward(tag, dqkv, rd, S)

        def old(out=ro, dqkv=rd):
            """the old gates' whole-tensor figures"""
            return {"out": rel(out, ro), **{nm: rel(a, b) for (nm, a), b in zip(_thirds(dqkv, W).items(), _thirds(rd, W).values())}}

        gates()                                                                 # the clean result passes
        clean = _with_extra_keys(qkv, dO, mode, T, n, dh)
        assert rel(clean[0], ro) < 1e-13 and rel(clean[1], rl) < 1e-13
        if mode == "space":   # frame 1 of clip 1; its last row is the single live row of the second tile
            b, last, nb = 1, 1 + 1 * n + (n - 1), n          # neighbouring group: the same row of the next frame
            block = torch.arange(1 + n, 1 + 2 * n)           # the queries of that frame's block
            left_out = block                                 # the keys of one frame's CLS partial
        else:                 # patch position 28 of clip 0 (the one-position last chunk); its last row is row 19 of a 20-row tile
            b, last, nb = 0, 1 + (T - 1) * n + 28, -1        # neighbouring group: the same frame of position 27
            block = 1 + torch.arange(T) * n + 28             # the queries of chunk 1's block
            p = torch.arange(2, 28, 4)                       # the positions of wave 2 of chunk 0
            left_out = (1 + torch.arange(T)[:, None] * n + p[None, :]).reshape(-1)
        r = b * S + last
        seen = {}
        # ---- (a) the last live row of the group's last tile also sees ONE padding key at score 0
        bad = _with_extra_keys(qkv, dO, mode, T, n, dh, (b, last, S, True))
        out_a, lse_a, dq_a = ro + (bad[0] - clean[0]), rl + (bad[1] - clean[1]), rd + (bad[2] - clean[2])
        assert int(((out_a - ro).abs().sum(1) > 0).sum()) == 1               # one row of out; dK / dV of the group's keys follow
        fails(lambda: gates(out=out_a), " out", f"[{r}, ")
        fails(lambda: gates(lse=lse_a), "lse2", f"(row {r},")
        fails(lambda: gates(dqkv=dq_a), " dq", f"[{r}, ")
        seen["a"] = old(out_a, dq_a)
        # ---- (b) the CLS output merged without one frame's (SPACE) / one wave's (TIME) partial
        bad = _with_extra_keys(qkv, dO, mode, T, n, dh, (b, 0, left_out, False))
        out_b, lse_b = ro.clone(), rl.clone()
        out_b[b * S], lse_b[b * S] = bad[0][b * S], bad[1][b * S]
        fails(lambda: gates(out=out_b), " out", f"[{b * S}, ")
        fails(lambda: gates(lse=lse_b), "lse2", f"(row {b * S},")
        seen["b"] = old(out_b)
        # ---- (c) one patch row's result taken from the same row of the neighbouring group
        out_c, lse_c, dq_c = ro.clone(), rl.clone(), rd.clone()
        out_c[r], lse_c[r], dq_c[r] = ro[r + nb], rl[r + nb], rd[r + nb]
        fails(lambda: gates(out=out_c), " out", f"[{r}, ")
        fails(lambda: gates(lse=lse_c), "lse2", f"(row {r},")
        fails(lambda: gates(dqkv=dq_c), " dq", f"[{r}, ")
        seen["c"] = old(out_c, dq_c)
        # ---- (d) dK of the CLS row without one block's share
        qr = torch.zeros(FC.B, S, dtype=torch.bool)
        qr[b, block] = True
        share = KB.attn_bwd_same_inputs(qkv.view(FC.B, S, 3 * W), dO.view(FC.B, S, W), ro.view(FC.B, S, W), rl.view(FC.B, S, FC.HEADS),
                                        FC.HEADS, dh, allowed=KB.divided_allowed(mode, T, n), q_rows=qr)[b, 0, W:2 * W]
        dq_d = rd.clone()
        dq_d[b * S, W:2 * W] -= share
        fails(lambda: gates(dqkv=dq_d), " dk", f"[{b * S}, ")
        seen["d"] = old(dqkv=dq_d)
        for k, v in seen.items():
            print(f"FAULT {mode} ({k}) whole-tensor rel:", {q: f"{x:.3g}" for q, x in v.items()})
        # the whole-tensor gates of test_attention_site_forward / _backward with that fault alone.  Under them, i.e. invisible so far:
        # the padding key in both modes (SPACE 4.4e-3 out, 4.4e-3 .. 4.7e-3 dq / dk / dv; TIME 9.7e-4, 1.0e-3 .. 1.2e-3) and the
        # dropped wave partial of TIME (3.1e-3).  NOT under them at these sizes (B = 2, 98 / 1 104 rows), so not asserted: a whole
        # frame's partial dropped from the SPACE CLS row (5.3e-2 of out), a row taken from the neighbouring group (SPACE 0.13 .. 0.14,
        # TIME 3.6e-2 .. 4.5e-2: one wholly wrong row of so few is seen by a norm over all of them), the CLS dK short of a block
        # (SPACE 0.10: a third of its queries; TIME 2.02e-2 against the 2e-2 gate).  So the premise this test set out with -- such
        # single faults are invisible to the whole-tensor gates -- holds for 3 of the 8 at these sizes and NOT for most single-row
        # faults: with 98 or 1 104 rows a wholly wrong row is 4e-2 .. 0.14 of the norm.  What the old gates cannot do at any size is
        # name the row, and they miss the same faults once the batch is a few hundred times larger (the per-row gates do not dilute).
        for k in {"space": ("b", "c", "d"), "time": ("c", "d")}[mode]:   # recorded, so that a change of these figures is noticed
            assert seen[k]["out"] >= 8e-3 or max(seen[k][q] for q in ("dq", "dk", "dv")) >= 2e-2, (mode, k, seen[k])
        for k in {"space": ("a",), "time": ("a", "b")}[mode]:
            assert seen[k]["out"] < 8e-3 and max(seen[k][q] for q in ("dq", "dk", "dv")) < 2e-2, (mode, k, seen[k])
