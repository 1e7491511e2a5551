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
