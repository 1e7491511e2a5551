"""Shared cases of the LayerNorm tests (a plain helper module, imported by the tests; nothing here touches a GPU at import): the
width and row-count lists derived from the kernels' own constants, operands inside NaN-poisoned buffers with the rows a
LayerNorm kernel can get wrong, the legal template forms read off the dispatch of tvts_amd/csrc/norm.hip, the checks one forward or
backward case runs, and one table of valid baseline calls with the single-argument changes every entry point must refuse.

tests/test_layernorm_edges_gpu.py runs fwd_case / bwd_case over the lists and launches every baseline of BASELINES once;
tests/test_layernorm_args_cpu.py calls every refusal of REFUSALS without a GPU; tests/test_kernel_bounds_cpu.py shows on the CPU
that the checks used here pass an fp32 emulation of the kernels and reject what a kernel gets wrong at a width or row edge."""
import torch

import kernel_bounds as KB
from gemm_cases import BF16, F32, I32, U8, Mat

# ------------------------------------------------------------------------------------------------ the kernels' constants
COLS4 = 64 * 4          # columns one trip of the 4-column kernels covers (ln_fwd_kernel<LnCols4<TX>, ...>, ln_bwd_kernel: G = IT = ceil(W / 256) trips)
COLS8 = 64 * 8          # ... of the 8-column bf16-row forward (ln_fwd_kernel<LnCols8, ...>: G = ceil(W / 512))
MAX_W = COLS4 * 5       # LN_MAX_IT
WAVES = 4               # rows a block holds at a time
FWD_BLOCKS = 2048       # cap of the forward grids: past 8192 rows a wave walks to a second row
BWD_BLOCKS = {2: 512, 3: 768, 4: 1024}  # 256 * ln_bwd_per_cu: 2048 / 3072 / 4096 rows per trip
REDUCE_COLS, REDUCE_PARTS, REDUCE_UNROLL = 64, 16, 8  # ln_dgamma_reduce_kernel: 64 columns x 16 row groups, 8 loads in flight

# 4-column kernels: the first column group partly filled, exact, one group past, then every IT with a 4-column tail / one group short
W_4COL = [4, COLS4 - 4, COLS4, COLS4 + 4, 2 * COLS4 + 4, 3 * COLS4 - 4, 4 * COLS4 - 4, 4 * COLS4 + 4, MAX_W - 4, MAX_W]
assert W_4COL == [4, 252, 256, 260, 516, 764, 1020, 1028, 1276, 1280]
# 8-column kernel (bf16 x, W % 8 == 0, every leading dimension % 8 == 0): the same around NP = 1, 2, 3
W_8COL = [8, COLS8 - 8, COLS8, COLS8 + 8, 2 * COLS8 - 8, 2 * COLS8, 2 * COLS8 + 8, MAX_W]
assert W_8COL == [8, 504, 512, 520, 1016, 1024, 1032, 1280]
# bf16 x that ln8_ok rejects -> the 4-column bf16 kernels: (W, ld % 8 of x, ld % 8 of y).  W % 8 == 4 with any pitch, and W = 512
# with a pitch of x or of y that is 4 past a multiple of 8
W_BF16_4COL = [(12, 4, 4), (COLS4 + 4, 0, 0), (2 * COLS4 + 4, 4, 0), (4 * COLS4 + 4, 0, 4), (COLS8, 4, 0), (COLS8, 0, 4)]

M_SMALL = [1, 3, 4, 5, 7]            # one block; waves without a row; a second block of one row / three rows
M_WRAP_FWD = [WAVES * FWD_BLOCKS + 5, 2 * WAVES * FWD_BLOCKS + 1]  # 8197: some waves get two rows, some one; 16385: one a third
M_WRAP_BWD = [WAVES * BWD_BLOCKS[4] + 5, 2 * WAVES * BWD_BLOCKS[4] + 5]  # 4101: >= two rows for some wave of every variant; 8197
assert M_WRAP_FWD == [8197, 16385] and M_WRAP_BWD == [4101, 8197]
# block counts of the backward (= partials the reduce kernel sums per column): none, under / at / over one row group each, the
# unrolled loop's boundary b + 7 * 16 < nblocks (112 / 113), one unrolled trip with every remainder, two trips
_P, _U = REDUCE_PARTS, REDUCE_UNROLL
REDUCE_NBLOCKS = [1, _P - 1, _P, _P + 1, (_U - 1) * _P, (_U - 1) * _P + 1, (_U - 1) * _P + 8, _U * _P, _U * _P + 1, 2 * _U * _P - _P + 1]
assert REDUCE_NBLOCKS == [1, 15, 16, 17, 112, 113, 120, 128, 129, 241]
M_REDUCE = [WAVES * n - (n % 3) for n in REDUCE_NBLOCKS]  # (a ragged last block for two of three)
assert [-(-m // WAVES) for m in M_REDUCE] == REDUCE_NBLOCKS
W_REDUCE = [4, REDUCE_COLS + 4, 4 * REDUCE_COLS + 4]  # c < W cuts the first, the second, the fifth 64-column block


def ln8_ok(W, lda, ldb):
    """the host's choice of the 8-column bf16-row forward (ln_cols8 of norm.hip)"""
    return W % 8 == 0 and W <= 1536 and lda % 8 == 0 and ldb % 8 == 0


# ------------------------------------------------------------------------------------------------ operands
def put(t, ldmod=0, rows=3):
    """a copy of the [M, W] tensor t as a view at column 8 (16 for uint8: 16 bytes or more from the allocation, a multiple of 16
    bytes) of a NaN buffer (0x7F, the e4m3 NaN, for uint8) with `rows` more rows and a leading dimension != W with ld % 8 == ldmod"""
    M, W = t.shape
    left = 16 if t.dtype == U8 else 8
    right = 8 + (ldmod - W) % 8
    if t.dtype.is_floating_point:
        buf = torch.full((M + rows, left + W + right), float("nan"), dtype=t.dtype, device=t.device)
    else:
        buf = torch.full((M + rows, left + W + right), 0x7F, dtype=t.dtype, device=t.device)
    v = buf[:M, left:left + W]
    v.copy_(t)
    assert v.stride(0) % 8 == ldmod and v.stride(0) > W and (v.data_ptr() - buf.data_ptr()) % 16 == 0
    return v


def put_vec(t):
    """a [W] vector 32 bytes into a NaN buffer with 8 more elements behind it"""
    buf = torch.full((t.numel() + 16,), float("nan"), dtype=t.dtype, device=t.device)
    v = buf[8:8 + t.numel()]
    v.copy_(t)
    return v


def out_mat(M, W, dtype, device, ldmod=0):
    """KB.guarded with guard columns chosen so that ld % 8 == ldmod -> (buffer, view)"""
    return KB.guarded(M, W, dtype, device, cols=8 + (ldmod - W) % 8)


def out_vec(M, device):
    """mean / rstd / row_scale: NaN-filled, 8 elements longer than the rows"""
    return torch.full((M + 8,), float("nan"), device=device)


ZERO, CONST, OFFSET, LAST = 1, 2, 3, 0  # the special rows, where M has room for them (LAST first: every M >= 1 has it)


def special_rows(M, W, seed, device, scale=1.0, last=-8.0):
    """fp32 [M, W]: unit normal rows scaled over logspace(-4, 1), then (as far as M has rows)
    row 0: unit spread, and the row's largest magnitude, negative, in its LAST column (inside the tail column group of a partly
           filled width: an amax or a variance that skips the tail misses it);
    row 1: all zero;  row 2: a constant non-zero row;  row 3: mean 1e3, unit spread.
    last: that last-column value (the backward's dy takes one that makes dx[0, W - 1] the largest |dx| of the whole tensor, which
    the per-tensor amax must see: the rows with a small spread of x have rstd up to 316 and |dx| up to ~1e4)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, W, generator=g)
    if M > 4:
        s = torch.ones(M)
        s[4:] = torch.logspace(-4, 1, M - 4)[torch.randperm(M - 4, generator=g)]
        x = x * s[:, None]
    x[LAST, W - 1] = last
    if M > ZERO:
        x[ZERO] = 0.0
    if M > CONST:
        x[CONST] = 0.75
    if M > OFFSET:
        x[OFFSET] += 1e3
    return (x * scale).to(device)


def affine(W, seed, device):
    """gamma, beta (poisoned views); the last column's gamma is the largest, so that the largest |xhat| stays the largest |y|"""
    g = torch.Generator().manual_seed(seed)
    gamma, beta = 1 + 0.1 * torch.randn(W, generator=g), 0.1 * torch.randn(W, generator=g)
    gamma[W - 1], beta[W - 1] = 1.5, -0.1
    return put_vec(gamma.to(device)), put_vec(beta.to(device))


def gather_list(R, Mx, seed, device):
    """R distinct rows of Mx in a permuted, non-monotonic order that holds row 0 and the last row (int32)"""
    assert 2 <= R <= Mx
    g = torch.Generator().manual_seed(seed)
    mid = (torch.randperm(Mx - 2, generator=g)[:R - 2] + 1).tolist()
    rows = [Mx - 1] + mid[:len(mid) // 2] + [0] + mid[len(mid) // 2:]
    if R > 3:
        assert any(a > b for a, b in zip(rows, rows[1:])) and any(a < b for a, b in zip(rows, rows[1:]))
    return torch.tensor(rows, dtype=I32, device=device)


# ------------------------------------------------------------------------------------------------ e4m3 copies
def e4m3_bits(v, inv):
    """uint8 bits of torch.float8_e4m3fn of the clamped v * inv (fp32 product, as the kernels form it)"""
    return (v.float() * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(U8)


def q8_rows_check(out16, q, rs, what, K=None):
    """per-row scales: row_scale = amax(bf16 output) / 448 within rtol 1e-6 (1.0 for an all-zero row), the bytes those of
    out * (1 / row_scale) with the scale the kernel wrote, and (K given) both bit for bit what quantize_fp8_rows makes of out16"""
    M = out16.shape[0]
    am = out16.float().abs().amax(1)
    want = torch.where(am > 0, am / 448.0, torch.ones_like(am))
    assert torch.allclose(rs[:M], want, rtol=1e-6, atol=0), f"{what}: row scales"
    KB.assert_equal_bits(q, e4m3_bits(out16, (1.0 / rs[:M])[:, None]), f"{what}: e4m3 bytes under the written scales")
    zero = am == 0
    assert bool((q[zero] == 0).all()) and bool((rs[:M][zero] == 1.0).all()), f"{what}: an all-zero row has scale 1 and zero bytes"
    if K is not None:
        # (the quantiser takes contiguous rows of whole 8-column groups: a copy, padded with zero columns that change no amax)
        W = out16.shape[1]
        pad = torch.zeros(M, (W + 7) // 8 * 8, dtype=BF16, device=out16.device)
        pad[:, :W] = out16
        q_ref, rs_ref = K.quantize_fp8_rows(pad)
        assert bool((q_ref[:, W:] == 0).all())
        KB.assert_equal_bits(q.contiguous(), q_ref[:, :W].contiguous(), f"{what}: e4m3 bytes against quantize_fp8_rows")
        KB.assert_equal_bits(rs[:M].contiguous(), rs_ref[:M].contiguous(), f"{what}: row scales against quantize_fp8_rows")


def q8_tensor_check(out16, q, ts, what):
    """one scale for the tensor: the bytes are torch e4m3 of the clamped out / tscale (tscale <= 0 behaves as 1.0)"""
    s = ts.float().reshape(())
    s = torch.where(s > 0, s, torch.ones_like(s))
    KB.assert_equal_bits(q, e4m3_bits(out16, 1.0 / s), f"{what}: e4m3 bytes under the tensor scale")


def tensor_scale_runs(amax_about):
    """(tscale, initial amax) of the per-tensor runs: a scale under which the largest values saturate, amax from 0 (afterwards the
    output's exact maximum); amax starting above the maximum (kept); tscale = 0 (behaves as 1.0)"""
    return [(amax_about / 448.0 / 4.0, 0.0), (amax_about / 448.0, 2.0 * amax_about + 1.0), (0.0, 0.0)]


# ------------------------------------------------------------------------------------------------ forms
# Forward.  kernel: what the host's dispatch launches for the form (asserted through ln8_ok on the case's own leading dimensions);
# widths: the list the form runs over.  q8: None, "rows" (one scale per row) or "tensor"; y=False: the e4m3 bytes are the only output.
def _f(name, kernel, x, y, widths, q8=None, cls=False, has_y=True):
    return dict(name=name, kernel=kernel, x=x, y=y, widths=widths, q8=q8, cls=cls, has_y=has_y)


FWD_FORMS = [
    _f("f32_bf16", "ln_fwd_kernel<LnCols4<float>, bf16, G>", F32, BF16, "W_4COL"),
    _f("f32_f32", "ln_fwd_kernel<LnCols4<float>, float, G>", F32, F32, "W_4COL"),
    _f("bf16_8col", "ln_fwd_kernel<LnCols8, bf16, G>", BF16, BF16, "W_8COL"),
    _f("bf16_4col", "ln_fwd_kernel<LnCols4<bf16>, bf16, G>", BF16, BF16, "W_BF16_4COL"),
    _f("f32_q8rows", "ln_fwd_kernel<LnCols4<float>, bf16, G, Q8>", F32, BF16, "W_4COL", q8="rows"),
    _f("f32_q8tensor", "ln_fwd_kernel<LnCols4<float>, bf16, G, Q8>", F32, BF16, "W_4COL", q8="tensor"),
    _f("bf16_8col_q8rows", "ln_fwd_kernel<LnCols8, bf16, G, Q8>", BF16, BF16, "W_8COL", q8="rows"),
    _f("bf16_8col_q8tensor", "ln_fwd_kernel<LnCols8, bf16, G, Q8>", BF16, BF16, "W_8COL", q8="tensor"),
    _f("bf16_8col_q8only_rows", "ln_fwd_kernel<LnCols8, bf16, G, Q8>, y = NULL", BF16, BF16, "W_8COL", q8="rows", has_y=False),
    _f("bf16_8col_q8only_tensor", "ln_fwd_kernel<LnCols8, bf16, G, Q8>, y = NULL", BF16, BF16, "W_8COL", q8="tensor", has_y=False),
    _f("bf16_4col_q8rows", "ln_fwd_kernel<LnCols4<bf16>, bf16, G, Q8>", BF16, BF16, "W_BF16_4COL", q8="rows"),
    _f("bf16_4col_q8tensor", "ln_fwd_kernel<LnCols4<bf16>, bf16, G, Q8>", BF16, BF16, "W_BF16_4COL", q8="tensor"),
    _f("cls_8col", "ln_fwd_kernel<LnCols8, bf16, G, false, CLS>", BF16, BF16, "W_8COL", cls=True),
    _f("cls_4col", "ln_fwd_kernel<LnCols4<bf16>, bf16, G, false, CLS>", BF16, BF16, "W_BF16_4COL", cls=True),
    _f("cls_8col_q8rows", "ln_fwd_kernel<LnCols8, bf16, G, Q8, CLS>", BF16, BF16, "W_8COL", q8="rows", cls=True),
    _f("cls_4col_q8rows", "ln_fwd_kernel<LnCols4<bf16>, bf16, G, Q8, CLS>", BF16, BF16, "W_BF16_4COL", q8="rows", cls=True),
]
FWD_BY_NAME = {f["name"]: f for f in FWD_FORMS}


def fwd_widths(form):
    """(W, ld % 8 of x, ld % 8 of y and q8) of a forward form"""
    if form["widths"] == "W_4COL":
        return [(W, (W + 4 * i) % 8, (W + 4 * (i // 2)) % 8) for i, W in enumerate(W_4COL)]  # both flavours of both pitches
    if form["widths"] == "W_8COL":
        return [(W, 0, 0) for W in W_8COL]
    return list(W_BF16_4COL)


# Backward: the instantiations ln_bwd_kernel<TDY, IT, R1, R2, TX, Q8, TR1, CLS> the three entry points reach.
def _b(entry, x, dy, res1, res2, outs, q8=None, rows=False, cls=False):
    n = f"{entry}-x{'16' if x == BF16 else '32'}-dy{'16' if dy == BF16 else '32'}-r1{ {None: 'no', F32: '32', BF16: '16'}[res1] }-r2{'16' if res2 else 'no'}-{outs}"
    n += (f"-q8{q8}" if q8 else "") + ("-rows" if rows else "")
    return dict(name=n, entry=entry, x=x, dy=dy, res1=res1, res2=res2, outs=outs, q8=q8, rows=rows, cls=cls)


FORMS = []
_outs = ["both", "dx", "dxb"]
# tvts_layernorm_bwd: bf16 x takes bf16 dy and no or a bf16 res1; fp32 x with a bf16 res1 takes bf16 dy; fp32 x otherwise fp32 or
# bf16 dy with no or an fp32 res1; res2 (bf16) with each.  dx / dx_bf16 / both are run-time arguments: rotated over the forms
for x, dy, res1 in [(BF16, BF16, None), (BF16, BF16, BF16), (F32, BF16, BF16), (F32, F32, None), (F32, F32, F32), (F32, BF16, None), (F32, BF16, F32)]:
    for res2 in (False, True):
        FORMS.append(_b("bwd", x, dy, res1, res2, _outs[len(FORMS) % 3]))
FORMS += [_b("bwd", F32, F32, F32, True, "both", rows=True), _b("bwd", BF16, BF16, BF16, False, "dxb", rows=True),
          _b("bwd", F32, BF16, None, False, "dx", rows=True)]
# tvts_layernorm_bwd_fp8: bf16 dy, every row, dx_bf16 required, res2 only with res1
for q8 in ("rows", "tensor"):
    for x, res1, res2 in [(BF16, None, False), (BF16, BF16, False), (BF16, BF16, True), (F32, BF16, False), (F32, BF16, True),
                          (F32, None, False), (F32, F32, False), (F32, F32, True)]:
        FORMS.append(_b("bwd_fp8", x, BF16, res1, res2, "both" if x == F32 else "dxb", q8=q8))
# tvts_layernorm_bwd_cls: all bf16, the plain launch and the CLS launch behind it
for q8 in (None, "rows", "tensor"):
    for res1, res2 in [(None, False), (BF16, False), (BF16, True)]:
        FORMS.append(_b("bwd_cls", BF16, BF16, res1, res2, "dxb", q8=q8, cls=True))
BWD_BY_NAME = {f["name"]: f for f in FORMS}
assert len(BWD_BY_NAME) == len(FORMS)
# the two forms that run over every width of W_4COL
FORM_F32_RES12 = _b("bwd", F32, F32, F32, True, "both")
FORM_ALL_BF16 = _b("bwd", BF16, BF16, BF16, False, "both")


# ------------------------------------------------------------------------------------------------ one forward case
def fwd_case(K, dev, form, M, W, ldx=0, ldy=0, *, seed=0, period=0, gathered=False, extra=0, refresh=True, zero_beta=False, eps=1e-5):
    """One forward launch of `form` on M rows of width W and every check of it -> worst |err| / bound.
    ldx / ldy: ld % 8 of the input and of the outputs (y and q8).  gathered: the rows come through a permuted list out of M + 5.
    extra: the buffers hold M + extra rows and the kernel is told M: the rows past M keep their poison.  period: the hybrid
    stream (form['cls']): rows r % period == 0 are read from the fp32 side array, their stream rows are stale sentinels.
    zero_beta: beta = 0, so that the all-zero row of x gives an all-zero row of y: its e4m3 copy has scale 1.0 and zero bytes
    (q8_rows_check; with a beta the row equals beta, which every case asserts)."""
    what = f"ln fwd {form['name']} [{M},{W}] ld {ldx}/{ldy}"
    Mt = M + extra
    Mx = Mt + 5 if gathered else Mt
    x_true = special_rows(Mx, W, seed, dev)
    gamma, beta = affine(W, seed + 1, dev)
    if zero_beta:
        beta.zero_()
    rows = gather_list(Mt, Mx, seed + 2, dev) if gathered else None
    xin = put(x_true.to(form["x"]), ldx)
    seen = xin.float()
    kw = {}
    if form["cls"]:
        assert period and M % period == 0 and not gathered and not extra
        cls_rows = torch.arange(0, M, period, device=dev)
        cls_x = x_true[cls_rows].contiguous()
        xin[cls_rows] = 777.0
        seen = xin.float()
        seen[cls_rows] = cls_x
        kw = dict(cls_x=cls_x, cls_period=period, refresh=refresh)
        before = xin.clone()
    if rows is not None:
        seen = seen[rows.long()]
        kw["rows"] = rows
    if extra or gathered:
        kw["M"] = M
    # the kernel the case is written for
    expect8 = form["x"] == BF16 and ln8_ok(W, xin.stride(0), ldy)  # (y and q8 share the flavour ldy of their pitch)
    assert expect8 == ("LnCols8" in form["kernel"]), (what, "reaches the 8-column kernel" if expect8 else "reaches the 4-column kernel")
    ybuf, y = out_mat(Mt, W, form["y"], dev, ldy)
    mean, rstd = out_vec(Mt, dev), out_vec(Mt, dev)
    q8 = form["q8"]
    runs = [(None, None)]
    if q8:
        qbuf, q = out_mat(Mt, W, U8, dev, ldy)
        kw["q8"] = q
        if q8 == "tensor":  # the output's maximum first, from a per-row run of the same form
            y0 = torch.empty(Mt, W, dtype=BF16, device=dev)
            kx = {k: v for k, v in kw.items() if k != "q8"}
            if form["cls"]:
                kx["refresh"] = False
            K.layernorm_fwd(xin, gamma, beta, eps, y0, q8=torch.empty(Mt, W, dtype=U8, device=dev), row_scale=out_vec(Mt, dev), **kx)
            runs = tensor_scale_runs(float(y0[:M].float().abs().max()))
    worst = 0.0
    for ts, am0 in runs:
        ybuf.fill_(float("nan")); mean.fill_(float("nan")); rstd.fill_(float("nan"))
        if q8:
            qbuf.fill_(0xFF)
        if q8 == "rows":
            kw["row_scale"] = out_vec(Mt, dev)
        elif q8 == "tensor":
            kw["tscale"], kw["amax"] = torch.tensor([ts], device=dev), torch.tensor([am0], device=dev)
        K.layernorm_fwd(xin, gamma, beta, eps, y if form["has_y"] else None, mean, rstd, **kw)
        if not form["has_y"]:  # the bf16 values the bytes were made of: a launch of the same kernel that also stores them
            kx = dict(kw, q8=torch.empty(Mt, W, dtype=U8, device=dev))
            if q8 == "tensor":
                kx["amax"] = torch.zeros(1, device=dev)
            K.layernorm_fwd(xin, gamma, beta, eps, y, **kx)
        worst = max(worst, KB.ln_fwd_check(seen[:M], gamma, beta, eps, y[:M], mean[:M], rstd[:M], what=what))
        KB.check_guards(ybuf, Mt, W, what)
        for name, t in (("y", y), ("mean", mean), ("rstd", rstd)) + ((("row_scale", kw["row_scale"]),) if q8 == "rows" else ()):
            assert bool(torch.isnan(t[M:]).all()), f"{what}: {name} written past row {M}"
        if M > ZERO and not gathered:
            KB.assert_equal_bits(y[ZERO], beta.to(form["y"]), f"{what}: the all-zero row is beta")
        if q8:
            KB.check_guards(qbuf, Mt, W, what + " q8")
            assert bool((q[M:] == 0xFF).all()), f"{what}: q8 written past row {M}"
            if q8 == "rows":
                q8_rows_check(y[:M], q[:M], kw["row_scale"], what, K)
                if zero_beta and M > ZERO and not gathered:
                    assert float(kw["row_scale"][ZERO]) == 1.0 and int(q[ZERO].max()) == 0, f"{what}: the all-zero row"
            else:
                q8_tensor_check(y[:M], q[:M], kw["tscale"], what)
                am1 = max(am0, float(y[:M].float().abs().max()))  # exact: the maximum of the bf16 values, or the larger start
                assert float(kw["amax"]) == am1, (what, "amax", float(kw["amax"]), am1, ts, am0)
                if ts > 0 and am0 == 0.0:
                    assert int((q[:M] & 0x7F).max()) == 0x7E, f"{what}: nothing saturated under tscale {ts}"
        if form["cls"]:
            rounded = before.clone()
            if refresh:
                rounded[cls_rows] = cls_x.bfloat16()
            KB.assert_equal_bits(xin.contiguous(), rounded.contiguous(), f"{what}: the stream after the launch (refresh={refresh})")
            # rows that are no CLS row: the bits of the plain bf16-row kernel the same pitches reach (with the same e4m3 copy)
            other = torch.ones(M, dtype=torch.bool, device=dev); other[cls_rows] = False
            if bool(other.any()):
                _, y0 = out_mat(Mt, W, form["y"], dev, ldy)
                kx = {k: v for k, v in kw.items() if k not in ("cls_x", "cls_period", "refresh")}
                if q8:
                    kx.update(q8=out_mat(Mt, W, U8, dev, ldy)[1], row_scale=out_vec(Mt, dev))
                K.layernorm_fwd(xin, gamma, beta, eps, y0, **kx)
                KB.assert_equal_bits(y[other], y0[other], f"{what}: rows that are no CLS row against the plain kernel")
    return worst


# ------------------------------------------------------------------------------------------------ one backward case
def _fwd_stats(K, xin, gamma, beta, eps, M, rows, dev, cls_kw):
    mean, rstd = out_vec(M, dev), out_vec(M, dev)
    y = torch.empty(M, xin.shape[1], dtype=BF16 if xin.dtype == BF16 else F32, device=dev)
    kw = dict(cls_kw)
    if rows is not None:
        kw.update(rows=rows, M=M)
    K.layernorm_fwd(xin, gamma, beta, eps, y, mean, rstd, **kw)
    return mean, rstd


def bwd_case(K, dev, form, M, W, ldin=0, ldout=0, *, seed=0, period=0, workspace=True, extra=0, eps=1e-5):
    """One backward launch of `form` and every check of it -> (worst |err| / bound of dx, {dgamma, dbeta: worst column ratio}).
    form['rows']: the rows come through a permuted list out of M + 5 and the results are scattered into poisoned buffers.
    extra: as fwd_case.  period: the hybrid stream (form['cls'])."""
    what = f"ln {form['name']} [{M},{W}] ld {ldin}/{ldout}" + ("" if workspace else " atomics")
    Mt = M + extra
    Mx = Mt + 5 if form["rows"] else Mt
    rows = gather_list(Mt, Mx, seed + 2, dev) if form["rows"] else None
    rl = rows.long()[:M] if rows is not None else torch.arange(M, device=dev)
    x_true = special_rows(Mx, W, seed, dev)
    gamma, beta = affine(W, seed + 1, dev)
    xin = put(x_true.to(form["x"]), ldin)
    seen = xin.float()
    cls_kw, cls = {}, form["cls"]
    if cls:
        assert period and M % period == 0 and not extra
        cls_rows = torch.arange(0, M, period, device=dev)
        other = torch.ones(M, dtype=torch.bool, device=dev); other[cls_rows] = False
        cls_x = x_true[cls_rows].contiguous()
        xin[cls_rows] = 777.0
        truth = xin.float(); truth[cls_rows] = cls_x
        cls_kw = dict(cls_x=cls_x, cls_period=period)
    mean, rstd = _fwd_stats(K, xin, gamma, beta, eps, Mt, rows, dev, cls_kw)  # (refreshes the stream's CLS rows)
    seen = xin.float()  # what the plain launch reads
    dy_true = special_rows(Mt, W, seed + 3, dev, last=-2e5)  # row 1 all zero: without residuals dx is zero there
    dy = put(dy_true.to(form["dy"]), ldin)
    res1 = res2 = cls_res1 = None
    if form["res1"] is not None:
        r1_true = special_rows(Mx, W, seed + 4, dev, scale=0.5)
        res1 = put(r1_true.to(form["res1"]), ldin)
        if cls:
            cls_res1 = r1_true[cls_rows].contiguous()
            res1[cls_rows] = -555.0
    if form["res2"]:
        res2 = put(special_rows(Mx, W, seed + 5, dev, scale=0.25).bfloat16(), ldin)
    dbuf, dx = out_mat(Mx, W, F32, dev, ldout) if form["outs"] in ("both", "dx") else (None, None)
    bbuf, dxb = out_mat(Mx, W, BF16, dev, ldout) if form["outs"] in ("both", "dxb") else (None, None)
    g = torch.Generator().manual_seed(seed + 6)
    dg0, db0 = torch.randn(W, generator=g).to(dev), torch.randn(W, generator=g).to(dev)
    q8 = form["q8"]
    kw = dict(res1=res1, res2=res2, workspace=workspace)
    if rows is not None:
        kw["rows"] = rows
    if extra or rows is not None:
        kw["M"] = M
    if cls:
        cls_dx = torch.full((M // period, W), float("nan"), device=dev)
        kw.update(cls_period=period, cls_x=cls_x, cls_res1=cls_res1, cls_dx=cls_dx)

    def launch(**more):
        dgb, dbb = put_vec(dg0), put_vec(db0)
        for b in (dbuf, bbuf):
            if b is not None:
                b.fill_(float("nan"))
        K.layernorm_bwd(dy, xin, mean, rstd, gamma, dx, dx_bf16=dxb, dgamma=dgb, dbeta=dbb, **kw, **more)
        return dgb, dbb

    # the plain run of the same arguments: every form's dx / dx_bf16 / dgamma / dbeta, and what a Q8 run must reproduce
    dg, db = launch()
    plain = [t.clone() if t is not None else None for t in (dx, dxb, dg, db)]
    cols = {}

    def checks(tag):
        r1s = res1.float()[rl] if res1 is not None else None
        r2s = res2.float()[rl] if res2 is not None else None
        xs = seen[rl]
        if cls:  # CLS rows: input and stream gradient from the fp32 side arrays
            xs = truth[:M]
            if r1s is not None:
                r1s = r1s.clone(); r1s[cls_rows] = cls_res1
        w = KB.ln_bwd_check(dy[:M], xs, mean[:M], rstd[:M], gamma, dx=dx[rl] if dx is not None else None,
                            dx_bf16=dxb[rl] if dxb is not None else None, res1=r1s, res2=r2s, what=what + tag)
        if cls:
            w = max(w, KB.ln_bwd_check(dy[cls_rows], truth[cls_rows], mean[cls_rows], rstd[cls_rows], gamma, dx=cls_dx,
                                       res1=cls_res1, res2=r2s[cls_rows] if r2s is not None else None, what=what + tag + " cls_dx"))
            KB.assert_equal_bits(dxb[cls_rows], cls_dx.bfloat16(), what + tag + ": the CLS rows of dx_bf16 are cls_dx rounded")
        keep = torch.ones(Mx, dtype=torch.bool, device=dev); keep[rl] = False
        for name, buf, t in (("dx", dbuf, dx), ("dx_bf16", bbuf, dxb)):
            if t is not None:
                KB.check_guards(buf, Mx, W, f"{what}{tag} {name}")
                assert bool(torch.isnan(t[keep]).all()), f"{what}{tag}: {name} written outside the {M} listed rows"
        w_cols = KB.ln_cols_check(dy[:M], seen[rl], mean[:M], rstd[:M], dg, db, dg0, db0, what=what + tag)
        for k, v in w_cols.items():
            cols[k] = max(cols.get(k, 0.0), v)
        return w

    worst = checks("")
    if workspace:  # the fixed order of the partial sums: a second run, same bits
        dg2, db2 = launch()
        KB.assert_equal_bits(dg2, plain[2], what + ": dgamma of a second run"); KB.assert_equal_bits(db2, plain[3], what + ": dbeta of a second run")
    if cls:  # rows that are no CLS row: the bits of the plain bf16-stream kernel the same arguments reach
        ref = torch.full((M, W), float("nan"), dtype=BF16, device=dev)
        K.layernorm_bwd(dy, xin, mean, rstd, gamma, None, dx_bf16=ref, res1=res1, res2=res2)
        KB.assert_equal_bits(dxb[:M][other], ref[other], what + ": rows that are no CLS row against the plain kernel")
    if not q8:
        return worst, cols
    qbuf, q = out_mat(Mx, W, U8, dev, ldout)
    if q8 == "rows":
        rs = out_vec(Mt, dev)
        dg, db = launch(q8=q, row_scale=rs)
        worst = max(worst, checks(" q8 rows"))
        q8_rows_check(dxb[:M], q[:M], rs, what, K)
        assert bool(torch.isnan(rs[M:]).all()), f"{what}: row_scale written past row {M}"
        if M > ZERO and res1 is None and res2 is None:
            assert float(rs[ZERO]) == 1.0 and int(q[ZERO].max()) == 0, f"{what}: the all-zero row"
        variants = [None]
    else:
        variants = tensor_scale_runs(float(plain[1][:M].float().abs().max()))
    for v in variants:
        if v is not None:
            ts, am0 = v
            tst, amt = torch.tensor([ts], device=dev), torch.tensor([am0], device=dev)
            qbuf.fill_(0xFF)
            dg, db = launch(q8=q, tscale=tst, amax=amt)
            worst = max(worst, checks(f" q8 tensor {ts:g}"))
            q8_tensor_check(dxb[:M], q[:M], tst, what)
            am1 = max(am0, float(dxb[:M].float().abs().max()))
            assert float(amt) == am1, (what, "amax", float(amt), am1, ts, am0)
            if ts > 0 and am0 == 0.0:
                assert int((q[:M] & 0x7F).max()) == 0x7E, f"{what}: nothing saturated under tscale {ts}"
        KB.check_guards(qbuf, Mx, W, what + " q8")
        # the other outputs of a Q8 run: those of the plain run (test_layernorm_bwd_fp8_output)
        KB.assert_equal_bits(dxb, plain[1], what + ": dx_bf16 of the Q8 run")
        if dx is not None:
            KB.assert_equal_bits(dx, plain[0], what + ": dx of the Q8 run")
        assert torch.allclose(dg, plain[2], rtol=1e-5, atol=1e-6) and torch.allclose(db, plain[3], rtol=1e-5, atol=1e-6), what
    return worst, cols


# ------------------------------------------------------------------------------------------------ baselines and refusals
def _fwd(M=5, W=16, ld=24, **kw):
    d = dict(x=Mat(M, ld, F32), ldx=ld, x_bf16=0, rows=None, gamma=Mat(1, W, F32), beta=Mat(1, W, F32), eps=1e-5, M=M, W=W,
             y=Mat(M, ld, BF16), ldy=ld, y_f32=0, mean=Mat(1, M, F32), rstd=Mat(1, M, F32))
    d.update(kw)
    return d


def _fwd8(M=5, W=16, ld=24, **kw):
    d = dict(x=Mat(M, ld, BF16), ldx=ld, x_bf16=1, rows=None, gamma=Mat(1, W, F32), beta=Mat(1, W, F32), eps=1e-5, M=M, W=W,
             y=Mat(M, ld, BF16), ldy=ld, q8=Mat(M, ld, U8, "zero"), ldq=ld, row_scale=Mat(1, M, F32), tscale=None, amax_acc=None,
             mean=Mat(1, M, F32), rstd=Mat(1, M, F32))
    d.update(kw)
    return d


def _fwd_cls(M=6, W=16, ld=24, **kw):
    d = dict(x=Mat(M, ld, BF16), ldx=ld, cls_x=Mat(M // 3, W, F32), cls_period=3, x_refresh=None, gamma=Mat(1, W, F32), beta=Mat(1, W, F32),
             eps=1e-5, M=M, W=W, y=Mat(M, ld, BF16), ldy=ld, q8=Mat(M, ld, U8, "zero"), ldq=ld, row_scale=Mat(1, M, F32), tscale=None,
             amax_acc=None, mean=Mat(1, M, F32), rstd=Mat(1, M, F32))
    d.update(kw)
    return d


def _bwd(M=5, W=16, ld=24, **kw):
    d = dict(dy=Mat(M, ld, BF16), lddy=ld, dy_f32=0, x=Mat(M, ld, F32), ldx=ld, x_bf16=0, rows=None, mean=Mat(1, M, F32, "zero"),
             rstd=Mat(1, M, F32, 1.0), gamma=Mat(1, W, F32), res1=Mat(M, ld, F32), res1_bf16=0, ldr=ld, res2_bf16=Mat(M, ld, BF16), ldr2=ld,
             M=M, W=W, dx=Mat(M, ld, F32), lddx=ld, dx_bf16=Mat(M, ld, BF16), lddxb=ld, dgamma=Mat(1, W, F32), dbeta=Mat(1, W, F32),
             workspace=Mat(1, 4096, F32), workspace_elems=4096)
    d.update(kw)
    return d


def _bwd8(M=5, W=16, ld=24, **kw):
    d = dict(dy=Mat(M, ld, BF16), lddy=ld, x=Mat(M, ld, F32), ldx=ld, x_bf16=0, mean=Mat(1, M, F32, "zero"), rstd=Mat(1, M, F32, 1.0),
             gamma=Mat(1, W, F32), res1=Mat(M, ld, F32), res1_bf16=0, ldr=ld, res2_bf16=Mat(M, ld, BF16), ldr2=ld, M=M, W=W,
             dx=Mat(M, ld, F32), lddx=ld, dx_bf16=Mat(M, ld, BF16), lddxb=ld, q8=Mat(M, ld, U8, "zero"), ldq=ld, row_scale=Mat(1, M, F32),
             tscale=None, amax_acc=None, dgamma=Mat(1, W, F32), dbeta=Mat(1, W, F32), workspace=Mat(1, 4096, F32), workspace_elems=4096)
    d.update(kw)
    return d


def _bwd_cls(M=6, W=16, ld=24, **kw):
    d = dict(dy=Mat(M, ld, BF16), lddy=ld, x=Mat(M, ld, BF16), ldx=ld, cls_x=Mat(M // 3, W, F32), cls_res1=Mat(M // 3, W, F32),
             cls_dx=Mat(M // 3, W, F32), cls_period=3, mean=Mat(1, M, F32, "zero"), rstd=Mat(1, M, F32, 1.0), gamma=Mat(1, W, F32),
             res1_bf16=Mat(M, ld, BF16), ldr=ld, res2_bf16=Mat(M, ld, BF16), ldr2=ld, M=M, W=W, dx_bf16=Mat(M, ld, BF16), lddxb=ld,
             q8=Mat(M, ld, U8, "zero"), ldq=ld, row_scale=Mat(1, M, F32), tscale=None, amax_acc=None, dgamma=Mat(1, W, F32),
             dbeta=Mat(1, W, F32), workspace=Mat(1, 4096, F32), workspace_elems=4096)
    d.update(kw)
    return d


# name -> (entry point, its arguments by the header's names; `stream` is added by the caller).  Every leading dimension (24) is
# larger than its row (16), so that "shorter than the row" and "not divisible" are told apart.
BASELINES = {
    "fwd": ("tvts_layernorm_fwd", _fwd()),
    "fwd_bf16": ("tvts_layernorm_fwd", _fwd(x=Mat(5, 24, BF16), x_bf16=1)),
    "fwd_fp8": ("tvts_layernorm_fwd_fp8", _fwd8()),
    "fwd_fp8_only": ("tvts_layernorm_fwd_fp8", _fwd8(y=None, ldy=0)),
    "fwd_cls": ("tvts_layernorm_fwd_cls", _fwd_cls()),
    "fwd_cls_only": ("tvts_layernorm_fwd_cls", _fwd_cls(y=None, ldy=0)),
    "bwd": ("tvts_layernorm_bwd", _bwd()),
    "bwd_bf16": ("tvts_layernorm_bwd", _bwd(x=Mat(5, 24, BF16), x_bf16=1, res1=Mat(5, 24, BF16), res1_bf16=1)),
    "bwd_fp8": ("tvts_layernorm_bwd_fp8", _bwd8()),
    "bwd_fp8_bf16": ("tvts_layernorm_bwd_fp8", _bwd8(x=Mat(5, 24, BF16), x_bf16=1, res1=Mat(5, 24, BF16), res1_bf16=1)),
    "bwd_cls": ("tvts_layernorm_bwd_cls", _bwd_cls()),
}

# (baseline, the ONE argument changed, its value, why the call is refused).  "pin": refused before this table existed.
REFUSALS = [
    # ---- tvts_layernorm_fwd
    ("fwd", "W", 14, "pin: W % 4"), ("fwd", "W", 1284, "pin: W > 1280"), ("fwd", "W", 0, "pin: W <= 0"), ("fwd", "M", 0, "pin: M <= 0"),
    ("fwd", "M", -1, "pin: M <= 0"), ("fwd", "ldx", 22, "pin: ldx % 4"), ("fwd", "ldy", 22, "pin: ldy % 4"),
    ("fwd_bf16", "y_f32", 1, "pin: bf16 x with fp32 y"),
    ("fwd", "ldx", 12, "ldx < W"), ("fwd", "ldx", 0, "ldx < W (every row the first: passes ldx % 4)"), ("fwd", "ldy", 12, "ldy < W"),
    ("fwd", "x", None, "null x"), ("fwd", "gamma", None, "null gamma"), ("fwd", "beta", None, "null beta"), ("fwd", "y", None, "null y"),
    # ---- tvts_layernorm_fwd_fp8
    ("fwd_fp8", "W", 14, "pin: W % 4"), ("fwd_fp8", "W", 1284, "pin: W > 1280"), ("fwd_fp8", "M", 0, "pin: M <= 0"),
    ("fwd_fp8", "ldx", 22, "pin: ldx % 4"), ("fwd_fp8", "ldy", 22, "pin: ldy % 4"), ("fwd_fp8", "ldq", 22, "pin: ldq % 4"),
    ("fwd_fp8", "q8", None, "pin: no q8"), ("fwd_fp8", "row_scale", None, "pin: q8 without a scale"),
    ("fwd_fp8_only", "x_bf16", 0, "pin: e4m3-only on fp32 x"), ("fwd_fp8_only", "W", 12, "pin: e4m3-only with W % 8"),
    ("fwd_fp8_only", "ldx", 20, "pin: e4m3-only with ldx % 8"), ("fwd_fp8_only", "ldq", 20, "pin: e4m3-only with ldq % 8"),
    ("fwd_fp8", "ldx", 12, "ldx < W"), ("fwd_fp8", "ldy", 12, "ldy < W"), ("fwd_fp8", "ldq", 12, "ldq < W"), ("fwd_fp8", "ldq", 0, "ldq < W"),
    ("fwd_fp8", "x", None, "null x"), ("fwd_fp8", "gamma", None, "null gamma"), ("fwd_fp8", "beta", None, "null beta"),
    ("fwd_fp8_only", "ldx", 8, "ldx < W"), ("fwd_fp8_only", "ldq", 8, "ldq < W"),
    # ---- tvts_layernorm_fwd_cls
    ("fwd_cls", "W", 14, "pin: W % 4"), ("fwd_cls", "M", 0, "pin: M <= 0"), ("fwd_cls", "ldx", 22, "pin: ldx % 4"), ("fwd_cls", "ldy", 22, "pin: ldy % 4"),
    ("fwd_cls", "ldq", 22, "pin: ldq % 4"), ("fwd_cls", "cls_x", None, "pin: no cls_x"), ("fwd_cls", "cls_period", 0, "pin: cls_period <= 0"),
    ("fwd_cls", "cls_period", 4, "pin: M % cls_period"), ("fwd_cls", "row_scale", None, "pin: q8 without a scale"),
    ("fwd_cls_only", "q8", None, "pin: neither y nor q8"), ("fwd_cls_only", "W", 12, "pin: e4m3-only with W % 8"),
    ("fwd_cls_only", "ldx", 20, "pin: e4m3-only with ldx % 8"), ("fwd_cls_only", "ldq", 20, "pin: e4m3-only with ldq % 8"),
    ("fwd_cls", "ldx", 12, "ldx < W"), ("fwd_cls", "ldy", 12, "ldy < W"), ("fwd_cls", "ldq", 12, "ldq < W"),
    ("fwd_cls", "x", None, "null x"), ("fwd_cls", "gamma", None, "null gamma"), ("fwd_cls", "beta", None, "null beta"),
    # ---- tvts_layernorm_bwd
    ("bwd", "W", 14, "pin: W % 4"), ("bwd", "W", 1284, "pin: W > 1280"), ("bwd", "M", 0, "pin: M <= 0"), ("bwd", "lddy", 22, "pin: lddy % 4"),
    ("bwd", "ldx", 22, "pin: ldx % 4"), ("bwd", "ldr", 22, "pin: ldr % 4"), ("bwd", "ldr2", 22, "pin: ldr2 % 4"), ("bwd", "lddx", 22, "pin: lddx % 4"),
    ("bwd", "lddxb", 22, "pin: lddxb % 4"),
    ("bwd_bf16", "dy_f32", 1, "pin: bf16 x with fp32 dy"), ("bwd_bf16", "res1_bf16", 0, "pin: bf16 x with fp32 res1"),
    ("bwd", "lddy", 12, "lddy < W"),
    ("bwd", "ldx", 12, "ldx < W"), ("bwd", "ldx", 0, "ldx < W"), ("bwd", "ldr", 12, "ldr < W"), ("bwd", "ldr", 0, "ldr < W (a broadcast row: passes ldr % 4)"),
    ("bwd", "ldr2", 12, "ldr2 < W"), ("bwd", "lddx", 12, "lddx < W"), ("bwd", "lddxb", 12, "lddxb < W"),
    ("bwd", "dy", None, "null dy"), ("bwd", "x", None, "null x"), ("bwd", "mean", None, "null mean"), ("bwd", "rstd", None, "null rstd"),
    ("bwd", "gamma", None, "null gamma"), ("bwd", "dbeta", None, "dgamma without dbeta"), ("bwd", "dgamma", None, "dbeta without dgamma"),
    ("bwd", "workspace_elems", -1, "workspace_elems < 0"),
    # ---- tvts_layernorm_bwd_fp8
    ("bwd_fp8", "W", 14, "pin: W % 4"), ("bwd_fp8", "M", 0, "pin: M <= 0"), ("bwd_fp8", "lddy", 22, "pin: lddy % 4"), ("bwd_fp8", "ldx", 22, "pin: ldx % 4"),
    ("bwd_fp8", "ldr", 22, "pin: ldr % 4"), ("bwd_fp8", "ldr2", 22, "pin: ldr2 % 4"), ("bwd_fp8", "lddx", 22, "pin: lddx % 4"),
    ("bwd_fp8", "lddxb", 22, "pin: lddxb % 4"), ("bwd_fp8", "ldq", 22, "pin: ldq % 4"), ("bwd_fp8", "dx_bf16", None, "pin: no dx_bf16"),
    ("bwd_fp8", "q8", None, "pin: no q8"), ("bwd_fp8", "row_scale", None, "pin: q8 without a scale"), ("bwd_fp8", "res1", None, "pin: res2 without res1"),
    ("bwd_fp8_bf16", "res1_bf16", 0, "pin: bf16 x with fp32 res1"), ("bwd_fp8_bf16", "res1", None, "pin: res2 without res1"),
    ("bwd_fp8", "lddy", 12, "lddy < W"), ("bwd_fp8", "ldx", 12, "ldx < W"), ("bwd_fp8", "ldr", 12, "ldr < W"), ("bwd_fp8", "ldr2", 12, "ldr2 < W"),
    ("bwd_fp8", "lddx", 12, "lddx < W"), ("bwd_fp8", "lddxb", 12, "lddxb < W"), ("bwd_fp8", "ldq", 12, "ldq < W"),
    ("bwd_fp8", "dy", None, "null dy"), ("bwd_fp8", "x", None, "null x"), ("bwd_fp8", "mean", None, "null mean"), ("bwd_fp8", "rstd", None, "null rstd"),
    ("bwd_fp8", "gamma", None, "null gamma"), ("bwd_fp8", "dbeta", None, "dgamma without dbeta"), ("bwd_fp8", "dgamma", None, "dbeta without dgamma"),
    ("bwd_fp8", "workspace_elems", -1, "workspace_elems < 0"),
    # ---- tvts_layernorm_bwd_cls
    ("bwd_cls", "W", 14, "pin: W % 4"), ("bwd_cls", "M", 0, "pin: M <= 0"), ("bwd_cls", "lddy", 22, "pin: lddy % 4"), ("bwd_cls", "ldx", 22, "pin: ldx % 4"),
    ("bwd_cls", "ldr", 22, "pin: ldr % 4"), ("bwd_cls", "ldr2", 22, "pin: ldr2 % 4"), ("bwd_cls", "lddxb", 22, "pin: lddxb % 4"),
    ("bwd_cls", "ldq", 22, "pin: ldq % 4"), ("bwd_cls", "dx_bf16", None, "pin: no dx_bf16"), ("bwd_cls", "row_scale", None, "pin: q8 without a scale"),
    ("bwd_cls", "res1_bf16", None, "pin: res2 (and cls_res1) without res1"), ("bwd_cls", "cls_period", 0, "pin: cls_period <= 0"),
    ("bwd_cls", "cls_period", 4, "pin: M % cls_period"),
    ("bwd_cls", "lddy", 12, "lddy < W"), ("bwd_cls", "ldx", 12, "ldx < W"), ("bwd_cls", "ldr", 12, "ldr < W"), ("bwd_cls", "ldr2", 12, "ldr2 < W"),
    ("bwd_cls", "lddxb", 12, "lddxb < W"), ("bwd_cls", "ldq", 12, "ldq < W"),
    ("bwd_cls", "dy", None, "null dy"), ("bwd_cls", "x", None, "null x"), ("bwd_cls", "mean", None, "null mean"), ("bwd_cls", "rstd", None, "null rstd"),
    ("bwd_cls", "gamma", None, "null gamma"), ("bwd_cls", "dbeta", None, "dgamma without dbeta"), ("bwd_cls", "dgamma", None, "dbeta without dgamma"),
    ("bwd_cls", "workspace_elems", -1, "workspace_elems < 0"),
]


def call(lib, protos, name, alloc, stream=None, **change):
    """the baseline `name` with the arguments of `change` replaced -> the entry point's return code.  alloc(Mat) -> a pointer"""
    fn, base = BASELINES[name]
    args = dict(base)
    bad = set(change) - set(args)
    assert not bad, (name, bad)
    args.update(change)
    vals = []
    for an in protos[fn][2]:
        if an == "stream":
            vals.append(stream)
            continue
        v = args[an]
        vals.append(alloc(v) if isinstance(v, Mat) else v)
    return getattr(lib, fn)(*vals)


# ------------------------------------------------------------------------------------------------ an fp32 emulation of the kernels
class Emulation:
    """layernorm_fwd / layernorm_bwd / quantize_fp8_rows of tvts_amd.hip in plain fp32 torch on any device: two-pass mean and
    variance, fp32 accumulation, the bf16 rounding before the e4m3 copy, results written through the same strided views and row
    lists.  fwd_case / bwd_case run on it as they run on the kernels (tests/test_kernel_bounds_cpu.py).

    mistake: what a kernel gets wrong at a width or row edge --
      "var_tail"    the variance without the last four columns          "c12_tail"   the backward's row means c1 / c2 without them
      "amax_tail"   the amax of the e4m3 copy without the tail group    "dgamma_tail" dgamma / dbeta missing the last four columns' sums
      "row_late"    the last row's result written one row late"""

    def __init__(self, mistake=None):
        self.mistake = mistake

    @staticmethod
    def _scale(out16, tscale, amax, tail_free=False):
        v = out16.float().abs()
        am_rows = (v[:, :-4] if tail_free and v.shape[1] > 4 else v).amax(1)
        if amax is not None:
            amax.copy_(torch.maximum(amax, am_rows.max().reshape(1)))
        if tscale is not None:
            s = tscale.float().reshape(())
            return torch.where(s > 0, s, torch.ones_like(s)).expand(out16.shape[0])
        return torch.where(am_rows > 0, am_rows / 448.0, torch.ones_like(am_rows))

    def quantize_fp8_rows(self, x, q=None, row_scale=None, tscale=None, amax=None):
        s = self._scale(x, tscale, amax)
        return e4m3_bits(x, (1.0 / s)[:, None]), (None if tscale is not None else s)

    @staticmethod
    def _store(t, dst, val):
        ok = dst < t.shape[0]  # (a row written past the view would land in the guard rows: dropped here)
        t[dst[ok]] = val[ok]

    def _dst(self, M, rows_idx):
        idx = rows_idx.clone()
        if self.mistake == "row_late" and M > 1:
            idx[-1] = idx[-1] + 1
        return idx

    def layernorm_fwd(self, x, gamma, beta, eps, y, mean=None, rstd=None, rows=None, M=None, q8=None, row_scale=None, tscale=None,
                      amax=None, cls_x=None, cls_period=0, refresh=True):
        M = (rows.numel() if rows is not None else x.shape[0]) if M is None else M
        W = x.shape[1]
        src = rows.long()[:M] if rows is not None else torch.arange(M, device=x.device)
        v = x[src].float()
        if cls_x is not None:
            cr = torch.arange(0, M, cls_period, device=x.device)
            v[cr] = cls_x
            if refresh:
                x[cr] = cls_x.to(x.dtype)
        mu = v.sum(1, keepdim=True) / W
        d = v - mu
        sq = d * d
        if self.mistake == "var_tail" and W > 4:
            sq = sq[:, :-4]
        rs = torch.rsqrt(sq.sum(1, keepdim=True) / W + eps)
        o = d * rs * gamma.float() + beta.float()
        dst = self._dst(M, torch.arange(M, device=x.device))
        ydt = y.dtype if y is not None else BF16
        if y is not None:
            self._store(y, dst, o.to(ydt))
        if mean is not None:
            mean[:M] = mu[:, 0]
        if rstd is not None:
            rstd[:M] = rs[:, 0]
        if q8 is not None:
            o16 = o.to(BF16)
            s = self._scale(o16, tscale, amax, self.mistake == "amax_tail")
            self._store(q8, dst, e4m3_bits(o16, (1.0 / s)[:, None]))
            if row_scale is not None and tscale is None:
                row_scale[:M] = s

    def layernorm_bwd(self, dy, x, mean, rstd, gamma, dx, *, dx_bf16=None, res1=None, res2=None, dgamma=None, dbeta=None, rows=None,
                      M=None, workspace=True, q8=None, row_scale=None, tscale=None, amax=None, cls_period=0, cls_x=None, cls_res1=None,
                      cls_dx=None):
        M = (rows.numel() if rows is not None else x.shape[0]) if M is None else M
        W = x.shape[1]
        src = rows.long()[:M] if rows is not None else torch.arange(M, device=x.device)
        g32 = gamma.float()

        def rows_out(xv, r1v, which):
            d = dy[:M].float()[which]
            xh = (xv - mean[:M][which, None]) * rstd[:M][which, None]
            g = d * g32
            gs, gx = g, g * xh
            if self.mistake == "c12_tail" and W > 4:
                gs, gx = gs[:, :-4], gx[:, :-4]
            c1, c2 = gs.sum(1, keepdim=True) / W, gx.sum(1, keepdim=True) / W
            o = rstd[:M][which, None] * (g - c1 - xh * c2)
            if r1v is not None:
                o = o + r1v
            if res2 is not None:
                o = o + res2[src].float()[which]
            return o, d, xh

        every = torch.arange(M, device=x.device)
        o, d, xh = rows_out(x[src].float(), res1[src].float() if res1 is not None else None, every)
        if dgamma is not None:
            ag, ab = (d * xh).sum(0), d.sum(0)
            if self.mistake == "dgamma_tail":
                ag[-4:], ab[-4:] = 0.0, 0.0
            dgamma += ag
            dbeta += ab
        if cls_period:
            cr = torch.arange(0, M, cls_period, device=x.device)
            oc, _, _ = rows_out(cls_x if cls_x is not None else x[cr].float(),
                                cls_res1 if cls_res1 is not None else (res1[cr].float() if res1 is not None else None), cr)
            o[cr] = oc
            if cls_dx is not None:
                cls_dx.copy_(oc)
        dst = self._dst(M, src) if rows is None else src
        if dx is not None:
            self._store(dx, dst, o)
        if dx_bf16 is not None:
            self._store(dx_bf16, dst, o.to(BF16))
        if q8 is not None:
            o16 = o.to(BF16)
            s = self._scale(o16, tscale, amax, self.mistake == "amax_tail")
            self._store(q8, dst, e4m3_bits(o16, (1.0 / s)[:, None]))
            if row_scale is not None and tscale is None:
                row_scale[:M] = s
