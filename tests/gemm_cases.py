"""Shared cases of the GEMM tests (a plain helper module, imported by the tests): operands inside NaN-poisoned buffers, the form
loops of the per-element bound tests, which kernel a case was written for, and one table of valid baseline calls with the
single-argument changes every entry point must refuse.

tests/test_kernels_gpu.py runs the form loops at the training step's sizes, tests/test_gemm_edges_gpu.py at the smallest shapes
that reach each edge path of a kernel (rows / columns sticking out of a wave tile, views whose leading dimension is not their
width); tests/test_gemm_args_cpu.py calls every refusal of REFUSALS without a GPU, tests/test_gemm_edges_gpu.py launches every
baseline of BASELINES once, so a refusal cannot pass because some other argument of its call was wrong as well."""
import ctypes

import torch

import kernel_bounds as KB

BF16, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32


# ------------------------------------------------------------------------------------------------ poisoned operands
def poisoned(M, W, dtype, device, rows=3, left=8, right=8):
    """an [M, W] operand view at row 0, column `left` of an [M + rows, left + W + right] buffer whose every other element is NaN
    (0x7F, the e4m3 NaN, for uint8); -> (buffer, view).  left / right are multiples of 16 bytes (8 elements of bf16 / fp32, 16 of
    uint8) and `right` grows to the next row pitch that is one as well, so every row of the view starts on a 16-byte boundary.
    A kernel that clamps rows to M - 1 and never reads past its K / N columns never uses poison; one that over-reads a stage, a
    row or a column carries NaN into a checked output."""
    esz = torch.empty((), dtype=dtype).element_size()
    assert (left * esz) % 16 == 0 and (right * esz) % 16 == 0, (left, right, dtype)
    while ((left + W + right) * esz) % 16:
        right += 1
    if dtype.is_floating_point:
        buf = torch.full((M + rows, left + W + right), float("nan"), dtype=dtype, device=device)
    else:
        buf = torch.full((M + rows, left + W + right), 0x7F, dtype=torch.uint8, device=device)
    return buf, buf[:M, left:left + W]


def place(t):
    """a copy of the 2-D (or 1-D: one row) tensor t as a poisoned view"""
    pad = 16 if t.dtype == U8 else 8
    if t.dim() == 1:
        _, v = poisoned(1, t.numel(), t.dtype, t.device, left=pad, right=pad)
        v.copy_(t[None])
        return v[0]
    _, v = poisoned(t.shape[0], t.shape[1], t.dtype, t.device, left=pad, right=pad)
    v.copy_(t)
    return v


def place_pair(p, q, gap=8):
    """p [M, Na] and q [M, Nb] as column slices of ONE poisoned buffer with `gap` NaN columns between them (leading dimension of
    both = 8 + Na + gap + Nb + 8, not their width); an over-read to the right of p meets the gap, not q"""
    pad = 16 if p.dtype == U8 else 8
    gap = max(gap, pad)
    Na, Nb = p.shape[1], q.shape[1]
    _, v = poisoned(p.shape[0], Na + gap + Nb, p.dtype, p.device, left=pad, right=pad)
    v[:, Na:Na + gap] = float("nan") if p.dtype.is_floating_point else 0x7F
    pv, qv = v[:, :Na], v[:, Na + gap:]
    pv.copy_(p)
    qv.copy_(q)
    return pv, qv


def nt_operands(M, N, Kd, seed, device, strided=True):
    """a [M, Kd], b [N, Kd] (bf16), bias [N] (fp32), an fp32 residual and a bf16 gate input [M, N] -- all poisoned views"""
    g = torch.Generator(device=device).manual_seed(seed)
    a = torch.randn(M, Kd, generator=g, device=device).bfloat16()
    b = (torch.randn(N, Kd, generator=g, device=device) * Kd ** -0.5).bfloat16()
    bias = torch.randn(N, generator=g, device=device)
    res = torch.randn(M, N, generator=g, device=device)
    h = (torch.randn(M, N, generator=g, device=device) * 1.5).bfloat16()
    if strided:
        a, b, bias, res, h = (place(t) for t in (a, b, bias, res, h))
    return a, b, bias, res, h


# ------------------------------------------------------------------------------------------------ which kernel
NT_KERNEL = {256: 256, 128: 128, "128noring": 128, "ring2": 1128, "ring3": 1192, "ring4": 1256}


def expect_kernel(K, M, N, tile):
    """the case was written for the kernel `tile` names: tvts_gemm_nt_select must report it (256: the pipelined 256 x 256 kernel,
    128: the double-buffered 128 x 128 one, 1128 / 1192 / 1256: the ring form with 128 / 192 / 256 tile rows)"""
    got = K.gemm_nt_select(M, N, tile=tile)
    assert got == NT_KERNEL[tile], f"a [{M}, {N}] result under tile={tile!r} runs on kernel {got}, the case is written for {NT_KERNEL[tile]}"
    return got


def tn_ranges(M, splits, stage=64):
    """the contraction ranges tvts_gemm_tn_bf16 makes of a forced range count (it renormalises: ranges are whole 64-row stages) ->
    (ranges, rows of the last one)"""
    cdiv = lambda x, y: -(-x // y)  # noqa: E731
    per = cdiv(cdiv(M, splits), stage) * stage
    n = cdiv(M, per)
    return n, M - (n - 1) * per


# ------------------------------------------------------------------------------------------------ the side kernels' edge cases
# (tests/test_gemm_side_edges_gpu.py runs them, tests/test_kernel_bounds_cpu.py plants faults at the smallest of them)
COLSUM_M = (1, 31, 33, 4096, 4097, 8193)  # one row; either side of the 32 row lanes; one range, two (2049 + 2048 rows), three
COLSUM_N = (8, 72, 136)                   # one column thread; a ragged second / third 64-column block
COLSUM_RANGE_ROWS = 4096                  # tvts_colsum_bf16: ceil(M / 4096) row ranges, at most 256, when the workspace holds them
# (M, N, K) of tvts_gemm_small_f32 around its dispatch cut (the fp32 MFMA tile from M >= 32, N >= 32, K >= 16)
SMALL_SHAPES = ((31, 32, 16), (32, 31, 16), (32, 32, 15), (32, 32, 16), (33, 65, 17), (64, 64, 32), (65, 63, 33), (64, 64, 64),
                (36, 40, 20), (1, 1, 1), (17, 5, 3))
ROWS_LINEAR_R = (1, 15, 16, 17, 33)
ROWS_LINEAR_K = (32, 64, 96, 128, 160, 416, 512, 544)  # waves without a step; either side of the unrolled loop for waves 0 and 3
ROWS_LINEAR_N = (16, 48)
# name -> (forced range count, [(M, Na, Nb, accumulate, colsum, strided output)]) of tvts_gemm_tn_bf16_grouped
TN_GROUPS = {
    "one_strided": (2, [(65, 136, 72, False, True, True)]),
    "one_dense": (2, [(65, 136, 72, True, True, False)]),
    "one_split_dense": (2, [(520, 136, 72, True, True, False)]),
    "trio_unsplit": (1, [(520, 136, 72, True, True, True), (520, 264, 8, False, False, False), (520, 128, 392, True, False, True)]),
    "trio": (2, [(520, 136, 72, True, True, True), (520, 264, 8, False, False, False), (520, 128, 392, True, False, True)]),
    "mixed_m": (2, [(1040, 136, 264, True, True, True), (300, 72, 136, False, False, True), (1040, 8, 8, False, True, False)]),
    "few_items": (2, [(520, 8, 8, False, False, True), (64, 136, 8, True, True, False)]),
}


def small_vec_eligible(M, N, Kd, sa, sb):
    """tvts_gemm_small_f32 stages the problem with 16-byte loads (given aligned bases): the MFMA tile, each operand unit-stride in
    one direction with the other stride and the extent along the vector multiples of 4"""
    if not (M >= 32 and N >= 32 and Kd >= 16):
        return False
    va = (sa[0] % 4 == 0 and Kd % 4 == 0) if sa[1] == 1 else (sa[0] == 1 and sa[1] % 4 == 0 and M % 4 == 0)
    vb = (sb[0] % 4 == 0 and N % 4 == 0) if sb[1] == 1 else (sb[0] == 1 and sb[1] % 4 == 0 and Kd % 4 == 0)
    return va and vb


def tn_group_ranges(M, splits):
    """the contraction ranges a member of a grouped launch gets from the group's range count: a member keeps at least 256 rows per
    range (it takes fewer ranges than the group), then whole 64-row stages as in tn_ranges -> (ranges, rows of the last one)"""
    sp = max(int(splits), 1)
    while sp > 1 and M // sp < 256:
        sp -= 1
    return tn_ranges(M, sp)


def tn_group_items(problems, splits):
    """work items of a grouped launch: 128 x 128 output tiles times ranges, summed over the members"""
    cdiv = lambda x, y: -(-x // y)  # noqa: E731
    return sum(cdiv(Na, 128) * cdiv(Nb, 128) * tn_group_ranges(M, splits)[0] for (M, Na, Nb, *_) in problems)


# ------------------------------------------------------------------------------------------------ form loops
def form(got, a, b, **kw):
    """check_gemm of one form, its own line in the record"""
    acc0 = KB.pop_acc_worst()
    w = KB.check_gemm(got, a, b, **kw)
    acc = KB.pop_acc_worst()
    print(f"FORM {kw['what']} {w:.4g} acc {acc:.4g}")
    KB.ACC_WORST[0] = max(acc0, acc)
    return w


def _name(f):
    return "streamk" if f.get("streamk") else str(f.get("tile"))


def _nt(K, f, *args, **kw):
    """gemm_nt under the form f; a stream-K form must have taken the walk"""
    sk0 = K.STREAMK_TAKEN[0]
    K.gemm_nt(*args, **kw, **f)
    if f.get("streamk"):
        assert K.STREAMK_TAKEN[0] == sk0 + 1, "stream-K accepted but not taken"


def nt_forms(K, a, b, bias, res, h, *, forms, act_forms, must_take=(), edge=False, cols=8):
    """NT plain / epilogues / side_deriv / stream-K / ring forms, every element within gemm_bound, guard rows and columns kept.
    forms: the dispatch options of the plain launches (bf16 and fp32 result with bias; fp32 residual into an fp32 result where the
    form is a tile kernel); act_forms: those of both activations with their pre-activation side output and of both gates, with
    side_deriv off and on; then the bf16 residual stream through the gate slot.  A form the shape cannot take may refuse it
    (stream-K and ring forms only) unless must_take names it.
    edge (tests/test_gemm_edges_gpu.py): every form also runs the fp32 residual into fp32 and bf16 results and the plain product
    with no bias into bf16, and the bf16 residual stream runs under every act_form.  -> (worst |err| / bound, forms taken)"""
    M, N = a.shape[0], b.shape[0]
    DEV = a.device
    worst = 0.0
    taken = set()
    for f in forms:
        name = _name(f)
        for dt in (torch.bfloat16, torch.float32):
            buf, out = KB.guarded(M, N, dt, DEV, cols=cols)
            sk0 = K.STREAMK_TAKEN[0]
            try:
                K.gemm_nt(a, b, out, bias=bias, **f)
            except K.HipError:
                assert f.get("streamk") or "ring" in str(f.get("tile")), f  # a form the shape cannot take refuses it (no silent fall-back)
                print(f"FORM nt {name} {dt} refused at {M},{N},{a.shape[1]}")
                continue
            if f.get("streamk"):
                assert K.STREAMK_TAKEN[0] == sk0 + 1, "stream-K accepted but not taken"
            taken.add(name)
            worst = max(worst, KB.check_gemm(out, a, b, bias=bias, what=f"nt {f} {dt}"))
            KB.check_guards(buf, M, N, f"nt {f} {dt}")
        buf, out = KB.guarded(M, N, torch.float32, DEV, cols=cols)
        if (edge and name in taken) or (f.get("streamk") is None and "ring" not in str(f.get("tile"))):
            _nt(K, f, a, b, out, bias=bias, residual=res)
            worst = max(worst, KB.check_gemm(out, a, b, bias=bias, residual=res, what=f"nt residual {f}"))
            KB.check_guards(buf, M, N)
        if edge and name in taken:
            buf, out = KB.guarded(M, N, torch.bfloat16, DEV, cols=cols)
            _nt(K, f, a, b, out, bias=bias, residual=res)
            worst = max(worst, KB.check_gemm(out, a, b, bias=bias, residual=res, what=f"nt residual bf16 {f}"))
            KB.check_guards(buf, M, N, f"nt residual bf16 {f}")
            buf, out = KB.guarded(M, N, torch.bfloat16, DEV, cols=cols)
            _nt(K, f, a, b, out)
            worst = max(worst, KB.check_gemm(out, a, b, what=f"nt plain no bias {f}"))
            KB.check_guards(buf, M, N, f"nt plain no bias {f}")
    for act in ("quick_gelu", "gelu"):
        for af in act_forms:
            tile = _name(af) if af.get("streamk") else af.get("tile")
            for deriv in (False, True):
                buf, out = KB.guarded(M, N, torch.bfloat16, DEV, cols=cols)
                pbuf, pre = KB.guarded(M, N, torch.bfloat16, DEV, cols=cols)
                _nt(K, af, a, b, out, bias=bias, act=act, preact=pre, side_deriv=deriv)
                worst = max(worst, KB.check_gemm(out, a, b, bias=bias, act=act, preact=pre, deriv=deriv, what=f"nt {act} {tile} {deriv}"))
                KB.check_guards(buf, M, N); KB.check_guards(pbuf, M, N)
                gbuf, gout = KB.guarded(M, N, torch.bfloat16, DEV, cols=cols)
                hh = pre if deriv else h
                _nt(K, af, a, b, gout, gate_h=hh, gate_act=act, side_deriv=deriv)
                worst = max(worst, KB.check_gemm(gout, a, b, gate_h=hh, gate_act=act, deriv=deriv, what=f"nt gate {act} {tile} {deriv}"))
                KB.check_guards(gbuf, M, N)
    for af in (act_forms if edge else [dict()]):
        buf, out = KB.guarded(M, N, torch.bfloat16, DEV, cols=cols)
        _nt(K, af, a, b, out, bias=bias, residual=h)  # the bf16 residual stream through the gate slot
        worst = max(worst, KB.check_gemm(out, a, b, bias=bias, add_bf16=h, what=f"nt bf16 residual {af}" if edge else "nt bf16 residual"))
        KB.check_guards(buf, M, N)
    missing = set(must_take) - taken
    assert not missing, f"forms refused at {M},{N},{a.shape[1]}: {missing}"
    return worst, taken


def tn_forms(K, p, q, init, kws, *, may_refuse=lambda kw: bool(kw.get("fused")), cs_init=None):
    """TN (weight gradient) under every dispatch of kws, accumulate off and on: every element within gemm_bound with K = M, guard
    columns untouched (row pitch ldo > Nb).  A refusal is only allowed where may_refuse(kw) says so (default: the fused reduce,
    which needs more than one range).  cs_init [Na] (tests/test_gemm_edges_gpu.py): every launch runs again with the fused bias
    gradient colsum, accumulated on top of cs_init: every column within sum_bound (n = M addends and the initial value) of the
    float64 column sum of p, and the element after colsum[Na - 1] kept.  -> (worst |err| / bound, launches that ran fused)"""
    M, Na, Nb = p.shape[0], p.shape[1], q.shape[1]
    DEV = p.device
    pt, qt = p.t(), q.t()
    worst = 0.0
    fused_runs = 0
    if cs_init is not None:
        cs_ref = p.double().sum(0) + cs_init.double()
        cs_bound = KB.sum_bound(p.double().abs().sum(0), M, init=cs_init)
    for kw in kws:
        for accumulate in (False, True):
            for with_cs in ((False, True) if cs_init is not None else (False,)):
                buf, out = KB.guarded(Na, Nb, torch.float32, DEV)
                if accumulate:
                    out.copy_(init)
                extra = {}
                if with_cs:
                    csbuf = torch.full((Na + 8,), float("nan"), device=DEV)
                    csbuf[:Na] = cs_init
                    extra["colsum"] = csbuf[:Na]
                sk0 = K.STREAMK_TAKEN[0]
                try:
                    K.gemm_tn(p, q, out, accumulate=accumulate, **kw, **extra)
                except K.HipError:
                    assert may_refuse(kw), kw  # the fused reduce needs a split; a one-split shape refuses it
                    print(f"FORM tn fused {kw} refused at {M},{Na},{Nb}")
                    continue
                if kw.get("fused"):
                    assert K.STREAMK_TAKEN[0] == sk0 + 1, "fused reduce accepted but not taken"
                    fused_runs += 1
                what = f"tn {kw} acc={accumulate}" + (" colsum" if with_cs else "")
                worst = max(worst, KB.check_gemm(out, pt, qt, residual=init if accumulate else None, K=M, what=what))
                KB.check_guards(buf, Na, Nb, what)
                if with_cs:
                    worst = max(worst, KB.assert_within(csbuf[:Na], cs_ref, cs_bound, what + ": colsum (per column)"))
                    assert bool(torch.isnan(csbuf[Na:]).all()), f"{what}: colsum written past column {Na}"
    return worst, fused_runs


def fp8_nt_forms(K, a, b8, sb, bias, res, g, *, put=lambda t: t, cols=8):
    """fp8 NT with tensor and row scales (bf16 / fp32 out, bias, residual, GELU + pre-activation) and the fp8 gate form; S of the
    bound over the decoded e4m3 values times |sa sb|.  a: the fp32 activation, quantised here per tensor and per row; g: the
    generator the gate inputs are drawn from; put: how an operand reaches the kernel (tests/test_gemm_edges_gpu.py: `place`)"""
    M, N = a.shape[0], b8.shape[0]
    DEV = a.device
    bd = KB.decode_e4m3(b8)
    worst = 0.0
    for kind in ("tensor", "rows"):
        a8, sa = K.quantize_fp8(a) if kind == "tensor" else K.quantize_fp8_rows(a.bfloat16())
        a8 = put(a8)
        ad = KB.decode_e4m3(a8)
        scale = sa.double() * sb.double() if kind == "rows" else float(sa) * float(sb)
        for dt in (torch.bfloat16, torch.float32):
            buf, out = KB.guarded(M, N, dt, DEV, cols=cols)
            K.gemm_nt_fp8(a8, sa, b8, sb, out, bias=bias)
            worst = max(worst, form(out, ad, bd, scale=scale, bias=bias, what=f"fp8 {kind} {dt}"))
            KB.check_guards(buf, M, N)
        buf, out = KB.guarded(M, N, torch.float32, DEV, cols=cols)
        K.gemm_nt_fp8(a8, sa, b8, sb, out, bias=bias, residual=res)
        worst = max(worst, form(out, ad, bd, scale=scale, bias=bias, residual=res, what=f"fp8 {kind} residual"))
        KB.check_guards(buf, M, N, f"fp8 {kind} residual")
        buf, out = KB.guarded(M, N, torch.bfloat16, DEV, cols=cols)
        pbuf, pre = KB.guarded(M, N, torch.bfloat16, DEV, cols=cols)
        K.gemm_nt_fp8(a8, sa, b8, sb, out, bias=bias, act="gelu", preact=pre)
        worst = max(worst, form(out, ad, bd, scale=scale, bias=bias, act="gelu", preact=pre, what=f"fp8 {kind} gelu"))
        KB.check_guards(buf, M, N); KB.check_guards(pbuf, M, N)
        h = put((torch.randn(M, N, generator=g, device=DEV) * 1.5).bfloat16())
        for act in ("quick_gelu", "gelu"):
            buf, out = KB.guarded(M, N, torch.bfloat16, DEV, cols=cols)
            K.gemm_nt_fp8(a8, sa, b8, sb, out, gate_h=h, gate_act=act)
            worst = max(worst, form(out, ad, bd, scale=scale, gate_h=h, gate_act=act, what=f"fp8 {kind} gate {act}"))
            KB.check_guards(buf, M, N)
    return worst


def fp8_tn_forms(K, p8, sp, q8, sq, init, *, guard=False):
    """fp8 TN: out (+)= sp sq P8^T Q8 over K = M tokens, accumulate off and on, with the workspace and without.  guard
    (tests/test_gemm_edges_gpu.py): the output sits in a guarded buffer (ldo > Nb) whose guards must stay"""
    M, Na, Nb = p8.shape[0], p8.shape[1], q8.shape[1]
    DEV = p8.device
    worst = 0.0
    for accumulate in (False, True):
        for ws in (True, False):
            if guard:
                buf, out = KB.guarded(Na, Nb, torch.float32, DEV)
                if accumulate:
                    out.copy_(init)
            else:
                out = init.clone() if accumulate else torch.full((Na, Nb), float("nan"), device=DEV)
            K.gemm_tn_fp8(p8, sp, q8, sq, out, accumulate=accumulate, workspace=ws)
            worst = max(worst, form(out, KB.decode_e4m3(p8).t(), KB.decode_e4m3(q8).t(), scale=float(sp) * float(sq),
                                    residual=init if accumulate else None, K=M, what=f"fp8 tn acc={accumulate} ws={ws}"))
            if guard:
                KB.check_guards(buf, Na, Nb, f"fp8 tn acc={accumulate} ws={ws}")
    return worst


# ------------------------------------------------------------------------------------------------ baselines and refusals
class Mat:
    """a matrix (or vector: rows = 1) argument of a baseline call: rows x ld elements of dtype.  fill: "randn" (floats: N(0, 1) / 4;
    uint8: e4m3 codes of such values), "zero", or a number (a scale)"""

    def __init__(self, rows, ld, dtype, fill="randn"):
        self.rows, self.ld, self.dtype, self.fill = rows, ld, dtype, fill

    def dummy(self):
        """a host buffer no refused call ever reads"""
        return ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)

    def tensor(self, device, seed):
        n = self.rows * self.ld
        if self.fill == "zero":
            return torch.zeros(n, dtype=self.dtype, device=device)
        if self.fill != "randn":
            return torch.full((n,), float(self.fill), dtype=self.dtype, device=device)
        x = torch.randn(n, generator=torch.Generator().manual_seed(seed)) / 4
        if self.dtype == U8:
            return x.to(torch.float8_e4m3fn).view(U8).to(device)
        return x.to(self.dtype).to(device)


TILE_256, STREAMK = 2, 32  # TVTS_GEMM_TILE_256, TVTS_GEMM_STREAMK (include/tvts_hip.h)
NT_WS = "nt_workspace"     # stands for the stream-K workspace: (pointer, tvts_gemm_nt_workspace_bytes())


def _base_nt(M=5, N=16, Kd=64, ld=72, ldc=24, **kw):
    d = dict(A=Mat(M, ld, BF16), lda=ld, B=Mat(N, ld, BF16), ldb=ld, M=M, N=N, K=Kd, bias=Mat(1, N, F32), residual=None, ldr=0, act=0,
             preact=None, ldp=0, gate_h=None, ldh=0, gate_act=0, out=Mat(M, ldc, BF16), ldc=ldc, out_f32=0, workspace=None,
             workspace_bytes=0, opts=0)
    d.update(kw)
    return d


def _base_nt8(M=5, N=16, Kd=128, ld=144, ldc=24, **kw):
    d = dict(A=Mat(M, ld, U8), lda=ld, B=Mat(N, ld, U8), ldb=ld, M=M, N=N, K=Kd, scale_a=Mat(1, 1, F32, 0.01), scale_a_rows=0,
             scale_b=Mat(1, 1, F32, 0.02), bias=Mat(1, N, F32), residual=None, ldr=0, act=0, preact=None, ldp=0,
             out=Mat(M, ldc, BF16), ldc=ldc, out_f32=0, q8out=None, ldq8=0, q8_scale=None, q8_amax=None, opts=0)
    d.update(kw)
    return d


def _base_nt8_gate(M=5, N=16, Kd=128, ld=144, ldc=24, **kw):
    d = dict(A=Mat(M, ld, U8), lda=ld, B=Mat(N, ld, U8), ldb=ld, M=M, N=N, K=Kd, scale_a=Mat(1, 1, F32, 0.01), scale_a_rows=0,
             scale_b=Mat(1, 1, F32, 0.02), bias=None, gate_h=Mat(M, ldc, BF16), ldh=ldc, gate_act=2, out=Mat(M, ldc, BF16), ldc=ldc,
             q8out=None, ldq8=0, q8_scale=None, q8_amax=None, opts=0)
    d.update(kw)
    return d


# name -> (entry point, its arguments by the header's names; `stream` is added by the caller).  Sizes are the smallest each entry
# point takes; every leading dimension is larger than its row, so that "shorter than the row" and "not divisible" are told apart.
BASELINES = {
    "nt_res": ("tvts_gemm_nt_bf16", _base_nt(residual=Mat(5, 24, F32), ldr=24)),
    "nt_act": ("tvts_gemm_nt_bf16", _base_nt(act=1, preact=Mat(5, 24, BF16), ldp=24)),
    "nt_gate": ("tvts_gemm_nt_bf16", _base_nt(gate_h=Mat(5, 24, BF16), ldh=24, gate_act=1)),
    "nt_act_256": ("tvts_gemm_nt_bf16", _base_nt(act=1, preact=Mat(5, 24, BF16), ldp=24, opts=TILE_256)),
    "nt_gate_256": ("tvts_gemm_nt_bf16", _base_nt(gate_h=Mat(5, 24, BF16), ldh=24, gate_act=1, opts=TILE_256)),
    # the shortest K and the fewest tiles (3 x 4) the stream-K plan of the 256 kernel accepts
    "nt_streamk": ("tvts_gemm_nt_bf16", _base_nt(M=520, N=1016, Kd=192, ld=200, ldc=1024, workspace=NT_WS, workspace_bytes=NT_WS, opts=STREAMK)),
    "nt8_res": ("tvts_gemm_nt_fp8", _base_nt8(residual=Mat(5, 24, F32), ldr=24, out=Mat(5, 24, F32), out_f32=1)),
    "nt8_act_q8": ("tvts_gemm_nt_fp8", _base_nt8(act=2, preact=Mat(5, 24, BF16), ldp=24, q8out=Mat(5, 24, U8, "zero"), ldq8=24,
                                            q8_scale=Mat(1, 1, F32, 2.0 / 448.0), q8_amax=Mat(1, 1, F32, "zero"))),
    "nt8_gate": ("tvts_gemm_nt_fp8_gate", _base_nt8_gate()),
    "nt8_gate_q8": ("tvts_gemm_nt_fp8_gate", _base_nt8_gate(q8out=Mat(5, 24, U8, "zero"), ldq8=24, q8_scale=Mat(1, 1, F32, 2.0 / 448.0),
                                                       q8_amax=Mat(1, 1, F32, "zero"))),
    "tn": ("tvts_gemm_tn_bf16", dict(P=Mat(5, 24, BF16), ldp=24, Q=Mat(5, 40, BF16), ldq=40, M=5, Na=16, Nb=32, out=Mat(16, 40, F32),
                                     ldo=40, accumulate=0, colsum=Mat(1, 16, F32), workspace=Mat(1, 4096, F32), workspace_elems=4096,
                                     counters=Mat(1, 64, I32, "zero"), n_counters=64, opts=0)),
    "tn8": ("tvts_gemm_tn_fp8", dict(P8=Mat(5, 32, U8), ldp=32, Q8=Mat(5, 48, U8), ldq=48, M=5, Na=16, Nb=32,
                                     scale_p=Mat(1, 1, F32, 0.01), scale_q=Mat(1, 1, F32, 0.02), out=Mat(16, 40, F32), ldo=40,
                                     accumulate=0, colsum=Mat(1, 16, F32), workspace=Mat(1, 4096, F32), workspace_elems=4096, opts=0)),
    "rows_linear": ("tvts_rows_linear_bf16", dict(A=Mat(3, 40, BF16), lda=40, W=Mat(16, 40, BF16), ldw=40, R=3, N=16, K=32,
                                                  bias=Mat(1, 16, F32), residual=Mat(3, 24, F32), ldr=24, out=Mat(3, 24, F32), ldo=24)),
    "colsum": ("tvts_colsum_bf16", dict(X=Mat(5, 24, BF16), ld=24, M=5, N=16, out=Mat(1, 16, F32), workspace=Mat(1, 4096, F32),
                                        workspace_elems=4096)),
}

# (baseline, the ONE argument changed, its value, why the call is refused).  "pin": refused before this table existed.
REFUSALS = [
    # ---- tvts_gemm_nt_bf16
    ("nt_res", "K", 32, "pin: K % 64"), ("nt_res", "N", 14, "pin: N % 4"), ("nt_res", "lda", 68, "pin: lda % 8"),
    ("nt_res", "ldb", 68, "pin: ldb % 8"), ("nt_res", "ldc", 22, "pin: ldc % 4"), ("nt_res", "ldr", 22, "pin: ldr % 4"),
    ("nt_res", "M", 0, "pin: M <= 0"), ("nt_res", "M", -1, "pin: M <= 0"), ("nt_res", "N", 0, "pin: N <= 0"), ("nt_res", "K", 0, "pin: K <= 0"),
    ("nt_res", "A", None, "null A"), ("nt_res", "B", None, "null B"), ("nt_res", "out", None, "null out"),
    ("nt_res", "lda", 56, "lda < K"), ("nt_res", "ldb", 56, "ldb < K"), ("nt_res", "ldc", 12, "ldc < N"), ("nt_res", "ldr", 12, "ldr < N"),
    ("nt_res", "ldr", 0, "ldr == 0 (a broadcast row: passes ldr % 4)"), ("nt_res", "workspace_bytes", -1, "workspace_bytes < 0"),
    ("nt_act", "ldp", 22, "pin: ldp % 4"), ("nt_act", "ldp", 12, "ldp < N"), ("nt_act", "act", 3, "pin: act is not an activation"),
    ("nt_gate", "act", 1, "pin: act together with a gate"), ("nt_gate", "ldh", 22, "pin: ldh % 4"), ("nt_gate", "ldh", 12, "ldh < N"),
    ("nt_gate", "gate_act", 0, "pin: gate_h without a gate"),
    ("nt_act_256", "ldc", 20, "pin: forced tile 256 with ldc % 8"), ("nt_act_256", "ldp", 20, "pin: forced tile 256 with ldp % 8"),
    ("nt_gate_256", "ldh", 20, "pin: forced tile 256 with ldh % 8"),
    ("nt_streamk", "ldc", 1020, "forced stream-K with ldc % 8 (only the 256 kernel has the walk)"),
    ("nt_streamk", "workspace", None, "pin: forced stream-K without a workspace"), ("nt_streamk", "K", 64, "pin: forced stream-K with one K stage"),
    # ---- tvts_gemm_nt_fp8
    ("nt8_res", "K", 64, "pin: K % 128"), ("nt8_res", "N", 12, "pin: N % 8"), ("nt8_res", "lda", 136, "pin: lda % 16"),
    ("nt8_res", "ldb", 136, "pin: ldb % 16"), ("nt8_res", "ldc", 20, "pin: ldc % 8"), ("nt8_res", "ldr", 22, "pin: ldr % 4"),
    ("nt8_res", "scale_a", None, "pin: no scale_a"), ("nt8_res", "scale_b", None, "pin: no scale_b"), ("nt8_res", "M", 0, "pin: M <= 0"),
    ("nt8_res", "N", 0, "pin: N <= 0"), ("nt8_res", "K", 0, "pin: K <= 0"), ("nt8_res", "out", None, "pin: neither out nor q8out"),
    ("nt8_res", "A", None, "null A"), ("nt8_res", "B", None, "null B"), ("nt8_res", "lda", 112, "lda < K"), ("nt8_res", "ldb", 112, "ldb < K"),
    ("nt8_res", "ldc", 8, "ldc < N"), ("nt8_res", "ldr", 12, "ldr < N"),
    ("nt8_act_q8", "ldp", 20, "pin: ldp % 8"), ("nt8_act_q8", "q8_scale", None, "pin: q8out without its scale"),
    ("nt8_act_q8", "ldq8", 20, "pin: ldq8 % 8"), ("nt8_act_q8", "ldp", 8, "ldp < N"), ("nt8_act_q8", "ldq8", 8, "ldq8 < N"),
    ("nt8_act_q8", "out_f32", 1, "pin: q8out of an fp32 result"),
    # ---- tvts_gemm_nt_fp8_gate
    ("nt8_gate", "gate_h", None, "pin: no gate_h"), ("nt8_gate", "ldh", 20, "pin: ldh % 8"), ("nt8_gate", "ldc", 20, "pin: ldc % 8"),
    ("nt8_gate", "K", 64, "pin: K % 128"), ("nt8_gate", "N", 12, "pin: N % 8"), ("nt8_gate", "scale_a", None, "pin: no scale_a"),
    ("nt8_gate", "scale_b", None, "pin: no scale_b"), ("nt8_gate", "M", 0, "pin: M <= 0"), ("nt8_gate", "out", None, "pin: neither out nor q8out"),
    ("nt8_gate", "A", None, "null A"), ("nt8_gate", "B", None, "null B"), ("nt8_gate", "lda", 112, "lda < K"), ("nt8_gate", "ldb", 112, "ldb < K"),
    ("nt8_gate", "ldh", 8, "ldh < N"), ("nt8_gate", "ldc", 8, "ldc < N"),
    ("nt8_gate_q8", "q8_scale", None, "pin: q8out without its scale"), ("nt8_gate_q8", "ldq8", 20, "pin: ldq8 % 8"), ("nt8_gate_q8", "ldq8", 8, "ldq8 < N"),
    # ---- tvts_gemm_tn_bf16
    ("tn", "Na", 12, "pin: Na % 8"), ("tn", "Nb", 28, "pin: Nb % 8"), ("tn", "ldp", 20, "pin: ldp % 8"), ("tn", "ldq", 36, "pin: ldq % 8"),
    ("tn", "ldo", 38, "pin: ldo % 4"), ("tn", "M", 0, "pin: M <= 0"), ("tn", "Na", 0, "pin: Na <= 0"), ("tn", "Nb", 0, "pin: Nb <= 0"),
    ("tn", "P", None, "null P"), ("tn", "Q", None, "null Q"), ("tn", "out", None, "null out"), ("tn", "ldp", 8, "ldp < Na"),
    ("tn", "ldq", 24, "ldq < Nb"), ("tn", "ldo", 28, "ldo < Nb"), ("tn", "workspace_elems", -1, "workspace_elems < 0"),
    # ---- tvts_gemm_tn_fp8
    ("tn8", "Na", 8, "pin: Na % 16"), ("tn8", "Nb", 24, "pin: Nb % 16"), ("tn8", "ldp", 24, "pin: ldp % 16"), ("tn8", "ldq", 40, "pin: ldq % 16"),
    ("tn8", "ldo", 38, "pin: ldo % 4"), ("tn8", "scale_p", None, "pin: no scale_p"), ("tn8", "scale_q", None, "pin: no scale_q"),
    ("tn8", "M", 0, "pin: M <= 0"), ("tn8", "P8", None, "null P8"), ("tn8", "Q8", None, "null Q8"), ("tn8", "out", None, "null out"),
    ("tn8", "ldp", 0, "ldp < Na"), ("tn8", "ldq", 16, "ldq < Nb"), ("tn8", "ldo", 28, "ldo < Nb"), ("tn8", "workspace_elems", -1, "workspace_elems < 0"),
    # ---- tvts_rows_linear_bf16
    ("rows_linear", "N", 8, "pin: N % 16"), ("rows_linear", "K", 16, "pin: K % 32"), ("rows_linear", "lda", 36, "pin: lda % 8"),
    ("rows_linear", "ldw", 36, "pin: ldw % 8"), ("rows_linear", "R", 0, "pin: R <= 0"), ("rows_linear", "A", None, "pin: null A"),
    ("rows_linear", "W", None, "pin: null W"), ("rows_linear", "out", None, "pin: null out"), ("rows_linear", "lda", 24, "lda < K"),
    ("rows_linear", "ldw", 24, "ldw < K"), ("rows_linear", "ldo", 12, "ldo < N"), ("rows_linear", "ldr", 12, "ldr < N"),
    # ---- tvts_colsum_bf16
    ("colsum", "N", 12, "pin: N % 8"), ("colsum", "ld", 20, "pin: ld % 8"), ("colsum", "M", 0, "pin: M <= 0"), ("colsum", "N", 0, "pin: N <= 0"),
    ("colsum", "X", None, "null X"), ("colsum", "out", None, "null out"), ("colsum", "ld", 8, "ld < N"),
    ("colsum", "workspace_elems", -1, "workspace_elems < 0"),
]


def call(lib, protos, name, alloc, stream=None, **change):
    """the baseline `name` with the arguments of `change` replaced -> the entry point's return code.  alloc(Mat) -> a pointer;
    NT_WS arguments come from alloc(NT_WS) -> (pointer, bytes)"""
    fn, base = BASELINES[name]
    args = dict(base)
    bad = set(change) - set(args)
    assert not bad, (name, bad)
    ws = alloc(NT_WS) if NT_WS in base.values() else None
    args.update(change)
    vals = []
    for an in protos[fn][2]:
        if an == "stream":
            vals.append(stream)
            continue
        v = args[an]
        if isinstance(v, Mat):
            v = alloc(v)
        elif isinstance(v, str) and v == NT_WS:
            v = ws[0] if an == "workspace" else ws[1]
        vals.append(v)
    return getattr(lib, fn)(*vals)
