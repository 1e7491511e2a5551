"""Per-element and per-row checks of kernel outputs against float64 references (a plain helper module, imported by the tests).

A whole-tensor norm ``rel(got, ref) = |got - ref| / |ref|`` over 10^8 elements does not see an error that sits in a few hundred of
them: one wrong row of a 150 720 x 768 product, one transposed 16 x 16 block or 16 zeroed values of one row all stay inside the
4e-3 gate of a bf16 output (tests/test_kernel_bounds_cpu.py shows it).  The checks below look at every element (GEMMs, exact
copies) or at every (row, head) slice (softmax attention, LayerNorm row reductions) and name the element and the tile it belongs to.

References are float64 torch on the device of the inputs, built from the exact values the kernel read (bf16 operands, decoded
e4m3 bytes times their scales), in row chunks so that a 150 720 x 3072 reference stays within a few GB.
"""
import math

import torch

U32 = 2.0 ** -24          # unit roundoff of fp32
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}  # unit roundoff of the output type: |fl(v) - v| <= u |v| (RNE)
SIG_BITS = {torch.bfloat16: 8, torch.float32: 24}
# Transcendental error of the kernels' activation epilogues (fast exp2 / rcp, erf by Abramowitz & Stegun 7.1.26 with
# |error| <= 1.5e-7): bounded by EPS_ACT * (|x| + |act(x)|) for act and EPS_ACT * (1 + 2|x| + |act'(x)|) for act'.
EPS_ACT = 2.0 ** -20
LIP_ACT = 1.13            # max |act'(x)| of QuickGELU (1.0998) and erf-GELU (1.1289): the Lipschitz constant of both
LIP_DERIV = 0.86          # max |act''(x)| (QuickGELU 0.851, erf-GELU 0.798): the Lipschitz constant of act'
TILE, SLAB, COLS = 256, 16, 16


# ------------------------------------------------------------------------------------------------ reporting
ACC_WORST = [0.0]  # worst accumulation-part ratio of the checks since the last pop_acc_worst()


def pop_acc_worst():
    v, ACC_WORST[0] = ACC_WORST[0], 0.0
    return v


class Report:
    """Violations of |got - ref| <= bound, merged over row chunks; ``raise_if_bad`` names the first offender and its tile."""

    def __init__(self, what):
        self.what, self.count, self.first, self.worst, self.nonfinite, self.n = what, 0, None, 0.0, 0, 0
        self.worst_acc = 0.0

    def add(self, got, ref, bound, row0=0, out_dtype=None):
        """out_dtype (the type the kernel rounded to; bound = u_out |ref| + acc): also measure how much of the pre-rounding part
        acc is used, max(0, |err| - half ulp(got)) / acc -- the output rounding alone takes up to u_out |ref| of every bound, so the
        total ratio of a correctly rounded result reaches ~1 by construction; this one shows the headroom of the accumulation"""
        got = got.double() if got.dtype != torch.float64 else got
        ref = ref.double() if ref.dtype != torch.float64 else ref
        bound = bound.double() if torch.is_tensor(bound) else torch.tensor(float(bound), dtype=torch.float64, device=ref.device)
        got2, ref2 = got.reshape(got.shape[0], -1) if got.dim() > 1 else got[:, None], ref.reshape(got.shape[0], -1) if ref.dim() > 1 else ref[:, None]
        b2 = bound.expand(ref.shape).reshape(got2.shape) if bound.dim() > 0 else bound
        err = (got2 - ref2).abs()
        finite = torch.isfinite(got2)
        bad = (~finite) | (err > b2)
        self.n += got2.numel()
        nb = int(bad.sum())
        if nb:
            self.count += nb
            self.nonfinite += int((~finite).sum())
            if self.first is None:
                idx = int(torch.nonzero(bad.reshape(-1))[0])
                r, c = divmod(idx, got2.shape[1])
                self.first = (row0 + r, c, float(got2[r, c]), float(ref2[r, c]),
                              float(b2[r, c] if b2.dim() > 0 else b2))
        ratio = torch.where(finite, err / b2.clamp_min(1e-300), torch.zeros_like(err))
        self.worst = max(self.worst, float(ratio.max()) if ratio.numel() else 0.0)
        if out_dtype is not None and got2.numel():
            ag = got2.abs()
            half = torch.where(ag > 0, torch.exp2(torch.floor(torch.log2(ag.clamp_min(1e-300))) - SIG_BITS[out_dtype]), torch.zeros_like(ag))
            acc = (b2 - U_OUT[out_dtype] * ref2.abs()).clamp_min(1e-300)
            ex = torch.where(finite, (err - half).clamp_min(0.0) / acc, torch.zeros_like(err))
            self.worst_acc = max(self.worst_acc, float(ex.max()))
        return self

    def raise_if_bad(self):
        if not self.count:
            ACC_WORST[0] = max(ACC_WORST[0], self.worst_acc)
        if self.count:
            r, c, g, ref, b = self.first
            raise AssertionError(
                f"{self.what}: {self.count} of {self.n} elements outside the bound ({self.nonfinite} non-finite); first at "
                f"(row {r}, col {c}) got {g!r} ref {ref!r} bound {b:.3g}: 256x256 tile ({r // TILE}, {c // TILE}), 16-row slab "
                f"{(r % TILE) // SLAB} of that tile (global slab {r // SLAB}), column group {c // COLS} (16 columns); worst "
                f"|err| / bound = {self.worst:.3g}")
        return self.worst


def assert_within(got, ref, bound, what="output"):
    """|got - ref| <= bound element by element (bound: tensor broadcastable to ref, or a number); any non-finite value fails.
    Returns the worst |err| / bound (the headroom a test reports)."""
    return Report(what).add(got, ref, bound).raise_if_bad()


def assert_equal_bits(got, want, what="output"):
    """bit-for-bit equality (NaNs included) with the first differing element named like assert_within does"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ib = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    g, w = got.contiguous().view(ib), want.contiguous().view(ib)
    diff = g != w
    n = int(diff.sum())
    if n:
        d2 = diff.reshape(diff.shape[0], -1) if diff.dim() > 1 else diff[:, None]
        r, c = divmod(int(torch.nonzero(d2.reshape(-1))[0]), d2.shape[1])
        gv, wv = got.reshape(d2.shape)[r, c], want.reshape(d2.shape)[r, c]
        raise AssertionError(f"{what}: {n} of {diff.numel()} elements differ; first at (row {r}, col {c}) got {gv.item()!r} "
                             f"want {wv.item()!r}: 256x256 tile ({r // TILE}, {c // TILE}), 16-row slab {(r % TILE) // SLAB}, "
                             f"column group {c // COLS}")


def rows_rel(got, ref, groups=1, floor=0.05, out_dtype=None):
    """relative L2 error of every (row, group) slice: got / ref [R, C] with C = groups * d (1-D: every element its own slice).
    The denominator is max(|ref slice|, floor * mean |ref slice|) so that a slice whose reference is ~0 (a head of one row that
    happens to cancel) does not divide by noise.  out_dtype: the type the kernel rounded its result to -- each element's error is
    first reduced by half an ulp of got in that type (max(0, |err| - half ulp)), so that the tolerance measures the kernel's error
    before its output rounding instead of the rounding noise every correct result carries."""
    got, ref = got.double(), ref.double()
    if got.dim() == 1:
        got, ref = got[:, None], ref[:, None]
    R = got.shape[0]
    err = (got - ref).abs()
    if out_dtype is not None:
        ag = got.abs()
        half = torch.where(ag > 0, torch.exp2(torch.floor(torch.log2(ag.clamp_min(1e-300))) - SIG_BITS[out_dtype]), torch.zeros_like(ag))
        err = (err - half).clamp_min(0.0)
    g = err.reshape(R, groups, -1)
    r = ref.reshape(R, groups, -1)
    num, den = g.norm(dim=2), r.norm(dim=2)
    return num / torch.maximum(den, floor * den.mean().clamp_min(1e-300)), torch.isfinite(got).all()


def assert_rows_within(got, ref, tol, groups=1, what="rows", floor=0.05, out_dtype=None):
    """every (row, group) slice within tol relative L2 (rows_rel); returns the worst slice error"""
    e, finite = rows_rel(got, ref, groups, floor, out_dtype)
    worst = float(e.max())
    bad = e > tol
    if not bool(finite) or bool(bad.any()):
        nb = int(bad.sum())
        first = torch.nonzero(bad)[0].tolist() if nb else None
        raise AssertionError(f"{what}: {nb} of {e.numel()} (row, group) slices above tol {tol:g} (all finite: {bool(finite)}); "
                             f"first (row, group) = {first}; worst {worst:.3g}")
    return worst


# ------------------------------------------------------------------------------------------------ guarded outputs
def guarded(M, N, dtype, device, rows=3, cols=8):
    """an [M, N] output view with `rows` guard rows under it and `cols` guard columns right of it (leading dimension N + cols),
    filled with NaN (0xFF bytes for integer types); -> (buffer, view)"""
    if dtype.is_floating_point:
        buf = torch.full((M + rows, N + cols), float("nan"), dtype=dtype, device=device)
    else:
        buf = torch.full((M + rows, N + cols), 0xFF, dtype=torch.uint8, device=device).view(dtype)
    return buf, buf[:M, :N]


def check_guards(buf, M, N, what="output"):
    """the guard rows and columns of `guarded` are untouched"""
    def untouched(t):
        return bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t.view(torch.uint8) == 0xFF).all())
    assert untouched(buf[M:]), f"{what}: rows past {M} were written"
    assert untouched(buf[:M, N:]), f"{what}: columns past {N} were written (leading dimension {buf.shape[1]})"


# ------------------------------------------------------------------------------------------------ GEMM references and bounds
def decode_e4m3(q8):
    """uint8 e4m3 (OCP, fn) bytes -> float64 values"""
    return q8.view(torch.float8_e4m3fn).double()


def gemm_ref(a, b, r0=0, r1=None, *, scale=None, bias=None, residual=None):
    """rows r0:r1 of ref = scale * (a @ b^T) + bias + residual and of S = |scale| * (|a| @ |b|^T) + |bias| + |residual|, float64.
    a [M, K], b [N, K] in any float type (decoded values); scale: None, a number, or float64 [M] (one per row)."""
    r1 = a.shape[0] if r1 is None else r1
    ac, bd = a[r0:r1].double(), b.double()
    ref, S = ac @ bd.t(), ac.abs() @ bd.abs().t()
    if scale is not None:
        s = scale[r0:r1, None] if torch.is_tensor(scale) and scale.numel() > 1 else scale
        ref, S = ref * s, S * (s.abs() if torch.is_tensor(s) else abs(s))
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    if residual is not None:
        rr = residual[r0:r1].double()
        ref, S = ref + rr, S + rr.abs()
    return ref, S


def gemm_acc_bound(S, K, c=4):
    """bound on |v - ref| of the fp32 value v the kernel holds before its output rounding: (K + c) u S / (1 - (K + c) u)"""
    n = (K + c) * U32
    return S * (n / (1.0 - n))


def gemm_bound(ref, S, K, out_dtype, c=4, acc=None):
    """Per-element bound for an MFMA product with fp32 accumulation, valid for ANY summation order.

    Derivation.  The kernel forms v_ij = fl(sum of the K products a_ik b_jk, the bias and the residual) in fp32.  bf16 x bf16 and
    e4m3 x e4m3 products are exact in fp32 (8 + 8 and 4 + 4 significand bits), so every rounding is one of the additions (and, for
    fp8, the one or two multiplications by the scales).  Whatever the order -- a tile kernel's MFMA chain, split-K partials
    reduced afterwards, stream-K, fp32 atomics -- the sum is a binary tree of n = K + c - 1 roundings, and the standard result
    for recursive summation (Higham, Accuracy and Stability, Thm 4.3 / eq. 4.4) gives

        |v_ij - ref_ij| <= gamma_n * S_ij,   gamma_n = n u / (1 - n u),   S_ij = sum_k |a_ik||b_jk| + |bias_j| (+ |res_ij|),

    u = 2^-24.  Each scale multiplication is one more relative rounding of a partial whose magnitude is <= S, so it is covered
    by c (default 4: bias, residual, two scale factors).  For fp8, S is taken over the decoded values times |sa sb|.  The
    result is then rounded to nearest even in the output type: |out - v| <= u_out |v| (u_out = 2^-8 for bf16, 2^-24 for
    fp32), and |v| <= |ref| + acc, so

        |out_ij - ref_ij| <= u_out |ref_ij| + (1 + u_out) gamma_n S_ij.

    A value just above a power of two can use the whole rounding term, so the total |err| / bound of a correct bf16 result
    reaches ~1; Report measures the used share of the accumulation term separately (worst_acc).

    No order-dependent term appears, so one bound serves every kernel form.  `acc`: the pre-rounding bound when it is not the
    plain gamma_n S (activations and gates: act_bound / gate_bound)."""
    acc = gemm_acc_bound(S, K, c) if acc is None else acc
    u = U_OUT[out_dtype]
    return u * ref.abs() + (1.0 + u) * acc + 1e-38


def act_ref(x, act):
    """float64 QuickGELU / erf-GELU"""
    if act == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def act_deriv_ref(x, act):
    if act == "quick_gelu":
        s = torch.sigmoid(1.702 * x)
        return s * (1.0 + 1.702 * x * (1.0 - s))
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def act_bound(pre_ref, pre_acc, act, out_dtype):
    """y = act(v) with |v - pre_ref| <= pre_acc: |act(v) - act(pre_ref)| <= L pre_acc (L = LIP_ACT), plus the kernel's
    transcendental error EPS_ACT (|x| + |act(x)|) (x within pre_acc of pre_ref: |x| <= |pre_ref| + pre_acc), then the output
    rounding as in gemm_bound.  -> (ref, bound)"""
    y = act_ref(pre_ref, act)
    acc = LIP_ACT * pre_acc + EPS_ACT * (pre_ref.abs() + pre_acc + y.abs() + LIP_ACT * pre_acc)
    acc = acc * (1 + 2 * U32)  # the multiply inside act and the fp32 rounding of y
    u = U_OUT[out_dtype]
    return y, u * y.abs() + (1.0 + u) * acc + 1e-38


def gate_bound(z_ref, z_acc, h, act, out_dtype, deriv=False):
    """out = z * g(h), h the exact (bf16) gate input, g = act' (or, deriv, g = h itself: the stored derivative).
    |z g~ - z_ref g| <= |g| z_acc + |z_ref| eps_g + z_acc eps_g, eps_g = EPS_ACT (1 + 2|h| + |g|) (0 for deriv), plus the fp32
    rounding of the product and the output rounding.  -> (ref, bound)"""
    h = h.double()
    g = h if deriv else act_deriv_ref(h, act)
    eps_g = torch.zeros_like(g) if deriv else EPS_ACT * (1.0 + 2.0 * h.abs() + g.abs())
    ref = z_ref * g
    acc = g.abs() * z_acc + z_ref.abs() * eps_g + z_acc * eps_g
    acc = acc + U32 * (ref.abs() + acc)
    u = U_OUT[out_dtype]
    return ref, u * ref.abs() + (1.0 + u) * acc + 1e-38


def check_gemm(got, a, b, *, what, scale=None, bias=None, residual=None, act=None, preact=None, gate_h=None, gate_act=None,
               deriv=False, add_bf16=None, K=None, c=4, chunk=8192):
    """got[M, N] against the float64 product of a [M, K] and b [N, K] (decoded values), every element within gemm_bound /
    act_bound / gate_bound; preact (the side output of an activation epilogue, bf16) is checked against the pre-activation, or
    (deriv) against act' of it.  add_bf16: the bf16 residual stream added in the gate slot.  Returns the worst |err| / bound
    over all the outputs checked."""
    K = a.shape[1] if K is None else K
    M = got.shape[0]
    reps = [Report(what)] + ([Report(what + " (pre-activation side output)")] if preact is not None else [])
    for r0 in range(0, M, chunk):
        r1 = min(M, r0 + chunk)
        ref, S = gemm_ref(a, b, r0, r1, scale=scale, bias=bias, residual=residual)
        acc = gemm_acc_bound(S, K, c)
        if act is not None:
            y, bnd = act_bound(ref, acc, act, got.dtype)
            reps[0].add(got[r0:r1], y, bnd, r0, got.dtype)
            if preact is not None:
                if deriv:
                    d, dbnd = _deriv_bound(ref, acc, act)
                    reps[1].add(preact[r0:r1], d, dbnd, r0, preact.dtype)
                else:
                    reps[1].add(preact[r0:r1], ref, gemm_bound(ref, S, K, preact.dtype, acc=acc), r0, preact.dtype)
        elif gate_h is not None:
            y, bnd = gate_bound(ref, acc, gate_h[r0:r1], gate_act, got.dtype, deriv=deriv)
            reps[0].add(got[r0:r1], y, bnd, r0, got.dtype)
        elif add_bf16 is not None:
            hr = add_bf16[r0:r1].double()
            ref2 = ref + hr
            acc2 = acc + U32 * (ref2.abs() + acc)
            reps[0].add(got[r0:r1], ref2, gemm_bound(ref2, S + hr.abs(), K, got.dtype, acc=acc2), r0, got.dtype)
        else:
            reps[0].add(got[r0:r1], ref, gemm_bound(ref, S, K, got.dtype, c=c), r0, got.dtype)
        del ref, S, acc
    return max(r.raise_if_bad() for r in reps)


def _deriv_bound(pre_ref, pre_acc, act):
    """the bf16 side output act'(v) of a side_deriv forward: |act''| <= LIP_DERIV over the reals (QuickGELU 0.851 at 0, erf-GELU
    2 phi(0) = 0.798), plus EPS_ACT (1 + 2|x| + |act'|), then the bf16 rounding"""
    d = act_deriv_ref(pre_ref, act)
    acc = LIP_DERIV * pre_acc + EPS_ACT * (1.0 + 2.0 * (pre_ref.abs() + pre_acc) + d.abs() + LIP_DERIV * pre_acc)
    u = U_OUT[torch.bfloat16]
    return d, u * d.abs() + (1.0 + u) * acc + 1e-38


# ------------------------------------------------------------------------------------------------ LayerNorm references and bounds
def _gamma(n):
    return n * U32 / (1.0 - n * U32)


def ln_fwd_check(x, gamma, beta, eps, y=None, mean=None, rstd=None, *, what, chunk=16384):
    """LayerNorm forward outputs against float64, per element.  x is what the kernel read (fp32, or bf16 widened).

    Bound.  The kernel forms m = fl(sum x / W) and the variance in fp32 in some order (two-pass or E[x^2] - m^2):
    |m - mean| <= gamma_W s1 with s1 = mean |x|; the variance is off by at most gamma_{W+4} (s2 + 2 s1^2) (s2 = mean x^2), so
    rstd carries a relative error e_r <= gamma_{W+4} (s2 + 2 s1^2) / (var + eps) + 4u (the square root and its reciprocal).
    y = (x - m) rstd g + b then errs by |g| rstd (|m - mean| + |x - mean| e_r) + 4u (|xhat g| + |b|), then the output rounding."""
    W = x.shape[1]
    reps = {k: Report(f"{what}: {k}") for k, t in (("y", y), ("mean", mean), ("rstd", rstd)) if t is not None}
    g64, b64 = gamma.double(), beta.double()
    for r0 in range(0, x.shape[0], chunk):
        r1 = min(x.shape[0], r0 + chunk)
        xc = x[r0:r1].double()
        mu = xc.mean(1, keepdim=True)
        var = ((xc - mu) ** 2).mean(1, keepdim=True)
        rs = 1.0 / torch.sqrt(var + eps)
        s1, s2 = xc.abs().mean(1, keepdim=True), (xc * xc).mean(1, keepdim=True)
        e_m = _gamma(W + 1) * s1
        e_r = _gamma(W + 4) * (s2 + 2 * s1 * s1) / (var + eps) + 4 * U32
        xh = (xc - mu) * rs
        if y is not None:
            ref = xh * g64 + b64
            acc = g64.abs() * rs * (e_m + (xc - mu).abs() * e_r) + 4 * U32 * ((xh * g64).abs() + b64.abs())
            u = U_OUT[y.dtype]
            reps["y"].add(y[r0:r1], ref, u * ref.abs() + (1 + u) * acc + 1e-38, r0, y.dtype)
        if mean is not None:
            reps["mean"].add(mean[r0:r1], mu[:, 0], (e_m + U32 * mu.abs())[:, 0] + 1e-38, r0)
        if rstd is not None:
            reps["rstd"].add(rstd[r0:r1], rs[:, 0], (rs * e_r * 1.01)[:, 0], r0)
    return max(r.raise_if_bad() for r in reps.values())


def ln_bwd_check(dy, x, mean, rstd, gamma, *, dx=None, dx_bf16=None, res1=None, res2=None, dgamma=None, dbeta=None,
                 dgamma0=None, dbeta0=None, col_tol=None, col_worst=None, what, chunk=16384):
    """LayerNorm backward outputs against float64 evaluated on the SAME mean / rstd the kernel read, per element (dx) and per
    column (dgamma, dbeta).

    Bound.  xhat = (x - mean) rstd is formed with |err| <= e_x = 3u (|xhat| + |x| rstd); with gd = g dy, the row means
    c1 = mean gd and c2 = mean gd xhat carry |err| <= gamma_W mean |gd| and gamma_{W+3} mean |gd xhat| + mean(|gd| e_x);
    dx = rstd (gd - c1 - xhat c2) + res1 + res2 then errs by rstd (u |gd| + e_c1 + |xhat| e_c2 + e_x |c2|) + 6u (|terms|).
    dgamma / dbeta (sums over all M rows, accumulated into dgamma0 / dbeta0): a worst-case gamma_M bound is larger than the sums
    themselves at M = 150 720, so every column is held to the calibrated relative tolerance col_tol (assert_rows_within); the
    worst column error goes into col_worst[name]."""
    M, W = x.shape
    g64 = gamma.double()
    reps = {}
    colsum = {k: torch.zeros(W, dtype=torch.float64, device=x.device) for k in ("dg", "db")}
    col_worst = {} if col_worst is None else col_worst
    for k, t in (("dx", dx), ("dx_bf16", dx_bf16)):
        if t is not None:
            reps[k] = Report(f"{what}: {k}")
    for r0 in range(0, M, chunk):
        r1 = min(M, r0 + chunk)
        xc, dyc = x[r0:r1].double(), dy[r0:r1].double()
        mu, rs = mean[r0:r1].double()[:, None], rstd[r0:r1].double()[:, None]
        xh = (xc - mu) * rs
        e_x = 3 * U32 * (xh.abs() + xc.abs() * rs)
        gd = g64 * dyc
        c1 = gd.mean(1, keepdim=True)
        c2 = (gd * xh).mean(1, keepdim=True)
        e_c1 = _gamma(W + 1) * gd.abs().mean(1, keepdim=True)
        e_c2 = _gamma(W + 4) * (gd * xh).abs().mean(1, keepdim=True) + (gd.abs() * e_x).mean(1, keepdim=True)
        core = rs * (gd - c1 - xh * c2)
        terms = rs * (gd.abs() + c1.abs() + (xh * c2).abs())
        ref = core
        acc = rs * (U32 * gd.abs() + e_c1 + xh.abs() * e_c2 + e_x * c2.abs()) + 6 * U32 * terms
        for r in (res1, res2):
            if r is not None:
                rr = r[r0:r1].double()
                ref = ref + rr
                acc = acc + 2 * U32 * (rr.abs() + ref.abs())
        for k, t in (("dx", dx), ("dx_bf16", dx_bf16)):
            if t is not None:
                u = U_OUT[t.dtype]
                reps[k].add(t[r0:r1], ref, u * ref.abs() + (1 + u) * acc + 1e-38, r0, t.dtype)
        colsum["dg"] += (dyc * xh).sum(0)
        colsum["db"] += dyc.sum(0)
    worst = max([r.raise_if_bad() for r in reps.values()] + [0.0])
    for name, got, init, ref in (("dgamma", dgamma, dgamma0, colsum["dg"]), ("dbeta", dbeta, dbeta0, colsum["db"])):
        if got is not None:
            ref = ref + (init.double() if init is not None else 0.0)
            col_worst[name] = assert_rows_within(got, ref, col_tol, what=f"{what}: {name} (per column)")
    return worst


def ln_cols_check(dy, x, mean, rstd, dgamma, dbeta, dgamma0, dbeta0, *, what):
    """dgamma / dbeta of a LayerNorm backward over a FEW THOUSAND rows at most, every column within a derived summation bound
    (ln_bwd_check's col_tol is calibrated for 150 720 rows, where a worst-case bound exceeds the sums themselves).

    dbeta[c] = dbeta0[c] + sum_r dy[r, c]: the addends are exact, so sum_bound with n = M addends in any order (a wave's running
    sum, four waves through LDS, per-block partials or atomics, the reduce kernel's groups, `+=`).
    dgamma[c] = dgamma0[c] + sum_r dy[r, c] xhat[r, c]: each addend is fl(dy fl(xhat)) with xhat formed as in ln_bwd_check
    (|err| <= e_x = 3u (|xhat| + |x| rstd)), i.e. off by at most |dy| e_x + u |dy xhat| before it is summed:

        |got - ref| <= gamma_{M+8} (sum |dy xhat| + |dgamma0|) + (1 + gamma_{M+8}) sum |dy| e_x.

    -> {"dgamma": worst |err| / bound, "dbeta": ...}"""
    M = x.shape[0]
    xc, dyc = x.double(), dy.double()
    mu, rs = mean[:M].double()[:, None], rstd[:M].double()[:, None]
    xh = (xc - mu) * rs
    e_x = 3 * U32 * (xh.abs() + xc.abs() * rs)
    gk = _gamma(M + 8)
    ref_g = (dyc * xh).sum(0) + dgamma0.double()
    bound_g = gk * ((dyc * xh).abs().sum(0) + dgamma0.double().abs()) + (1 + gk) * (dyc.abs() * e_x).sum(0) + 1e-45
    ref_b = dyc.sum(0) + dbeta0.double()
    bound_b = sum_bound(dyc.abs().sum(0), M, init=dbeta0)
    return {"dgamma": assert_within(dgamma, ref_g, bound_g, f"{what}: dgamma (per column)"),
            "dbeta": assert_within(dbeta, ref_b, bound_b, f"{what}: dbeta (per column)")}


# ------------------------------------------------------------------------------------------------ attention references
# per (row, head) relative L2 of the error beyond the bf16 rounding of each output value (rows_rel with out_dtype), calibrated on
# the MI355X.  Worst measured over the short-sequence and divided tests: out 2.25e-3, dq 3.81e-3, dk 3.24e-3, dv 3.15e-3; each tol
# >= 3x that and under the whole-tensor gates (8e-3 forward, 2e-2 backward).  The streaming FULL, kv_len, dropout, tail, one-row and
# split divided kernels of tests/test_attention_rows_gpu.py, against float64 on the output and lse2 they read, stay under the same
# table without a case of their own: worst out 2.58e-3 (kv_len dropout), dq 3.22e-3 (split, B/16 time), dk 3.03e-3, dv 2.87e-3
# (profiles/r09_attention_rows_bounds.txt), and so do the fused divided site kernels at every tile class and launch layout of
# tests/test_attention_fused_rows_gpu.py: worst out 2.09e-3, dq 3.24e-3, dk 3.00e-3, dv 3.01e-3, lse2 1.6e-5 absolute
# (profiles/r26_attention_fused_rows_bounds.txt); the bf16 roundings of P and dS alone give 2.9e-3 .. 4.2e-3 in float64
# (tests/test_kernel_bounds_cpu.py::test_bf16_rounding_emulation_sits_inside_the_attention_tolerances)
ATTN_ROW_TOL = {"out": 7e-3, "dq": 1.2e-2, "dk": 1.2e-2, "dv": 1.2e-2}
LSE2_TOL = 1e-3           # absolute, log2 domain: the gate test_short_sequence_attention holds between two kernels
# the divided geometries of the step (tests/test_kernels_gpu.py, tests/test_attention_rows_gpu.py)
DIVIDED = {"B16": dict(B=24, T=8, n=98, heads=12, dh=64), "H14": dict(B=2, T=16, n=76, heads=16, dh=80)}
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)


def bound_line(name, v):
    """print the worst |err| / bound and the worst used share of the bounds' accumulation terms (Report.worst_acc)"""
    print(f"BOUND {name} {v:.4g} acc {pop_acc_worst():.4g}")
    return v


def rows_check(got, ref, tol, heads, B, S, what):
    """every (row, head) slice, and the CLS rows (row 0 of every clip: the cross-group merges / sums) on their own"""
    w = assert_rows_within(got, ref, tol, groups=heads, what=what, out_dtype=torch.bfloat16)
    cls = torch.arange(B, device=got.device) * S
    wc = assert_rows_within(got[cls], ref[cls], tol, groups=heads, what=what + " (CLS rows)", out_dtype=torch.bfloat16)
    return w, wc


def _heads_of(x, heads, dh):
    """[B, S, heads * dh] -> float64 [B, heads, S, dh]"""
    B, S, _ = x.shape
    return x.double().reshape(B, S, heads, dh).permute(0, 2, 1, 3)


def _merged(x):
    """[B, heads, S, dh] -> [B, S, heads * dh]"""
    B, h, S, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, S, h * dh)


def attn_allowed(B, S, device, *, causal=False, kv_len=None, allowed=None):
    """bool [B, 1, S, S]: query row q of sequence b attends key k.  causal: k <= q; kv_len (int [B]): k < clamp(kv_len[b], 1, S);
    allowed: a bool [S, S] relation of its own (the divided geometries: divided_allowed)"""
    ok = torch.ones(B, 1, S, S, dtype=torch.bool, device=device)
    if causal:
        ok = ok & torch.ones(S, S, dtype=torch.bool, device=device).tril()
    if kv_len is not None:
        L = kv_len.to(device).long().clamp(1, S)
        ok = ok & (torch.arange(S, device=device)[None, :] < L[:, None])[:, None, None, :]
    if allowed is not None:
        ok = ok & allowed.to(device)
    return ok


def _drop_factor(drop_mask, p, like):
    """the factor dropout puts on the probabilities: 1 / (1 - p) where drop_mask is nonzero (kept), 0 where it is zero"""
    if drop_mask is None:
        return None
    return (drop_mask.to(like.device) != 0).to(like.dtype) / (1.0 - p)


def _bf16r(t):
    return t.bfloat16().double()


def attn_fwd_ref(qkv, heads, dh, *, causal=False, kv_len=None, drop_mask=None, p=0.0, allowed=None, emulate=False):
    """softmax attention of a packed [B, S, 3W] (q | k | v) tensor in float64 -> (out [B, S, W], lse2 [B, S, heads],
    P [B, heads, S, S]).  lse2: log2-domain log-sum-exp of the UNdropped scores, scale dh**-0.5 * log2(e); masked keys have
    probability 0; dropout multiplies the probabilities after the softmax (drop_mask [B, heads, S, S]: nonzero = kept).
    Differentiable (attn_autograd).  emulate: P rounded to bf16 before P.V, the one rounding the algorithm cannot avoid."""
    B, S, W3 = qkv.shape
    W = W3 // 3
    q, k, v = (_heads_of(qkv[..., i * W:(i + 1) * W], heads, dh) for i in range(3))
    ok = attn_allowed(B, S, qkv.device, causal=causal, kv_len=kv_len, allowed=allowed)
    s2 = (q @ k.transpose(-1, -2)) * (dh ** -0.5 * LOG2E)
    s2 = s2.masked_fill(~ok, float("-inf"))
    lse2 = torch.logsumexp(s2 * LN2, -1) / LN2
    P = torch.exp2(s2 - lse2[..., None])
    f = _drop_factor(drop_mask, p, P)
    Pd = P if f is None else P * f
    if emulate:
        Pd = _bf16r(Pd)
    return _merged(Pd @ v), lse2.permute(0, 2, 1), P


def attn_autograd(qkv, dO, heads, dh, **kw):
    """float64 autograd of attn_fwd_ref -> (out, dqkv)"""
    x = qkv.double().clone().requires_grad_(True)
    out, _, _ = attn_fwd_ref(x, heads, dh, **kw)
    out.backward(dO.double())
    return out.detach(), x.grad


def attn_bwd_same_inputs(qkv, dO, O_read, lse2_read, heads, dh, *, causal=False, kv_len=None, drop_mask=None, p=0.0, q_rows=None,
                         allowed=None, emulate=False):
    """dqkv [B, S, 3W] in float64 from the values a backward kernel READS: the packed qkv, dO, the saved output O_read (bf16,
    widened) and the saved log-sum-exp lse2_read [B, S, heads] -- the way ln_bwd_check holds the LayerNorm backward to the
    mean / rstd it read.  P = exp2(scale2 s - lse2_read) (0 where masked), delta = rowsum(dO o O_read), dV = P_drop^T dO,
    dP = (dO V^T) mask / (1 - p), dS = P o (dP - delta), dQ = scale dS K, dK = scale dS^T Q.
    q_rows (bool [B, S]): the query rows that exist (tail / one-row forms); every other row contributes nothing, whatever
    dO / O_read / lse2_read hold there (NaN included).  emulate: P_drop and dS rounded to bf16 before their products."""
    B, S, W3 = qkv.shape
    W = W3 // 3
    q, k, v = (_heads_of(qkv[..., i * W:(i + 1) * W], heads, dh) for i in range(3))
    ok = attn_allowed(B, S, qkv.device, causal=causal, kv_len=kv_len, allowed=allowed)
    dOh, Oh = _heads_of(dO, heads, dh), _heads_of(O_read, heads, dh)
    lse = lse2_read.double().permute(0, 2, 1)
    if q_rows is not None:
        qr = q_rows.to(qkv.device)[:, None, :]
        ok = ok & qr[..., None]
        dOh, Oh = torch.where(qr[..., None], dOh, torch.zeros_like(dOh)), torch.where(qr[..., None], Oh, torch.zeros_like(Oh))
        lse = torch.where(qr, lse, torch.zeros_like(lse))
    scale = dh ** -0.5
    s2 = (q @ k.transpose(-1, -2)) * (scale * LOG2E)
    P = torch.where(ok, torch.exp2(s2 - lse[..., None]), torch.zeros_like(s2))
    f = _drop_factor(drop_mask, p, P)
    delta = (dOh * Oh).sum(-1)
    Pd = P if f is None else P * f
    dP = dOh @ v.transpose(-1, -2)
    if f is not None:
        dP = dP * f
    dS = P * (dP - delta[..., None])
    if emulate:
        Pd, dS = _bf16r(Pd), _bf16r(dS)
    dV = Pd.transpose(-1, -2) @ dOh
    dQ = scale * (dS @ k)
    dK = scale * (dS.transpose(-1, -2) @ q)
    return torch.cat([_merged(dQ), _merged(dK), _merged(dV)], -1)


_DIVIDED_ALLOWED = {}


def divided_allowed(mode, T, n):
    """bool [S, S] (S = 1 + T n): which keys each query of the divided space / time attention sees, READ OFF
    oracle.divided_attention_core instead of restated: with q = k = 0 every visible key gets the same weight, and with one head
    of dh = S and V = I the output row q is that weight on exactly the keys q sees."""
    key = (mode, T, n)
    if key not in _DIVIDED_ALLOWED:
        from oracle import tvts_oracle as O
        S = 1 + T * n
        x = torch.zeros(1, S, 3 * S, dtype=torch.float64)
        x[0, :, 2 * S:] = torch.eye(S, dtype=torch.float64)
        _DIVIDED_ALLOWED[key] = O.divided_attention_core(x, 1, mode, T, n)[0] > 0
    return _DIVIDED_ALLOWED[key]


def divided_fwd_ref(qkv, heads, dh, mode, T, n, **kw):
    """attn_fwd_ref in the divided geometry: a patch query sees the CLS key and its group, the CLS query every key"""
    return attn_fwd_ref(qkv, heads, dh, allowed=divided_allowed(mode, T, n), **kw)


def divided_bwd_same_inputs(qkv, dO, O_read, lse2_read, heads, dh, mode, T, n, **kw):
    return attn_bwd_same_inputs(qkv, dO, O_read, lse2_read, heads, dh, allowed=divided_allowed(mode, T, n), **kw)


def divided_mixed_o_read(O_exact, out_kernel):
    """[B, S, W] float64: the output the FUSED divided backward takes D = rowsum(dO o O) from.  Its patch rows form D in registers
    from the unrounded output (O_exact, float64, stands for it); its CLS rows (row 0 of every clip) get D from attn_delta_kernel on
    the bf16 `out` the forward stored (out_kernel, widened)."""
    o = O_exact.double().clone()
    o[:, 0] = out_kernel[:, 0].double()
    return o


def attn_conditioning(qkv, dO, heads, dh, *, floor=0.05, o_read=None, **kw):
    """How far float64 autograd is from ANY backward that takes delta from the saved bf16 output: per (row, head) rows_rel of
    attn_bwd_same_inputs(O_read = bf16(O_exact), lse2_exact) against autograd -> {"dq" | "dk" | "dv": [B * S, heads]}.
    A property of the inputs alone (no kernel): with few keys dP - delta cancels and the rounding of O shows through in dQ / dK.
    o_read: the output a backward reads as a function of the exact one, where it is not bf16(O_exact) in every row
    (divided_mixed_o_read)."""
    B, S, W3 = qkv.shape
    W = W3 // 3
    out, ref = attn_autograd(qkv, dO, heads, dh, **kw)
    with torch.no_grad():
        _, lse2, _ = attn_fwd_ref(qkv, heads, dh, **kw)
        got = attn_bwd_same_inputs(qkv, dO, out.bfloat16() if o_read is None else o_read(out), lse2, heads, dh, **kw)
    res = {}
    for i, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(i * W, (i + 1) * W)
        res[nm] = rows_rel(got[..., sl].reshape(B * S, W), ref[..., sl].reshape(B * S, W), heads, floor)[0]
    return res


# ------------------------------------------------------------------------------------------------ ordered sums (embed kernels)
def sum_bound(S, n, out_dtype=torch.float32, init=None, ref=None, c=2):
    """Per-element bound for an fp32 sum of n addends, accumulated (`+=`) into an output that held `init`, in ANY order.

    Derivation (as gemm_bound).  The kernels add their rows in a fixed order of their own -- a thread's running sum, per-block
    partials, thread groups combined through LDS -- and finish with `out += t`.  Whatever the order, the n addends and the initial
    value are the leaves of a binary tree of n roundings, and recursive summation (Higham, Thm 4.3 / eq. 4.4) gives

        |got - ref| <= gamma_{n + c} * (S + |init|),   gamma_k = k u / (1 - k u),   u = 2^-24,

    S the float64 sum of the absolute addends.  c (default 2) covers what a kernel does to the finished sum besides adding: the
    division of a mean, one scale factor.  The addends themselves are exact (fp32 values read from memory).  n may be a tensor
    (one count per row: the rows of an embedding table get as many addends as tokens point at them).  For an output that is
    then rounded to bf16 pass out_dtype and `ref`: u_out |ref| is added as in gemm_bound."""
    S = S.double() if torch.is_tensor(S) else torch.tensor(float(S), dtype=torch.float64)
    if init is not None:
        S = S + (init.double().abs() if torch.is_tensor(init) else abs(float(init)))
    k = (n.double() if torch.is_tensor(n) else float(n)) + c
    acc = S * (k * U32 / (1.0 - k * U32))
    if out_dtype == torch.float32:
        return acc + 1e-45
    u = U_OUT[out_dtype]
    return u * ref.double().abs() + (1.0 + u) * acc + 1e-45


# ------------------------------------------------------------------------------------------------ loss heads
# Relative error of the loss kernels' __expf / __logf (hardware exp2 / log2 and one multiplication by log2 e / ln 2): taken at the
# project's figure for the fast transcendentals.  In a log-sum-exp it also absorbs the rounding of the arguments x - max
# (2u |x - max| per term, weighted by the softmax probabilities: <= 2u log G, under 2^-20 for G < 2900).
EPS_LOSS = EPS_ACT


def f32_const(v):
    """the fp32 value a kernel receives for the double v (eps, the betas, lr, wd), as a Python float"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def l2norm_check(x, eps, xn, inv, *, what):
    """xn = x / max(|x|, eps) and inv = +-1 / max(|x|, eps) (negative: the row was clamped, |x| <= eps) of l2norm_rows against
    float64, per element.  eps is taken as the fp32 value the kernel compares with.

    Bound.  s = fl(sum x^2) has only positive addends: relative error gamma_{E+c}; the square root halves it and adds its own
    rounding (counted twice: the build has no fast-math flag, but no claim of a correctly rounded sqrtf is relied on), the division
    1 / max(nrm, eps) two more, the product x * iv one:  |xn - ref| <= (gamma_{E+2} / 2 + 5u) |ref|,  |inv - ref| <= (gamma_{E+2} / 2
    + 4u) |ref|.  A clamped row divides by eps itself, which only removes terms.  The sign of inv must be the reference's unless
    the float64 norm is within that relative error of eps (a row of norm exactly eps may land on either side).  -> worst ratio"""
    E = x.shape[1]
    e32 = f32_const(eps)
    x64 = x.double()
    nrm = x64.pow(2).sum(1).sqrt()
    d = nrm.clamp_min(e32)
    r_n = _gamma(E + 2) / 2 + 5 * U32
    w = assert_within(xn, x64 / d[:, None], (x64 / d[:, None]).abs() * r_n + 1e-45, f"{what}: xn")
    w = max(w, assert_within(inv.abs(), 1.0 / d, (1.0 / d) * (r_n - U32) + 1e-45, f"{what}: |inv|"))
    sure = (nrm - e32).abs() > r_n * nrm + 1e-300
    want_clamped = nrm <= e32
    wrong = sure & ((inv < 0) != want_clamped)
    if bool(wrong.any()):
        r = int(torch.nonzero(wrong)[0])
        raise AssertionError(f"{what}: clamp flag (sign of inv) wrong on {int(wrong.sum())} rows; first row {r}: norm {float(nrm[r])!r} "
                             f"eps {e32!r} inv {float(inv[r])!r}")
    return w


def l2norm_bwd_ref(dxn, xn, inv):
    """float64 dx = |inv| (dxn - xn <xn, dxn>), or |inv| dxn on the rows whose inv is negative (clamped), and the bound's pieces"""
    d, n = dxn.double(), xn.double()
    iv = inv.double().abs()[:, None]
    clamped = (inv < 0)[:, None]
    s = (n * d).sum(1, keepdim=True)
    return torch.where(clamped, iv * d, iv * (d - n * s)), (d, n, iv, clamped, s)


def l2norm_bwd_check(dxn, xn, inv, dx, *, what):
    """dx of l2norm_rows_bwd against float64 evaluated on the xn and inv the kernel READ (as ln_bwd_check does with mean / rstd).

    Bound.  The dot s = <xn, dxn> is an fp32 sum of E rounded products: |s~ - s| <= e_s = sum_bound(sum |xn dxn|, E, c=3).  Then
    t = xn s~ (one rounding), d - t (one), the product with inv (one):
        |dx - ref| <= |inv| (|xn| e_s + u |xn s| + u (|d| + |xn s| + |xn| e_s)) + u |ref|.
    A clamped row is the one product inv * d: u |ref|.  -> worst ratio"""
    E = dxn.shape[1]
    ref, (d, n, iv, clamped, s) = l2norm_bwd_ref(dxn, xn, inv)
    e_s = sum_bound((n * d).abs().sum(1, keepdim=True), E, c=3)
    t = (n * s).abs()
    acc = iv * (n.abs() * e_s + U32 * t + U32 * (d.abs() + t + n.abs() * e_s)) + U32 * ref.abs()
    bound = torch.where(clamped, U32 * ref.abs(), acc) + 1e-45
    return assert_within(dx, ref, bound, f"{what}: dx")


def lse_bound(ref, mx, n):
    """|lse - ref| of an fp32 log-sum-exp m + log(sum exp(x - m)) over n terms: every exponential carries a relative error EPS_LOSS,
    so does the sum (absolute EPS_LOSS after the logarithm); the n - 1 additions of terms in (0, 1] give gamma_{n+2} relative on the
    sum (the same after the logarithm); the logarithm itself EPS_LOSS (1 + |log s|) with log s = ref - max; the last addition u |ref|.
    An online (max, sum) walk multiplies its running sum by further exponentials <= 1: counted in EPS_LOSS' headroom over the 1 ulp
    hardware exp2, and measured (the `acc` figure of the BOUND lines)."""
    return U32 * ref.abs() + _gamma(n + 2) + 2 * EPS_LOSS * (1.0 + (ref - mx).abs())


def infonce_ref(x, loss0=0.0):
    """float64 references and bounds of tvts_infonce on the x [G, G] the kernel read -> dict(lse, lse_b, dx, dx_b, loss, loss_b)"""
    G = x.shape[0]
    x64 = x.double()
    rl, cl = torch.logsumexp(x64, 1), torch.logsumexp(x64, 0)
    d_rl, d_cl = lse_bound(rl, x64.max(1).values, G), lse_bound(cl, x64.max(0).values, G)
    ar, ac = x64 - rl[:, None], x64 - cl[None, :]
    pr, pc = torch.exp(ar), torch.exp(ac)
    dx = (pr + pc - 2.0 * torch.eye(G, dtype=torch.float64, device=x.device)) / G
    dx_b = (pr * (EPS_LOSS + U32 * ar.abs() + d_rl[:, None]) + pc * (EPS_LOSS + U32 * ac.abs() + d_cl[None, :])) / G + 2 * U32 * dx.abs() + 1e-45
    dg = x64.diagonal()
    loss = float(loss0) - float((2.0 * dg - rl - cl).sum()) / G
    S = float((2.0 * dg.abs() + rl.abs() + cl.abs()).sum()) / G
    loss_b = float(sum_bound(S, 3 * G, init=loss0)) + float((d_rl + d_cl).sum()) / G
    return dict(lse=torch.cat([rl, cl]), lse_b=torch.cat([d_rl, d_cl]), dx=dx, dx_b=dx_b, loss=loss, loss_b=loss_b, pr=pr, pc=pc)


def infonce_check(x, lse=None, dx=None, loss=None, loss0=0.0, *, what):
    """tvts_infonce's lse [2G] (rows | columns), dx [G, G] and loss (accumulated into loss0) against float64 on the x the kernel read.

    lse:  lse_bound -- u |ref| + gamma_{G+2} + 2 EPS_LOSS (1 + |ref - max|), absolute.
    dx = (e^{x - rowlse} + e^{x - collse} - 2 delta) / G: each exponential p carries the relative error EPS_LOSS + u |x - lse| (the
          rounded argument) + d_lse (the error of the lse it subtracts, lse_bound); the two errors are divided by G, and the sum, the
          subtraction of 2 and the division add 2u |dx|.
    loss = loss0 - (1 / G) sum_i (2 x_ii - rowlse_i - collse_i): a sum_bound over its 3G terms (and loss0), plus the mean of the d_lse
          of the 2G values it reads.  -> {"lse" | "dx" | "loss": worst ratio}"""
    r = infonce_ref(x, loss0)
    out = {}
    if lse is not None:
        out["lse"] = assert_within(lse, r["lse"], r["lse_b"], f"{what}: lse")
    if dx is not None:
        out["dx"] = assert_within(dx, r["dx"], r["dx_b"], f"{what}: dx")
    if loss is not None:
        got = float(loss)
        assert math.isfinite(got) and abs(got - r["loss"]) <= r["loss_b"], f"{what}: loss {got!r} ref {r['loss']!r} bound {r['loss_b']:.3g}"
        out["loss"] = abs(got - r["loss"]) / r["loss_b"]
    return out


def ce_check(logits, labels, scale, dlogits=None, loss=None, loss0=0.0, *, what):
    """tvts_cross_entropy against float64: loss = loss0 + scale * mean_r (lse_r - x[r, label_r]), dlogits = scale (softmax - onehot) / R.

    lse_r: lse_bound over C terms (d_r).  dlogits: the exponential e^{x - lse} carries EPS_LOSS + u |x - lse| + d_r relative; the
    subtraction of the one-hot, the product with scale and the division (two roundings) add 4u |ref|.  loss: the kernel adds the R
    non-negative differences lse_r - x[r, label_r] (one rounding each, exact operands apart from d_r): a sum_bound over R addends
    (times |scale| / R; c = 5: that subtraction, the product, the division twice) and loss0, plus |scale| mean d_r.  -> {name: worst ratio}"""
    R, C = logits.shape
    x64 = logits.double()
    lb = labels.long()
    lse = torch.logsumexp(x64, 1)
    d = lse_bound(lse, x64.max(1).values, C)
    a = x64 - lse[:, None]
    p = torch.exp(a)
    onehot = torch.zeros_like(p).scatter_(1, lb[:, None], 1.0)
    ref = scale * (p - onehot) / R
    out = {}
    if dlogits is not None:
        b = abs(scale) / R * p * (EPS_LOSS + U32 * a.abs() + d[:, None]) + 4 * U32 * ref.abs() + 1e-45
        out["dlogits"] = assert_within(dlogits, ref, b, f"{what}: dlogits")
    if loss is not None:
        xl = x64.gather(1, lb[:, None])[:, 0]
        lref = float(loss0) + scale * float((lse - xl).sum()) / R
        S = abs(scale) / R * float((lse - xl).sum())
        lb_ = float(sum_bound(S, R, init=loss0, c=5)) + abs(scale) * float(d.sum()) / R
        got = float(loss)
        assert math.isfinite(got) and abs(got - lref) <= lb_, f"{what}: loss {got!r} ref {lref!r} bound {lb_:.3g}"
        out["loss"] = abs(got - lref) / lb_
    return out


def contrastive_bound(v, t, temp, eps):
    """float64 autograd of the contrastive head (cosine similarity / temp, InfoNCE both ways) and a per-element bound on the dv / dt
    that LossHead.contrastive returns, composed from the stage bounds above -> (loss, dv, dt, e_dv, e_dt).

    Stages.  vn, tn: relative error r_n (l2norm_check).  x = vn tn^T / temp: gemm_acc_bound(K = E) plus 2 r_n S for the operands,
    e_x its largest element.  dx: infonce_ref's dx_b, plus the softmax' response to a shift of every x by <= e_x: each probability
    changes by a factor within e^{+-2 e_x}, so |delta dx| <= 2.01 e_x (P_row + P_col) / G.  dvn = dx tn / temp (dtn = dx^T vn / temp):
    (e_dx |tn| + r_n |dx| |tn|) / temp plus gemm_acc_bound(K = G).  dv = inv (dvn - vn <vn, dvn>): the propagated
    inv (e_dvn + |vn| (<|vn|, e_dvn> + r_n <|vn|, |dvn|>)), 4 r_n on every term for the errors of vn and inv, and l2norm_bwd_check's own rounding terms."""
    G, E = v.shape
    e32 = f32_const(eps)
    vr, tr = v.double().clone().requires_grad_(True), t.double().clone().requires_grad_(True)
    nv, nt = vr.norm(dim=1, keepdim=True).clamp_min(e32), tr.norm(dim=1, keepdim=True).clamp_min(e32)
    x = (vr / nv) @ (tr / nt).t() / temp
    loss = -(torch.log_softmax(x, 1).diagonal().mean() + torch.log_softmax(x.t(), 1).diagonal().mean())
    loss.backward()
    with torch.no_grad():
        vn, tn, iv, it = (vr / nv).detach(), (tr / nt).detach(), 1.0 / nv, 1.0 / nt
        r_n = _gamma(E + 2) / 2 + 5 * U32
        Sx = vn.abs() @ tn.abs().t() / temp
        e_x = float((gemm_acc_bound(Sx, E) + 2 * r_n * Sx + U32 * x.abs()).max())
        r = infonce_ref(x.detach())
        e_dx = r["dx_b"] + 2.01 * e_x * (r["pr"] + r["pc"]) / G
        dx = r["dx"]
        out = []
        for dxm, e_dxm, a, b, ia in ((dx, e_dx, vn, tn, iv), (dx.t(), e_dx.t(), tn, vn, it)):
            S = dxm.abs() @ b.abs() / temp
            dn = dxm @ b / temp
            e_dn = (e_dxm @ b.abs()) / temp + r_n * S + gemm_acc_bound(S, G)
            s = (a * dn).sum(1, keepdim=True)
            terms = ia * (dn.abs() + a.abs() * s.abs())
            sa = (a * dn).abs().sum(1, keepdim=True)
            e_s = (a.abs() * e_dn).sum(1, keepdim=True) + r_n * sa + sum_bound(sa, E, c=3)
            out.append(ia * (e_dn + a.abs() * e_s) + (4 * r_n + 4 * U32) * terms + 1e-45)
    return float(loss.detach()), vr.grad, tr.grad, out[0], out[1]


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_check(p0, g, m0, v0, p1, m1, v1, shadow, *, lr, wd, step, beta1=0.9, beta2=0.999, eps=1e-6, grad_scale=1.0, what):
    """One Hugging Face AdamW step of tvts_adamw_hf on one parameter group, against float64 from the fp32 p0, g, m0, v0 the kernel
    read; p1, m1, v1 per element, the bf16 shadow bit for bit as bf16(p1).

    The constants are the fp32 values the kernel receives: b1 = fp32(beta1), o1 = fp32(1 - beta1) (b2, o2 alike), fp32(eps),
    fp32(lr), fp32(wd), and the step size ss = fp32(lr sqrt(1 - beta2^t) / (1 - beta1^t)) formed in double from the double betas.
    With gg = g grad_scale (one rounding, u):
      m1 = b1 m0 + o1 gg              |err| <= e_m = 3u (|b1 m0| + |o1 gg|)              (two products, gg, the sum)
      v1 = b2 v0 + o2 gg gg           |err| <= e_v = 5u v1                               (gg twice, two products, the sum; all terms >= 0)
      r  = sqrt(v1)                   |err| <= e_r = (e_v / 2 v1 + 2u) r = 4.5u r        (sqrt counted as two roundings)
      d  = r + eps                    |err| <= e_d = e_r + u d
      q  = ss m1 / d                  |err| <= e_q = ss e_m / d + |q| (5u + e_d / d)      (ss: one ulp between the host's and the
                                                                                          device's pow; product; division twice; 1u slack)
      p' = p0 - q                     |err| <= e_q + u |p'|
      p1 = p' - (lr wd) p'  (wd > 0)  |err| <= (1 + lr wd) e_p' + 2u |lr wd p'| + u |p1|
    An element with g = 0, m0 = v0 = 0 keeps p exactly (q = 0 / eps).  -> worst ratio"""
    b1, b2 = f32_const(beta1), f32_const(beta2)
    o1, o2 = f32_const(1.0 - beta1), f32_const(1.0 - beta2)
    e32, lr32, wd32, gs = f32_const(eps), f32_const(lr), f32_const(wd), f32_const(grad_scale)
    ss = f32_const(lr32 * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step))
    p, gg, m, v = p0.double(), g.double() * gs, m0.double(), v0.double()
    mr = b1 * m + o1 * gg
    e_m = 3 * U32 * ((b1 * m).abs() + (o1 * gg).abs())
    vr = b2 * v + o2 * gg * gg
    e_v = 5 * U32 * vr
    r = vr.sqrt()
    e_r = 4.5 * U32 * r * 1.001
    d = r + e32
    e_d = e_r + U32 * d
    q = ss * mr / d
    e_q = ss * e_m / d + q.abs() * (5 * U32 + e_d / d) * 1.001
    pr = p - q
    e_p = e_q + U32 * pr.abs()
    if wd32 > 0:
        dec = lr32 * wd32
        pr2 = pr - dec * pr
        e_p = (1 + dec) * e_p + 2 * U32 * (dec * pr).abs() + U32 * pr2.abs()
        pr = pr2
    w = assert_within(m1, mr, e_m + 1e-45, f"{what}: m")
    w = max(w, assert_within(v1, vr, e_v + 1e-45, f"{what}: v"))
    w = max(w, assert_within(p1, pr, e_p + 1e-45, f"{what}: p"))
    assert_equal_bits(shadow, p1.bfloat16(), f"{what}: bf16 shadow")
    return w
