"""The small kernels at the bottom of csrc/gemm.hip at the edges of their launch geometry, per element (run with -m gpu).

tvts_colsum_bf16 (bias gradients under frozen weights), tvts_gemm_small_f32 (the G x G similarity and its backward products),
tvts_rows_linear_bf16 (the CLS rows of the hybrid residual stream) and tvts_gemm_tn_bf16_grouped (every ViT weight gradient at the
reference's per-GPU batch) were held by whole-tensor gates at a few shapes.  Here each runs at the sizes where its code takes
another path -- row ranges and their fallbacks, the MFMA cut and the 16-byte staging choice, waves without a K step and either side
of the unrolled loop, ragged tiles / mixed contraction lengths / strided outputs inside one group -- on operands inside NaN-poisoned
buffers, into NaN-guarded outputs, every element against float64 within kernel_bounds.gemm_bound / sum_bound.  No tolerance of
its own: every gate is one of those derived bounds or bit equality.  Case tables: tests/gemm_cases.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_cases as GC  # noqa: E402
import kernel_bounds as KB  # noqa: E402


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


DEV = "cuda:0"
EINVAL = -22
NAN = float("nan")


def _lib():
    from tvts_amd import _lib as L
    return L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ 1. tvts_colsum_bf16
def _colsum(x, M, N, out, ws, ws_elems):
    rc = _lib().tvts_colsum_bf16(_ptr(x), x.stride(0), M, N, _ptr(out), _ptr(ws), ws_elems, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("M", GC.COLSUM_M)
def test_colsum_row_ranges_column_tails_and_workspace_fallbacks_within_the_bound(K, M):
    """out[n] += sum_m X[m, n] through the raw entry point, every column within sum_bound (M addends and the initial value) of the
    float64 sum of the bf16 values.  M = 4097 / 8193 take two / three row ranges (the last of 2048 / 2731 rows) when the workspace
    holds the partials; without one (NULL) and with one that is a single element short the entry point must fall back to ONE
    range, still be right and leave the short workspace unwritten.  N = 72 / 136 end in a block of 8 live columns out of 64;
    ld = N + 8 puts NaN right of every row; rows past M are NaN; out carries a sentinel behind column N - 1.  With the partials two
    calls give the same bits."""
    shared = K._tn_workspace(torch.device(DEV))
    ranges = min(-(-M // GC.COLSUM_RANGE_ROWS), 256)
    worst = 0.0
    for N in GC.COLSUM_N:
        for ld in (N, N + 8):
            g = torch.Generator(device=DEV).manual_seed(M + 7 * N + ld)
            buf, x = GC.poisoned(M, N, torch.bfloat16, DEV, left=0, right=ld - N)
            assert x.stride(0) == ld and x.data_ptr() % 16 == 0
            x.copy_(torch.randn(M, N, generator=g, device=DEV).bfloat16())
            init = torch.randn(N, generator=g, device=DEV)
            ref = x.double().sum(0) + init.double()
            bound = KB.sum_bound(x.double().abs().sum(0), M, init=init)
            short = torch.full((ranges * N,), NAN, device=DEV)
            got = {}
            for name, ws, elems in (("shared", shared, shared.numel()), ("null", None, 0), ("short", short, ranges * N - 1),
                                    ("shared again", shared, shared.numel())):
                out = torch.cat([init, torch.full((1,), 12345.0, device=DEV)])
                _colsum(x, M, N, out, ws, elems)
                what = f"colsum M={M} N={N} ld={ld} workspace={name}"
                worst = max(worst, KB.assert_within(out[:N], ref, bound, what))
                assert float(out[N]) == 12345.0, f"{what}: the element behind column {N - 1} was written"
                got[name] = out
            assert bool(torch.isnan(short).all()), f"colsum M={M} N={N} ld={ld}: a workspace one element short was written"
            KB.assert_equal_bits(got["shared again"], got["shared"], f"colsum M={M} N={N} ld={ld}, second call")
            KB.assert_equal_bits(got["short"], got["null"], f"colsum M={M} N={N} ld={ld}: short workspace against none (both one range)")
    KB.bound_line(f"colsum_edges[{M}]", worst)


# ------------------------------------------------------------------------------------------------ 2. tvts_gemm_small_f32
def _flat(values, misaligned):
    """the fp32 values (any shape) stored contiguously between NaNs, at a 16-byte boundary or one float past one"""
    n = values.numel()
    buf = torch.full((n + 12,), NAN, device=DEV)
    off = 5 if misaligned else 4
    v = buf[off:off + n]
    v.copy_(values.reshape(-1))
    assert v.data_ptr() % 16 == (4 if misaligned else 0)
    return v


def _small_operand(vals, transposed, misaligned=False):
    """vals [X, K] (A: X = M; B given as [N, K]) -> (storage, stride of x, stride of k): row-major [X, K] or its transpose [K, X]"""
    X, Kd = vals.shape
    if transposed:
        return _flat(vals.t().contiguous(), misaligned), 1, X
    return _flat(vals.contiguous(), misaligned), Kd, 1


def _small_patterns(av, bv, mis_a=False, mis_b=False):
    """the four unit-stride patterns: A [M, K] row-major / stored as [K, M]; B [K, N] row-major / stored as [N, K].
    bv is B^T [N, K] (check_gemm's second operand) -> (name, A storage, sa, B storage, sb)"""
    for ta in (False, True):
        for tb in (False, True):
            a_s, sai, sak = _small_operand(av, ta, mis_a)
            # B[k, j] = bv[j, k]: "row-major B" stores bv transposed
            b_s, sbj, sbk = _small_operand(bv, not tb, mis_b)
            yield f"A{'^T' if ta else ''} B{'^T' if tb else ''}", a_s, (sai, sak), b_s, (sbk, sbj)


@pytest.mark.parametrize("M,N,K_", GC.SMALL_SHAPES)
def test_gemm_small_dispatch_cut_stride_patterns_and_staging_choice_within_the_bound(K, M, N, K_):
    """C (+)= alpha A B + bias on fp32 operands (the products round too: c = 6), every element within gemm_bound, C inside a guarded
    buffer with ldc = N + 3.  The shapes sit on both sides of the MFMA cut (31 / 32 rows and columns, K = 15 / 16), stick out of
    the 64 x 64 tile and the 32-deep stage by one, or are the scalar kernel's smallest; each runs all four unit-stride patterns,
    with alpha and bias, accumulating, and plain.  Every pattern runs again with A, with B and with both one float past a 16-byte
    boundary: a problem the dispatcher stages with 16-byte loads then takes the scalar staging, which fills the same LDS for the
    same MFMA chain -- within the bound and the bits of the aligned run.  Last, an operand with neither stride 1: every second
    column of a matrix twice as wide (the columns between are NaN), A against both forms of B and B against row-major A."""
    g = torch.Generator(device=DEV).manual_seed(1000 * M + 10 * N + K_)
    av = torch.randn(M, K_, generator=g, device=DEV)
    bv = torch.randn(N, K_, generator=g, device=DEV)
    bias = GC.place(torch.randn(N, generator=g, device=DEV))
    init = torch.randn(M, N, generator=g, device=DEV)
    worst, eligible = 0.0, 0

    def run(a_s, sa, b_s, sb, what, **kw):
        buf, out = KB.guarded(M, N, torch.float32, DEV, cols=3)
        assert out.stride(0) == N + 3
        if kw.get("accumulate"):
            out.copy_(init)
        K.gemm_small(a_s, b_s, out, M=M, N=N, K=K_, sa=sa, sb=sb, **kw)
        torch.cuda.synchronize()
        KB.check_guards(buf, M, N, what)
        w = KB.check_gemm(out, av, bv, scale=kw.get("alpha"), bias=kw.get("bias"), residual=init if kw.get("accumulate") else None,
                          c=6, what=what)
        return out.clone(), w

    for name, a_s, sa, b_s, sb in _small_patterns(av, bv):
        tag = f"gemm_small {M},{N},{K_} {name}"
        first, w = run(a_s, sa, b_s, sb, tag + " alpha bias", alpha=0.5, bias=bias)
        worst = max(worst, w)
        worst = max(worst, run(a_s, sa, b_s, sb, tag + " accumulate", accumulate=True)[1])
        worst = max(worst, run(a_s, sa, b_s, sb, tag + " alpha bias accumulate", alpha=-1.5, bias=bias, accumulate=True)[1])
        worst = max(worst, run(a_s, sa, b_s, sb, tag + " plain")[1])
        eligible += GC.small_vec_eligible(M, N, K_, sa, sb)
    for mis_a, mis_b in ((True, True), (True, False), (False, True)):
        aligned = _small_patterns(av, bv)
        for (name, a_s, sa, b_s, sb), (_, a0, _, b0, _) in zip(_small_patterns(av, bv, mis_a, mis_b), aligned):
            tag = f"gemm_small {M},{N},{K_} {name} misaligned A={mis_a} B={mis_b}"
            want, _ = run(a0, sa, b0, sb, tag + " (aligned)", alpha=0.5, bias=bias)
            got, w = run(a_s, sa, b_s, sb, tag, alpha=0.5, bias=bias)
            worst = max(worst, w)
            KB.assert_equal_bits(got, want, tag + ": scalar staging against the aligned run")
    if M % 4 == 0 and N % 4 == 0 and K_ % 4 == 0 and M >= 32 and N >= 32 and K_ >= 16:
        assert eligible == 4, eligible  # these are the problems whose aligned runs took the 16-byte staging
    # neither stride 1
    wide_a = torch.full((M, 2 * K_), NAN, device=DEV)
    wide_a[:, 0::2] = av
    wide_b = torch.full((K_, 2 * N), NAN, device=DEV)
    wide_b[:, 0::2] = bv.t()
    for name, a_s, sa, b_s, sb in _small_patterns(av, bv):
        if name.startswith("A "):
            worst = max(worst, run(wide_a, (2 * K_, 2), b_s, sb, f"gemm_small {M},{N},{K_} A every second column, {name}", alpha=0.5, bias=bias)[1])
        if name == "A B":
            worst = max(worst, run(a_s, sa, wide_b, (2 * N, 2), f"gemm_small {M},{N},{K_} B every second column", alpha=0.5, bias=bias)[1])
            worst = max(worst, run(wide_a, (2 * K_, 2), wide_b, (2 * N, 2), f"gemm_small {M},{N},{K_} both every second column",
                                   accumulate=True)[1])
    KB.bound_line(f"gemm_small_edges[{M},{N},{K_}]", worst)


def test_gemm_small_refuses_empty_problems(K):
    """M, N, K <= 0 return -22 and write nothing"""
    lib = _lib()
    a, b = torch.ones(64, device=DEV), torch.ones(64, device=DEV)
    out = torch.full((64,), NAN, device=DEV)

    def rc(M, N, Kd):
        return lib.tvts_gemm_small_f32(_ptr(a), 8, 1, _ptr(b), 8, 1, M, N, Kd, 1.0, None, _ptr(out), 8, 0, _stream())
    for bad in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (8, -1, 8), (8, 8, -1)):
        assert rc(*bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert rc(8, 8, 8) == 0  # the same call with valid extents runs
    torch.cuda.synchronize()
    assert bool((out == 8.0).all())


# ------------------------------------------------------------------------------------------------ 3. tvts_rows_linear_bf16
@pytest.mark.parametrize("Kd", GC.ROWS_LINEAR_K)
def test_rows_linear_wave_steps_row_tiles_and_strides_within_the_bound(K, Kd):
    """out = residual + bias + A W^T for a few rows, every element within gemm_bound.  K = 32 / 64 / 96 leave three / two / one of
    the four waves without a 32-deep step, 128 / 160 give every wave one and wave 0 a second; 416 / 512 / 544 sit on both sides of
    the four-steps-in-flight loop's condition for wave 0 (384 < K) and wave 3 (480 < K).  R = 15 / 16 / 17 / 33 end inside, at and
    one past a 16-row tile; N = 16 is one column tile.  A is a strided row view (lda = S K, the rows between are NaN, and so are
    the rows behind the last one, which the ragged tile's lanes must not read), W has ldw = K + 8 with NaN in the gap, the residual
    ldr = N + 8, and out sits in a guarded buffer with ldo = N + 8 and a whole 16-row tile of guard rows under it.  With and without
    bias and residual; two calls give the same bits."""
    worst = 0.0
    for R in GC.ROWS_LINEAR_R:
        for N in GC.ROWS_LINEAR_N:
            for S in (1, 3):
                g = torch.Generator(device=DEV).manual_seed(Kd + 100 * R + N + S)
                full = torch.full((R * S + 2, Kd), NAN, dtype=torch.bfloat16, device=DEV)
                a = full[:R * S:S]
                a.copy_(torch.randn(R, Kd, generator=g, device=DEV).bfloat16())
                assert tuple(a.shape) == (R, Kd) and a.stride(0) == S * Kd and a.data_ptr() == full.data_ptr()
                _, w = GC.poisoned(N, Kd, torch.bfloat16, DEV, left=0, right=8)
                w.copy_((torch.randn(N, Kd, generator=g, device=DEV) * Kd ** -0.5).bfloat16())
                assert w.stride(0) == Kd + 8
                bias = GC.place(torch.randn(N, generator=g, device=DEV))
                _, res = GC.poisoned(R, N, torch.float32, DEV, left=0, right=8)
                res.copy_(torch.randn(R, N, generator=g, device=DEV))
                for b, r in ((bias, res), (None, None), (bias, None), (None, res)):
                    what = f"rows_linear R={R} K={Kd} N={N} S={S} bias={b is not None} residual={r is not None}"
                    buf, out = KB.guarded(R, N, torch.float32, DEV, rows=16, cols=8)
                    K.rows_linear(a, w, out, bias=b, residual=r)
                    torch.cuda.synchronize()
                    KB.check_guards(buf, R, N, what)
                    worst = max(worst, KB.check_gemm(out, a, w, bias=b, residual=r, what=what))
                    buf2, out2 = KB.guarded(R, N, torch.float32, DEV, rows=16, cols=8)
                    K.rows_linear(a, w, out2, bias=b, residual=r)
                    KB.assert_equal_bits(out2, out, what + ", second call")
    KB.bound_line(f"rows_linear_edges[{Kd}]", worst)


# ------------------------------------------------------------------------------------------------ 4. tvts_gemm_tn_bf16_grouped
def _group_problems(spec, seed):
    """the members of a group as TnGroup problems, each with what the checks need: operands as column slices of one poisoned buffer,
    the output in a guarded buffer (ldo = Nb + 4, or dense: guard rows only), the bias gradient with NaN behind it"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    probs = []
    for (M, Na, Nb, accumulate, colsum, strided) in spec:
        p = torch.randn(M, Na, generator=g, device=DEV).bfloat16()
        q = torch.randn(M, Nb, generator=g, device=DEV).bfloat16()
        p, q = GC.place_pair(p, q)
        init = torch.randn(Na, Nb, generator=g, device=DEV)
        cs_init = torch.randn(Na, generator=g, device=DEV)
        buf, out = KB.guarded(Na, Nb, torch.float32, DEV, cols=4 if strided else 0)
        assert out.stride(0) == (Nb + 4 if strided else Nb)
        csbuf = torch.full((Na + 8,), NAN, device=DEV) if colsum else None
        probs.append(dict(p=p, q=q, out=out, M=M, accumulate=accumulate, colsum=csbuf[:Na] if colsum else None, buf=buf, csbuf=csbuf,
                          init=init, cs_init=cs_init))
    return probs


def _group_reset(probs):
    for pr in probs:
        pr["buf"].fill_(NAN)
        if pr["accumulate"]:
            pr["out"].copy_(pr["init"])
        if pr["csbuf"] is not None:
            pr["csbuf"].fill_(NAN)
            pr["colsum"].copy_(pr["cs_init"])


@pytest.mark.parametrize("name", sorted(GC.TN_GROUPS))
def test_gemm_tn_grouped_ragged_mixed_and_strided_members_within_the_bound(K, name):
    """One grouped launch (and its one reduce launch) over members the ViT block never gives it: a single member; 128-tiles ragged
    in both directions (Na, Nb = 136, 72, 264, 8, 392); members with different M under one forced range count, so that a short
    one stays unsplit beside split ones (the grouped reduce returns at once for it); outputs with ldo = Nb + 4 beside dense ones,
    both branches of the reduce's element pass; item totals that are no multiple of 8, whose padded blocks must do nothing.  The
    workspace is the caller's, filled with NaN.  Every output is held per element to gemm_bound with K = M (on top of its initial
    value where it accumulates), every bias gradient to sum_bound, all guards must be intact, the group run twice gives the same
    bits, and every member has the bits of its own tvts_gemm_tn_bf16 launch on the 128 tile with the same contraction ranges."""
    splits, spec = GC.TN_GROUPS[name]
    items = GC.tn_group_items(spec, splits)
    if name in ("trio", "few_items", "one_strided"):
        assert items % 8 != 0, items
    if name == "mixed_m":
        assert [GC.tn_group_ranges(m[0], splits)[0] for m in spec] == [2, 1, 2]
    probs = _group_problems(spec, seed=len(name) + 31 * splits)
    ws = torch.full((1 << 20,), NAN, device=DEV)
    grp = K.TnGroup(probs, ws, splits=splits)
    runs = []
    for _ in range(2):
        _group_reset(probs)
        grp.run()
        torch.cuda.synchronize()
        runs.append([(pr["out"].clone(), None if pr["colsum"] is None else pr["colsum"].clone()) for pr in probs])
    worst = 0.0
    for i, (pr, (M, Na, Nb, accumulate, colsum, strided)) in enumerate(zip(probs, spec)):
        what = f"tn grouped {name}[{i}] ({M}, {Na}, {Nb}) acc={accumulate} colsum={colsum} strided={strided}"
        KB.check_guards(pr["buf"], Na, Nb, what)
        worst = max(worst, KB.check_gemm(pr["out"], pr["p"].t(), pr["q"].t(), residual=pr["init"] if accumulate else None, K=M, what=what))
        if colsum:
            cs_ref = pr["p"].double().sum(0) + pr["cs_init"].double()
            cs_bound = KB.sum_bound(pr["p"].double().abs().sum(0), M, init=pr["cs_init"])
            worst = max(worst, KB.assert_within(pr["colsum"], cs_ref, cs_bound, what + ": colsum (per column)"))
            assert bool(torch.isnan(pr["csbuf"][Na:]).all()), f"{what}: colsum written past column {Na}"
        KB.assert_equal_bits(runs[1][i][0], runs[0][i][0], what + ", second run")
        if colsum:
            KB.assert_equal_bits(runs[1][i][1], runs[0][i][1], what + ": colsum, second run")
        # the member's own launch: under the group's range count where that gives it the same ranges, else under the count the
        # group gave it (a member with fewer than 256 rows per range takes fewer)
        mine = GC.tn_group_ranges(M, splits)
        s1 = splits if GC.tn_ranges(M, splits) == mine else mine[0]
        assert GC.tn_ranges(M, s1) == mine, (M, splits, s1, mine)
        buf1, out1 = KB.guarded(Na, Nb, torch.float32, DEV, cols=4 if strided else 0)
        if accumulate:
            out1.copy_(pr["init"])
        cs1 = pr["cs_init"].clone() if colsum else None
        K.gemm_tn(pr["p"], pr["q"], out1, M=M, accumulate=accumulate, colsum=cs1, tile=128, splits=s1, fused=False)
        torch.cuda.synchronize()
        KB.check_guards(buf1, Na, Nb, what + " (single launch)")
        KB.assert_equal_bits(runs[0][i][0], out1.clone(), what + ": group against the single launch")
        if colsum:
            KB.assert_equal_bits(runs[0][i][1], cs1, what + ": colsum, group against the single launch")
    KB.bound_line(f"gemm_tn_grouped_edges[{name}]", worst)


def test_gemm_tn_grouped_refusals(K):
    """-22 from the raw entry point, nothing written: no member, more than 64, Na % 8, ldo % 4, a row pitch below the row (ldo < Nb,
    ldp < Na), a table one byte short, a workspace one element short of the forced ranges' partials, an upload without the host
    table.  The same call unchanged returns 0.  (tests/test_gemm_side_edges_cpu.py: every single-field change of the record.)"""
    lib = _lib()
    M, Na, Nb = 520, 136, 72
    ws = torch.full((1 << 16,), NAN, device=DEV)
    need = 2 * Na * Nb

    def member(na=Na, ldo_extra=4):
        p = torch.zeros(M, Na + 8, dtype=torch.bfloat16, device=DEV)[:, :na]
        q = torch.zeros(M, Nb, dtype=torch.bfloat16, device=DEV)
        out = torch.full((Na, Nb + ldo_extra), NAN, device=DEV)[:, :Nb]
        return dict(p=p, q=q, out=out, M=M, accumulate=False, colsum=None)

    def rc(pr, *, n=1, short_table=0, upload=1, host=True, ws_elems=None):
        grp = K.TnGroup([pr], ws, splits=2)
        code = lib.tvts_gemm_tn_bf16_grouped(ctypes.cast(grp.recs, ctypes.c_void_p), n, _ptr(grp.table),
                                             ctypes.c_void_p(grp.table_host.data_ptr()) if host else None, grp.table.numel() - short_table,
                                             upload, _ptr(ws), ws.numel() if ws_elems is None else ws_elems, grp.opts, _stream())
        torch.cuda.synchronize()
        return code, grp

    cases = {"n = 0": dict(n=0), "n = 65": dict(n=65), "a table one byte short": dict(short_table=1),
             "workspace one element short": dict(ws_elems=need - 1), "upload without a host table": dict(host=False)}
    for why, kw in cases.items():
        pr = member()
        code, _ = rc(pr, **kw)
        assert code == EINVAL, (why, code)
        assert bool(torch.isnan(pr["out"]).all()) and bool(torch.isnan(ws).all()), why
    narrow_out, narrow_p = member(), member()  # a row pitch below the row: rows that overlap (tvts_gemm_tn_bf16 refuses it as well)
    narrow_out["out"] = torch.as_strided(torch.full((Na * Nb,), NAN, device=DEV), (Na, Nb), (Nb - 4, 1))
    narrow_p["p"] = torch.as_strided(torch.zeros(M * Na, dtype=torch.bfloat16, device=DEV), (M, Na), (Na - 8, 1))
    for why, pr in (("Na % 8", member(na=Na - 4)), ("ldo % 4", member(ldo_extra=2)), ("ldo < Nb", narrow_out), ("ldp < Na", narrow_p)):
        code, _ = rc(pr)
        assert code == EINVAL, (why, code)
        assert bool(torch.isnan(pr["out"]).all()) and bool(torch.isnan(ws).all()), why
    pr = member()
    code, grp = rc(pr, ws_elems=need)  # exactly enough
    assert code == 0, code
    assert bool((pr["out"] == 0).all())
