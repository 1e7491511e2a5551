"""The LayerNorm kernels at their width, row and stride edges, per element against float64 (run with -m gpu).

tests/test_kernels_gpu.py holds them to kernel_bounds.ln_fwd_check / ln_bwd_check at the training step's own sizes: widths that are
multiples of 64, contiguous inputs, every bf16 row on the 8-column kernel.  Here the case runners of tests/ln_cases.py (fwd_case /
bwd_case: the checks, the guards, the e4m3 references, what each case asserts about the kernel it reaches) run over the lists that
module derives from the kernels' constants: column groups partly inside the row, one to seven rows, the grid-stride wrap of every
template form, row lists, the `M` argument, every operand a view inside a NaN-poisoned buffer with a leading dimension of both
flavours (ld % 8 == 0 and == 4) and every output inside NaN / 0xFF guards.  The bounds are derived (a ratio <= 1 passes; nothing
here is calibrated): dgamma / dbeta are held per column to kernel_bounds.ln_cols_check, the summation bound of their M addends.
Measured ratios: profiles/r15_layernorm_edges_bounds.txt."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
import ln_cases as LC  # noqa: E402


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


DEV = "cuda:0"


def _period(M):
    """a CLS period for a sweep over row counts: one clip, or two where M is even"""
    return M // 2 if M % 2 == 0 else M


def _done(name, worst, cols=None):
    assert worst <= 1.0, (name, worst)
    KB.bound_line(name, worst)
    for k, v in (cols or {}).items():
        assert v <= 1.0, (name, k, v)
        KB.bound_line(f"{name} {k} (per column)", v)


# ------------------------------------------------------------------------------------------------ forward
FWD_SMALL = [(f["name"], W, lx, ly) for f in LC.FWD_FORMS for (W, lx, ly) in LC.fwd_widths(f)]


@pytest.mark.parametrize("name,W,ldx,ldy", FWD_SMALL, ids=[f"{n}-{W}-ld{a}{b}" for n, W, a, b in FWD_SMALL])
def test_forward_forms_over_their_widths_at_one_to_seven_rows(K, name, W, ldx, ldy):
    """every forward form (ln_cases.FWD_FORMS names the kernel; fwd_case asserts from the case's own W and pitches that the host
    takes that one) over its width list x M_SMALL: y, mean, rstd within the bound, the all-zero row is beta, guards intact,
    the e4m3 copies (per row: scale, bytes, quantize_fp8_rows; per tensor: bytes with saturation, amax exact / kept, tscale = 0)"""
    form = LC.FWD_BY_NAME[name]
    worst = 0.0
    for M in LC.M_SMALL:
        worst = max(worst, LC.fwd_case(K, DEV, form, M, W, ldx, ldy, seed=M + W, period=_period(M) if form["cls"] else 0))
    if form["q8"] == "rows":  # beta = 0: the all-zero row of x is an all-zero row of y, scale 1.0 and zero bytes
        worst = max(worst, LC.fwd_case(K, DEV, form, 5, W, ldx, ldy, seed=W, period=5 if form["cls"] else 0, zero_beta=True))
    _done(f"ln_fwd_edges[{name},{W},ld{ldx}{ldy}]", worst)


def _wrap_widths(form):
    return {"W_4COL": [(4, 4, 0), (260, 0, 4)], "W_8COL": [(8, 0, 0), (256, 0, 0)], "W_BF16_4COL": [(12, 4, 4), (260, 0, 0)]}[form["widths"]]


FWD_WRAP = [(f["name"], M, *w) for f in LC.FWD_FORMS for M in LC.M_WRAP_FWD for w in _wrap_widths(f)]


@pytest.mark.parametrize("name,M,W,ldx,ldy", FWD_WRAP, ids=[f"{n}-{M}-{W}" for n, M, W, _, _ in FWD_WRAP])
def test_forward_grid_wrap_of_every_form(K, name, M, W, ldx, ldy):
    """the forward grid is capped at 2048 blocks of 4 rows: at 8197 rows some waves walk to a second row and some do not (`more`
    false on the first trip), at 16385 one wave walks to a third; narrow rows (W <= 260) keep the case small"""
    form = LC.FWD_BY_NAME[name]
    period = {8197: 7, 16385: 5}[M] if form["cls"] else 0
    _done(f"ln_fwd_wrap[{name},{M},{W}]", LC.fwd_case(K, DEV, form, M, W, ldx, ldy, seed=M + W, period=period))


@pytest.mark.parametrize("name,W,ldx,ldy", [("f32_bf16", 260, 4, 0), ("f32_q8rows", 1028, 0, 4), ("bf16_8col_q8only_rows", 520, 0, 0),
                                            ("bf16_8col", 1032, 0, 0), ("bf16_4col_q8tensor", 516, 4, 0)])
def test_forward_rows_past_the_m_argument_keep_their_poison(K, name, W, ldx, ldy):
    """M smaller than the buffers (6 of 9 rows, 8201 of 8204 on a wrapped grid): rows >= M of y, q8, mean, rstd and row_scale
    stay NaN / 0xFF"""
    form = LC.FWD_BY_NAME[name]
    worst = LC.fwd_case(K, DEV, form, 6, W, ldx, ldy, seed=W, extra=3)
    if W <= 520:
        worst = max(worst, LC.fwd_case(K, DEV, form, 8201, W, ldx, ldy, seed=W + 1, extra=3))
    _done(f"ln_fwd_m_argument[{name},{W}]", worst)


def test_bf16_rows_of_512_columns_reach_both_kernels_and_e4m3_only_needs_the_8_column_one(K):
    """bf16 x at W = 512: with every pitch a multiple of 8 the 8-column kernel runs, with ldx or ldy 4 past one the 4-column
    kernel (ln8_ok; fwd_case asserts the choice from the pitches) -- both within the bound.  The e4m3-only call (y = None) exists
    on the 8-column kernel alone: with ldx % 8 == 4, ldq % 8 == 4 or W % 8 == 4 it is refused and nothing is written"""
    worst = 0.0
    for name, lx, ly in (("bf16_8col", 0, 0), ("bf16_4col", 4, 0), ("bf16_4col", 0, 4), ("bf16_8col_q8rows", 0, 0), ("bf16_4col_q8rows", 4, 0),
                         ("bf16_4col_q8rows", 0, 4)):
        worst = max(worst, LC.fwd_case(K, DEV, LC.FWD_BY_NAME[name], 7, 512, lx, ly, seed=ly + 2 * lx))
    gamma, beta = LC.affine(512, 1, DEV)
    for W, lx, lq in ((512, 4, 0), (512, 0, 4), (516, 0, 0)):
        x = LC.put(LC.special_rows(7, W, 2, DEV).bfloat16(), lx)
        gm, bt = (gamma, beta) if W == 512 else LC.affine(W, 1, DEV)
        qbuf, q = LC.out_mat(7, W, LC.U8, DEV, lq)
        rs, mean = LC.out_vec(7, DEV), LC.out_vec(7, DEV)
        with pytest.raises(K.HipError):
            K.layernorm_fwd(x, gm, bt, 1e-5, None, mean, q8=q, row_scale=rs)
        torch.cuda.synchronize()
        assert bool((qbuf == 0xFF).all()) and bool(torch.isnan(rs).all()) and bool(torch.isnan(mean).all()), (W, lx, lq)
    _done("ln_fwd_512_both_kernels", worst)


@pytest.mark.parametrize("name,W,ldx,ldy", [("f32_f32", 260, 4, 0), ("f32_q8rows", 1028, 0, 4), ("bf16_8col", 520, 0, 0), ("bf16_8col_q8rows", 1032, 0, 0),
                                            ("bf16_4col", 516, 4, 0), ("bf16_4col_q8rows", 512, 0, 4), ("f32_bf16", 4, 4, 4)])
def test_forward_on_gathered_rows(K, name, W, ldx, ldy):
    """rows through a permuted, non-monotonic list that holds row 0 and the last row of the source, on fp32 rows and on bf16 rows
    of both kernels, with and without the e4m3 copy; 9 rows, and 8197 (the list read on the second trip)"""
    form = LC.FWD_BY_NAME[name]
    worst = LC.fwd_case(K, DEV, form, 9, W, ldx, ldy, seed=W, gathered=True)
    if W <= 520:
        worst = max(worst, LC.fwd_case(K, DEV, form, 8197, W, ldx, ldy, seed=W + 1, gathered=True))
    _done(f"ln_fwd_rows[{name},{W}]", worst)


# ------------------------------------------------------------------------------------------------ backward
BWD_ALL = [(f["name"], W, M) for f in LC.FORMS for W in (260, 1028) for M in (7, LC.M_WRAP_BWD[0])]


@pytest.mark.parametrize("name,W,M", BWD_ALL, ids=[f"{n}-{W}-{M}" for n, W, M in BWD_ALL])
def test_backward_forms_at_tail_widths_one_block_and_the_persistent_wrap(K, name, W, M):
    """every instantiation the three backward entry points reach (ln_cases.FORMS) at W = 260 / 1028 (a 4-column tail behind one and
    behind four full column groups; 1028 are the IT >= 4 forms, the fp32 ones without a prefetched row) on 7 rows and on 4101 (the
    grid is capped at 2048 / 3072 / 4096 rows a trip: a second row for some wave of every variant): dx / dx_bf16 within the
    bound, dgamma / dbeta (accumulated into non-zero values) per column within ln_cols_check and bit-identical on a second run,
    results scattered through a row list only into the listed rows, the hybrid stream's CLS rows from their fp32 side arrays, the
    e4m3 copies per row and per tensor (the per-tensor backward of the delayed-scaling step), and the other outputs of a Q8 run
    equal to the plain run's"""
    form = LC.BWD_BY_NAME[name]
    period = {7: 7, 4101: 3}[M] if form["cls"] else 0
    ldin = 0 if M == 7 else 4
    worst, cols = LC.bwd_case(K, DEV, form, M, W, ldin, 4 - ldin, seed=M + W, period=period)
    _done(f"ln_bwd_edges[{name},{W},{M}]", worst, cols)


@pytest.mark.parametrize("W", LC.W_4COL)
def test_two_backward_forms_over_every_4_column_width(K, W):
    """fp32 x + fp32 res1 + bf16 res2 with both outputs, and the all-bf16 form with a bf16 res1, over all of W_4COL on 5 and 13
    rows, and on 8197 at the narrow widths"""
    worst, cols = 0.0, {}
    for i, form in enumerate((LC.FORM_F32_RES12, LC.FORM_ALL_BF16)):
        for M in (5, 13) + ((LC.M_WRAP_BWD[1],) if W in (4, 260) else ()):  # 8197: a third row for a wave of the 2048-row grids
            w, c = LC.bwd_case(K, DEV, form, M, W, 4 * (i ^ (M == 5)), 4 * i, seed=M + W)
            worst = max(worst, w)
            cols = {k: max(cols.get(k, 0.0), v) for k, v in c.items()}
    _done(f"ln_bwd_widths[{W}]", worst, cols)


@pytest.mark.parametrize("workspace", [True, False], ids=["workspace", "atomics"])
@pytest.mark.parametrize("W", LC.W_REDUCE)
@pytest.mark.parametrize("M", LC.M_REDUCE)
def test_dgamma_dbeta_over_every_partial_count_of_the_reduce_kernel(K, M, W, workspace):
    """ln_dgamma_reduce_kernel sums ceil(M / 4) per-block partials per column in 16 row groups, 8 loads in flight while
    b + 112 < nblocks: block counts with zero, one and two unrolled trips and every remainder shape, at widths whose last
    64-column block is cut by c < W; with the workspace (two runs, same bits) and without (one atomic per column per block);
    accumulated into non-zero initial values, every column within the derived bound"""
    assert -(-M // 4) in LC.REDUCE_NBLOCKS
    worst, cols = LC.bwd_case(K, DEV, LC.FORM_F32_RES12, M, W, 0, 4, seed=M + W, workspace=workspace)
    _done(f"ln_bwd_reduce[{M},{W},{'ws' if workspace else 'atomic'}]", worst, cols)


def test_backward_rows_past_the_m_argument_keep_their_poison(K):
    worst = 0.0
    for form, W in ((LC.FORM_F32_RES12, 260), (LC.BWD_BY_NAME["bwd_fp8-x16-dy16-r116-r2no-dxb-q8rows"], 1028)):
        w, cols = LC.bwd_case(K, DEV, form, 6, W, 4, 0, seed=W, extra=3)
        worst = max(worst, w)
    _done("ln_bwd_m_argument", worst, cols)


# ------------------------------------------------------------------------------------------------ the hybrid stream
HYBRID = [(p, c) for p in (1, 2, 5) for c in (1, 4, 5)]


@pytest.mark.parametrize("period,clips", HYBRID)
def test_hybrid_stream_periods_and_clip_counts(K, period, clips):
    """tvts_layernorm_{fwd,bwd}_cls at W = 260 (the 4-column CLS forward, plain and with the e4m3 copy) and W = 520 (the 8-column
    one) with period 1 (every row a CLS row), 2 and 5 on 1, 4 and 5 clips: stale stream rows (777) and stale res1 rows (-555) are
    never read; refresh=False leaves the stream's bits, refresh=True writes the rounding once; cls_dx within the fp32 bound; the
    CLS rows of dx_bf16 are its rounding; every other row has the bits of the plain kernel"""
    M = period * clips
    worst, cols = 0.0, {}
    for name, W in (("cls_4col", 260), ("cls_4col_q8rows", 260), ("cls_8col", 520), ("cls_8col_q8rows", 520)):
        for refresh in (True, False):
            worst = max(worst, LC.fwd_case(K, DEV, LC.FWD_BY_NAME[name], M, W, 0, 0, seed=M, period=period, refresh=refresh))
    for form in LC.FORMS:
        if form["cls"] and form["q8"] != "tensor":
            w, c = LC.bwd_case(K, DEV, form, M, 260, 0, 0, seed=M + 1, period=period)
            worst = max(worst, w)
            cols = {k: max(cols.get(k, 0.0), v) for k, v in c.items()}
    _done(f"ln_hybrid[{period},{clips}]", worst, cols)


@pytest.mark.parametrize("W", [8, 12])
def test_hybrid_stream_cls_launch_grid_wrap(K, W):
    """4101 clips of period 2: the CLS launch of the backward (one wave per CLS row, 1024 blocks at most) walks to a second row; the
    8-column (W = 8) and the 4-column (W = 12) CLS forward"""
    M = 2 * 4101
    ld = 0 if W == 8 else 4
    worst = LC.fwd_case(K, DEV, LC.FWD_BY_NAME["cls_8col" if W == 8 else "cls_4col"], M, W, ld, ld, seed=W, period=2)
    w, cols = LC.bwd_case(K, DEV, LC.BWD_BY_NAME["bwd_cls-x16-dy16-r116-r216-dxb-q8rows"], M, W, ld, ld, seed=W, period=2)
    _done(f"ln_hybrid_wrap[{W}]", max(worst, w), cols)


# ------------------------------------------------------------------------------------------------ the refusal table's baselines
@pytest.mark.parametrize("name", sorted(LC.BASELINES))
def test_every_baseline_of_the_refusal_table_launches(K, name):
    """tests/test_layernorm_args_cpu.py derives every refused call from one of these by changing ONE argument; each is a valid call:
    it returns 0, runs, and leaves finite results"""
    from tvts_amd import _lib
    lib, protos = _lib.load(), _lib.prototypes()
    keep = {}

    def alloc(m):
        t = m.tensor(DEV, seed=len(keep))
        keep[id(m)] = t
        return ctypes.c_void_p(t.data_ptr())

    rc = LC.call(lib, protos, name, alloc, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _, base = LC.BASELINES[name]
    for an in ("y", "dx", "dx_bf16", "cls_dx", "dgamma", "dbeta", "row_scale"):
        m = base.get(an)
        if isinstance(m, LC.Mat):
            assert bool(torch.isfinite(keep[id(m)].float()).all()), (name, an)
