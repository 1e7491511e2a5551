"""Every producer of e4m3 bytes against the independent encoder of tests/fp8_cases.py, byte for byte (run with -m gpu).

With arch["fp8_wgrad"] the producing kernels write the e4m3 bytes INSTEAD of the bf16 result, so the bytes are the only record of
an activation or a gradient.  The encode step exists six times (pack4_e4m3 of csrc/common.h in the three quantisers and the
LayerNorm kernels, Q8Out::emit8 and the two CLS kernels of attention.hip, patch_readout of gemm_nt256.h); here each site meets the
value ladder of fp8_cases.py -- every finite code, every rounding tie and its neighbours, the subnormal edges, signed zeros, values
past the range -- under power-of-two scales (where the expected byte cannot be argued with) and two others, with its outputs inside
guards.  Where values can be injected exactly (the quantisers, the LayerNorm backward through its residual, the GEMM through its
bias) the ladder itself is the input; where they cannot (LayerNorm forward, attention) the statement is that the bytes equal
encode_e4m3 of the bf16 result the kernel stored, and the test asserts that this result reaches saturation, the subnormal codes and
zero.  Further: the only-output forms (attention q8_only, GEMM store_out=False, LayerNorm y=None), the running-maximum accumulator
from every starting value, scale slots of 0.0 and -1.0 (quantise under 1.0), tvts_fp8_update_scales slot by slot, and +-Inf / NaN
inputs (+-448 and 0xFE at every site; see DESIGN.md, "Numerics")."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp8_cases as FC  # noqa: E402
import gemm_cases as GC  # noqa: E402
import kernel_bounds as KB  # noqa: E402
import ln_cases as LC  # noqa: E402

BF16, F32, U8 = FC.BF16, FC.F32, FC.U8
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def _slot(v=0.0):
    """one fp32 device scalar between two NaN guards -> (buffer, view)"""
    buf = torch.full((3,), NAN, device=DEV)
    buf[1] = v
    return buf, buf[1:2]


def _slot_ok(buf):
    return bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[2]))


def _view_of(x):
    """x (CPU) as a strided device view inside a NaN-poisoned buffer"""
    _, v = GC.poisoned(x.shape[0], x.shape[1], x.dtype, DEV)
    v.copy_(x.to(DEV))
    assert v.stride(0) > x.shape[1]
    return v


def _bytes_eq(q, want, what):
    KB.assert_equal_bits(q.cpu().contiguous(), want.contiguous(), what)


def _exact_max(x):
    return float(x.double().abs().max())


def _kinds(b):
    """(a saturated code, a subnormal code, a zero) among the bytes b"""
    m = b.flatten() & 0x7F
    return bool((m == 0x7E).any()), bool(((m >= 1) & (m <= 7)).any()), bool((m == 0).any())


LADDER = {dt: FC.ladder(dt) for dt in (BF16, F32)}
INRANGE = {dt: FC.ladder(dt, past=False) for dt in (BF16, F32)}


# ------------------------------------------------------------------------------------------------ tvts_amax / tvts_quant_fp8
@pytest.mark.parametrize("rows,cols", [(1, 8), (3, 1056), (2050, 8)])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_quant_fp8_bytes_and_scale_on_the_ladder(K, dtype, rows, cols):
    """the per-tensor quantiser on strided views: amax is the exact maximum, scale_out == fl32(amax / 448), the bytes those of
    encode_e4m3(x, fl32(1 / scale_out)); 2050 rows: past the 2048-block grid cap, the grid-stride loop runs.  The ladder starts at
    flat offset 3 (it straddles the 16-byte pieces a lane converts).  Then with a given, smaller amax (`amax_given`: the stale
    scale of the transposed shadow): the full ladder saturates at +-448."""
    for i, s in enumerate(FC.SCALES):
        what = f"quant_fp8 {dtype} [{rows},{cols}] scale {s:g}"
        x = FC.fill_cyclic(rows, cols, FC.scaled(INRANGE[dtype], s).roll(-37 * i), offset=3 if rows * cols > 8 else 0)
        xv = _view_of(x)
        qbuf, q = KB.guarded(rows, cols, U8, DEV)
        (ab, am), (sb, sc) = _slot(NAN), _slot(NAN)
        K.quantize_fp8(xv, q=q, scale=sc, amax=am)
        torch.cuda.synchronize()
        KB.check_guards(qbuf, rows, cols, what)
        assert _slot_ok(ab) and _slot_ok(sb), what
        assert float(am) == _exact_max(x), (what, float(am), _exact_max(x))
        assert float(sc) == FC.scale_of(float(am)), (what, float(sc), FC.scale_of(float(am)))
        if s in FC.POW2_SCALES and rows * cols > 1100:
            assert float(sc) == s, (what, float(sc))
        _bytes_eq(q, FC.encode_e4m3(x, FC.inv_of(float(sc))), what)
        # a stale maximum: everything past it saturates
        full = FC.fill_cyclic(rows, cols, FC.scaled(LADDER[dtype], s).roll(-37 * i), offset=3 if rows * cols > 8 else 0)
        (ab, am), (sb, sc) = _slot(FC.fl32(448.0 * s)), _slot(NAN)
        qbuf, q = KB.guarded(rows, cols, U8, DEV)
        K.quantize_fp8(_view_of(full), q=q, scale=sc, amax=am, amax_given=True)
        torch.cuda.synchronize()
        KB.check_guards(qbuf, rows, cols, what + " given amax")
        assert float(am) == FC.fl32(448.0 * s) and float(sc) == FC.scale_of(448.0 * s), what
        want = FC.encode_e4m3(full, FC.inv_of(float(sc)))
        _bytes_eq(q, want, what + " given amax")
        if rows * cols > 1100:
            assert _kinds(want) == (True, True, True) and not bool(((want & 0x7F) == 0x7F).any())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_amax_is_the_exact_maximum(K, dtype):
    """1030 rows (past the 1024-block cap) with the maximum in the last element of the last row; a -0 input and an all-zero
    input give +0.0; a start value left in the slot does not survive (the entry point resets it)"""
    x = FC.fill_cyclic(1030, 8, INRANGE[dtype], offset=3)
    for last in (452.0, -456.0):
        x[-1, -1] = last
        ab, am = _slot(1e9)
        _lib_amax(K, _view_of(x), am)
        assert float(am) == abs(last) and _slot_ok(ab), (float(am), last)
    for fill in (0.0, -0.0):
        z = torch.full((1030, 8), fill, dtype=dtype)
        ab, am = _slot(NAN)
        _lib_amax(K, _view_of(z), am)
        assert int(am.view(torch.int32)) == 0 and _slot_ok(ab), fill
    one = torch.tensor([[-0.0, 0.0, 2.0 ** -130, 0, 0, 0, 0, -2.0 ** -133]], dtype=dtype)  # one row; subnormals are not flushed
    ab, am = _slot(NAN)
    _lib_amax(K, _view_of(one), am)
    assert float(am) == 2.0 ** -130


def _lib_amax(K, x, am):
    from tvts_amd import _lib
    rc = _lib.load().tvts_amax(K._p(x), 1 if x.dtype == F32 else 0, x.stride(0), x.shape[0], x.shape[1], K._p(am), K._stream())
    assert rc == 0
    torch.cuda.synchronize()


def test_quant_fp8_multi_against_the_encoder(K):
    """the whole-table quantiser: a ladder tensor, a 1 x 4 tensor, an all-zero tensor (scale 1, zero bytes) and a tensor with a bf16
    transposed shadow one of whose elements rounds UP past the master's maximum (-> +-448 under the master's scale); bytes, amax,
    scale and scale_t against the encoder; a second call (stale amax slots) gives the same bits"""
    lad = FC.scaled(INRANGE[F32], FC.ODD_SCALES[1])
    big = 1.0 + 3 * 2.0 ** -9                        # bf16 rounds it up to 1 + 2^-7
    g = torch.Generator().manual_seed(5)
    sh = (torch.randn(16, 24, generator=g) * 0.3).clamp(-1, 1)
    sh[3, 5], sh[7, 2] = big, -big
    masters = [lad.view(8, -1).contiguous(), torch.tensor([[0.5, -3.0, 2.0 ** -140, -0.0]]), torch.zeros(12, 8), sh]
    shadows = [None, None, None, sh.t().contiguous().bfloat16()]
    assert float(shadows[3].float().abs().max()) > big
    scal = torch.full((3 * len(masters) + 2,), NAN, device=DEV)
    ents, outs = [], []
    for i, (w, wt) in enumerate(zip(masters, shadows)):
        qb, q = KB.guarded(w.shape[0], w.shape[1], U8, DEV, cols=0)
        qtb, qt = KB.guarded(wt.shape[0], wt.shape[1], U8, DEV, cols=0) if wt is not None else (None, None)
        ents.append((w.to(DEV), q, wt.to(DEV) if wt is not None else None, qt, scal[1 + 3 * i:2 + 3 * i], scal[2 + 3 * i:3 + 3 * i],
                     scal[3 + 3 * i:4 + 3 * i] if wt is not None else None))
        outs.append((qb, q, qtb, qt))
    table, n = K.quantize_fp8_multi_table(ents, DEV)
    first = None
    for call in range(2):
        K.quantize_fp8_multi(table, n)
        torch.cuda.synchronize()
        for i, (w, wt) in enumerate(zip(masters, shadows)):
            what = f"quant_fp8_multi tensor {i} call {call}"
            qb, q, qtb, qt = outs[i]
            am, sc = float(scal[1 + 3 * i]), float(scal[2 + 3 * i])
            assert am == _exact_max(w) and sc == FC.scale_of(am), (what, am, sc)
            _bytes_eq(q, FC.encode_e4m3(w, FC.inv_of(sc)), what)
            KB.check_guards(qb, w.shape[0], w.shape[1], what)
            if wt is not None:
                assert float(scal[3 + 3 * i]) == sc, what
                want = FC.encode_e4m3(wt, FC.inv_of(sc))
                _bytes_eq(qt, want, what + " shadow")
                assert int(want[5, 3]) == 0x7E and int(want[2, 7]) == 0xFE  # the rounded-up elements sit at +-448
                KB.check_guards(qtb, wt.shape[0], wt.shape[1], what + " shadow")
            else:
                assert bool(torch.isnan(scal[3 + 3 * i])), what + ": scale_t slot of a tensor without a shadow"
        assert float(scal[2 + 3 * 2]) == 1.0 and int(outs[2][1].max()) == 0
        assert bool(torch.isnan(scal[0])) and bool(torch.isnan(scal[-1]))
        state = [scal.clone()] + [o[1].clone() for o in outs] + [outs[3][3].clone()]
        if first is not None:
            for a_, b_ in zip(first, state):
                KB.assert_equal_bits(a_, b_, "quant_fp8_multi second call")
        first = state


# ------------------------------------------------------------------------------------------------ tvts_quant_fp8_rows
ROWS_CASES = [(1, 8), (4, 8), (5, 8), (32773, 8), (1, 5120), (4, 5120), (5, 5120), (1, 5128), (4, 5128), (5, 5128)]


@pytest.mark.parametrize("rows,cols", ROWS_CASES)
def test_quant_fp8_rows_per_row_mode(K, rows, cols):
    """one scale per row: every row carries +-448 * 2^k as its largest magnitude, so row_scale == 2^k exactly and the expected
    bytes are those of the ladder itself; an all-zero row gets scale 1 and zero bytes.  5120 columns: the last register-resident
    width, 5128 the first that is read twice; 32 773 rows: past 4 x 8192 waves, a wave walks two rows.  The accumulator (from 0)
    receives the tensor's maximum."""
    what = f"quant_fp8_rows per row [{rows},{cols}]"
    zr = 2 if rows >= 4 else None
    x, k = FC.row_ladders(rows, cols, zero_row=zr)
    qbuf, q = KB.guarded(rows, cols, U8, DEV)
    rs = LC.out_vec(rows, DEV)
    ab, am = _slot(0.0)
    K.quantize_fp8_rows(_view_of(x), q=q, row_scale=rs, amax=am)
    torch.cuda.synchronize()
    KB.check_guards(qbuf, rows, cols, what)
    assert bool(torch.isnan(rs[rows:]).all()) and _slot_ok(ab), what
    want_rs = torch.exp2(k.double()).float()
    KB.assert_equal_bits(rs[:rows].cpu(), want_rs, what + " row scales")
    want = FC.encode_e4m3(x, torch.exp2(-k.double()).float()[:, None])
    _bytes_eq(q, want, what)
    assert float(am) == _exact_max(x), what
    if zr is not None:
        assert float(rs[zr]) == 1.0 and int(q[zr].max()) == 0, what
    if rows * cols > 1100:
        assert len(set(want.flatten().tolist())) == 254, what + ": the case does not reach every finite code"


@pytest.mark.parametrize("rows,cols", [(32773, 8), (1, 5120), (5, 5120), (1, 5128), (5, 5128), (1, 8)])
def test_quant_fp8_rows_tensor_mode_saturates(K, rows, cols):
    """one scale for the tensor (`tscale`, last step's): the full ladder, values past 448 * tscale saturate at 0x7E / 0xFE and
    never reach the NaN codes; row_scale may be absent; the accumulator receives the exact maximum"""
    for i, s in enumerate(FC.SCALES):
        what = f"quant_fp8_rows tensor [{rows},{cols}] tscale {s:g}"
        x = FC.fill_cyclic(rows, cols, FC.scaled(LADDER[BF16], s).roll(-41 * i), offset=3 if cols > 8 or rows > 1 else 0)
        qbuf, q = KB.guarded(rows, cols, U8, DEV)
        (tb, ts), (ab, am) = _slot(s), _slot(0.0)
        _, rs = K.quantize_fp8_rows(_view_of(x), q=q, tscale=ts, amax=am)
        torch.cuda.synchronize()
        assert rs is None and _slot_ok(tb) and _slot_ok(ab) and float(ts) == s, what
        KB.check_guards(qbuf, rows, cols, what)
        want = FC.encode_e4m3(x, FC.inv_of(s))
        _bytes_eq(q, want, what)
        assert float(am) == _exact_max(x), what
        if rows * cols > 1100:
            assert _kinds(want) == (True, True, True) and len(set(want.flatten().tolist())) == 254, what


# ------------------------------------------------------------------------------------------------ the accumulator and the scale slot
def _preloads(m):
    """start values of a running maximum whose call adds the maximum m -> (start, expected result)"""
    return [(0.0, m), (m, m), (FC.fl32(m / 3), m), (FC.fl32(m * 2.5), FC.fl32(m * 2.5))]


def test_quant_fp8_rows_accumulator_and_zero_scale(K):
    x = FC.fill_cyclic(37, 264, LADDER[BF16][:-8], offset=5)   # (without the tail: the maximum is 1e4's bf16, not the type's)
    x[x.double().abs() > 1e4] = 0
    m = _exact_max(x)
    xv = _view_of(x)
    for mode in ("rows", "tensor"):
        for start, want in _preloads(m):
            ab, am = _slot(start)
            kw = dict(tscale=_slot(0.25)[1]) if mode == "tensor" else {}
            K.quantize_fp8_rows(xv, amax=am, **kw)
            assert float(am) == want and _slot_ok(ab), (mode, start, float(am), want)
    for s in (0.0, -1.0):   # a scale slot that is not positive: quantise under 1.0
        q, _ = K.quantize_fp8_rows(xv, tscale=_slot(s)[1])
        _bytes_eq(q, FC.encode_e4m3(x, 1.0), f"quant_fp8_rows tscale {s}")


@pytest.mark.parametrize("n", [1, 256, 257, 513])
def test_fp8_update_scales_slot_by_slot(K, n):
    """scale == fl32(amax / 448) exactly where amax > 0 (a subnormal amax included), a scale > 0 is kept where amax == 0, a scale
    of 0 (or below) becomes 1.0 there, every amax slot is 0 afterwards, and the slots past n are untouched.  Neighbouring slots are
    of different kinds, so a kernel that wrote slot i + 1 from slot i's amax fails."""
    g = torch.Generator().manual_seed(n)
    i = torch.arange(n + 8)
    kind = (i + i // 4) % 4
    amax = torch.where(kind == 0, torch.rand(n + 8, generator=g) * 900 + 0.01, torch.zeros(n + 8))
    amax = torch.where(kind == 3, torch.full((n + 8,), 2.0 ** -140), amax)
    scale = torch.where(kind == 2, torch.zeros(n + 8), torch.rand(n + 8, generator=g) + 0.5)
    if n > 1:
        scale[1 % n] = -1.0 if int(kind[1 % n]) in (1, 2) else scale[1 % n]
    a_dev, s_dev = amax.to(DEV), scale.to(DEV)
    from tvts_amd import _lib
    rc = _lib.load().tvts_fp8_update_scales(K._p(a_dev), K._p(s_dev), n, K._stream())
    torch.cuda.synchronize()
    assert rc == 0
    want = scale.clone()
    for j in range(n):
        a = float(amax[j])
        want[j] = FC.scale_of(a) if a > 0 else (float(scale[j]) if float(scale[j]) > 0 else 1.0)
    KB.assert_equal_bits(s_dev.cpu(), want, f"update_scales n={n} scales")
    want_a = amax.clone()
    want_a[:n] = 0.0
    KB.assert_equal_bits(a_dev.cpu(), want_a, f"update_scales n={n} amax")
    K.fp8_update_scales(a_dev[:n], s_dev[:n])   # a second step: nothing was produced, every scale is kept
    KB.assert_equal_bits(s_dev.cpu(), want, f"update_scales n={n} second call")


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_inputs(M, W, xdt, ts, seed):
    """rows whose normalised values spread over the columns, gamma = ts * (2^-8, 1, 2^9, 0) repeated: under tscale = ts the bytes
    of column 0 are subnormal codes, of column 2 saturated, of column 3 zero"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, W, generator=g) * torch.logspace(-2, 1, M)[:, None] + 0.3).to(xdt)
    gamma = (torch.tensor([2.0 ** -8, 1.0, 2.0 ** 9, 0.0]).repeat(W // 4) * ts).float()
    beta = torch.zeros(W)
    return x, gamma, beta


LN_FWD = [("f32", 4, 0, False), ("f32", 8, 0, False), ("f32", 260, 4, False), ("bf16_8col", 8, 0, False), ("bf16_8col", 8, 0, True),
          ("bf16_8col", 264, 0, True), ("bf16_4col", 12, 4, False), ("cls_8col", 8, 0, False), ("cls_8col", 8, 0, True),
          ("cls_4col", 12, 4, False)]


@pytest.mark.parametrize("form,W,ldmod,only", LN_FWD, ids=[f"{f}-{W}{'-only' if o else ''}" for f, W, _, o in LN_FWD])
@pytest.mark.parametrize("mode", ["tensor", "rows"])
def test_layernorm_forward_copies_are_the_encoder_on_the_stored_result(K, form, W, ldmod, only, mode):
    """every forward form with an e4m3 copy at the smallest widths of ln_cases.py (and one width past a column group): the bytes
    equal encode_e4m3 of the bf16 result the kernel stored (only=True, y = None: of the result the same kernel stores when it is
    given a y -- no pointer to a bf16 buffer reaches the launch at all), under a power-of-two tensor scale that makes the
    expected bytes hold a saturated code, a subnormal code and a zero (asserted), or under the row's own scale; the accumulator
    from every start value; scale slots 0.0 and -1.0"""
    M = 12 if form.startswith("cls") else 13
    ts = 2.0 ** -3
    xdt = F32 if form == "f32" else BF16
    x, gamma, beta = _ln_inputs(M, W, xdt, ts, seed=W + M)
    xin = LC.put(x.to(DEV), ldmod)
    gm, bt = LC.put_vec(gamma.to(DEV)), LC.put_vec(beta.to(DEV))
    kw = {}
    if form.startswith("cls"):
        period = 4
        cls_rows = torch.arange(0, M, period)
        kw = dict(cls_x=x[cls_rows].float().contiguous().to(DEV) * 1.25, cls_period=period, refresh=False)
    expect8 = xdt == BF16 and LC.ln8_ok(W, xin.stride(0), ldmod)
    assert expect8 == ("8col" in form), (form, W, ldmod)

    def run(tscale=None, amax=None, with_y=True):
        ybuf, y = LC.out_mat(M, W, BF16, DEV, ldmod)
        qbuf, q = LC.out_mat(M, W, U8, DEV, ldmod)
        rs = LC.out_vec(M, DEV)
        K.layernorm_fwd(xin, gm, bt, 1e-5, y if with_y else None, q8=q, row_scale=rs if tscale is None else None, tscale=tscale,
                        amax=amax, **kw)
        torch.cuda.synchronize()
        KB.check_guards(qbuf, M, W, f"ln fwd {form} q8")
        if with_y:
            KB.check_guards(ybuf, M, W, f"ln fwd {form} y")
        else:
            assert bool(torch.isnan(ybuf).all())
        return y.cpu(), q, rs

    what = f"ln fwd {form} [{M},{W}] {mode}{' only' if only else ''}"
    if mode == "rows":
        y, q, rs = run()
        am_rows = y.double().abs().amax(1)
        want_rs = torch.tensor([FC.scale_of(float(a)) for a in am_rows], dtype=F32)
        KB.assert_equal_bits(rs[:M].cpu(), want_rs, what + " row scales")
        inv = torch.tensor([FC.inv_of(float(s)) for s in want_rs], dtype=F32)[:, None]
        _bytes_eq(q, FC.encode_e4m3(y, inv), what)
        if only:
            _, q2, rs2 = run(with_y=False)
            KB.assert_equal_bits(q2.cpu(), q.cpu(), what); KB.assert_equal_bits(rs2.cpu(), rs.cpu(), what)
        return
    (tb, tsd), (ab, am) = _slot(ts), _slot(0.0)
    y, q, _ = run(tsd, am)
    want = FC.encode_e4m3(y, FC.inv_of(ts))
    assert _kinds(want) == (True, True, True), (what, "the inputs no longer reach saturation, a subnormal code and zero", _kinds(want))
    _bytes_eq(q, want, what)
    m = _exact_max(y)
    assert float(am) == m and _slot_ok(ab) and _slot_ok(tb), (what, float(am), m)
    for with_y in ((True, False) if only else (True,)):
        for start, res in _preloads(m):
            ab, am = _slot(start)
            _, q2, _ = run(tsd, am, with_y)
            assert float(am) == res and _slot_ok(ab), (what, with_y, start, float(am), res)
            _bytes_eq(q2, want, what + f" y={with_y} amax from {start}")
        for s in (0.0, -1.0):
            _, q2, _ = run(_slot(s)[1], None, with_y)
            _bytes_eq(q2, FC.encode_e4m3(y, 1.0), what + f" y={with_y} tscale {s}")


LN_BWD = [("f32", 4, 0), ("f32", 260, 4), ("bf16", 8, 0), ("cls", 8, 0)]


@pytest.mark.parametrize("form,W,ldmod", LN_BWD, ids=[f"{f}-{W}" for f, W, _ in LN_BWD])
def test_layernorm_backward_copies_meet_the_ladder_through_the_residual(K, form, W, ldmod):
    """the backward forms with an e4m3 copy.  With dy = 0 the result is the residual res1, so the ladder reaches the encode step
    exactly (fp32 x: fp32 res1; the hybrid-stream form: bf16 res1); the bf16-x form of tvts_layernorm_bwd_fp8 takes no residual and
    gets rows of dy that spread dx over the range instead.  Statement in every case: the bytes equal encode_e4m3 of the dx_bf16 the
    kernel stored, the expected bytes hold a saturated code, a subnormal code and a zero; per-row scales == fl32(amax / 448);
    the accumulator from every start value; scale slots 0.0 and -1.0"""
    ts = 2.0 ** 5
    lad = FC.scaled(LADDER[BF16], ts)
    lad = lad[lad.double().abs() < 1e30]
    M = -(-lad.numel() // W)
    if form == "cls":
        M += -M % 4
    g = torch.Generator().manual_seed(W)
    xdt = F32 if form == "f32" else BF16
    x = (torch.randn(M, W, generator=g) + 0.1).to(xdt)
    xin = LC.put(x.to(DEV), ldmod)
    gamma = LC.put_vec((1 + 0.1 * torch.randn(W, generator=g)).to(DEV))
    mean, rstd = LC.out_vec(M, DEV), LC.out_vec(M, DEV)
    K.layernorm_fwd(xin, gamma, LC.put_vec(torch.zeros(W, device=DEV)), 1e-5, torch.empty(M, W, dtype=xdt, device=DEV), mean, rstd)
    kw = {}
    if form == "bf16":
        dy = torch.randn(M, W, generator=g) * torch.logspace(-6, 5, M)[:, None]
        dy[3] = 0.0
        res = None
    else:
        dy = torch.zeros(M, W)
        res = FC.fill_cyclic(M, W, lad, offset=0).to(F32 if form == "f32" else BF16)
        kw["res1"] = LC.put(res.to(DEV), ldmod)
    if form == "cls":
        kw.update(cls_period=4)
    dyv = LC.put(dy.bfloat16().to(DEV), ldmod)

    def run(tscale=None, amax=None):
        bbuf, dxb = LC.out_mat(M, W, BF16, DEV, ldmod)
        qbuf, q = LC.out_mat(M, W, U8, DEV, ldmod)
        rs = LC.out_vec(M, DEV)
        K.layernorm_bwd(dyv, xin, mean, rstd, gamma, None, dx_bf16=dxb, q8=q, row_scale=rs if tscale is None else None, tscale=tscale,
                        amax=amax, **kw)
        torch.cuda.synchronize()
        KB.check_guards(qbuf, M, W, f"ln bwd {form} q8"); KB.check_guards(bbuf, M, W, f"ln bwd {form} dx_bf16")
        return dxb.cpu(), q, rs

    what = f"ln bwd {form} [{M},{W}]"
    (tb, tsd), (ab, am) = _slot(ts), _slot(0.0)
    d16, q, _ = run(tsd, am)
    if res is not None:   # the injection worked: the stored result is the ladder (the sign of a zero aside)
        assert torch.equal(d16.double(), res.double()), what + ": dx_bf16 is not the residual"
    want = FC.encode_e4m3(d16, FC.inv_of(ts))
    assert _kinds(want) == (True, True, True), (what, _kinds(want))
    if res is not None:
        assert len(set(want.flatten().tolist()) | {0x80}) == 254, what + ": the case does not reach every finite code"
    _bytes_eq(q, want, what)
    m = _exact_max(d16)
    assert float(am) == m and _slot_ok(ab) and _slot_ok(tb), (what, float(am), m)
    for start, r in _preloads(m):
        ab, am = _slot(start)
        run(tsd, am)
        assert float(am) == r and _slot_ok(ab), (what, start, float(am), r)
    for s in (0.0, -1.0):
        _, q2, _ = run(_slot(s)[1])
        _bytes_eq(q2, FC.encode_e4m3(d16, 1.0), what + f" tscale {s}")
    d16, q, rs = run()
    am_rows = d16.double().abs().amax(1)
    want_rs = torch.tensor([FC.scale_of(float(a)) for a in am_rows], dtype=F32)
    KB.assert_equal_bits(rs[:M].cpu(), want_rs, what + " row scales")
    _bytes_eq(q, FC.encode_e4m3(d16, torch.tensor([FC.inv_of(float(s)) for s in want_rs], dtype=F32)[:, None]), what + " per row")


# ------------------------------------------------------------------------------------------------ GEMM epilogue
GM, GN, GK = 257, 264, 128   # the edge shape of the e4m3 GEMM's tests: rows and columns sticking out of the tiles


def _e4m3_bytes(t):
    return t.to(torch.float8_e4m3fn).view(U8)


def _gemm_run(K, a8, sa, b8, sb, kw, ts, am0, store_out, preact=False):
    obuf, out = KB.guarded(GM, GN, BF16, DEV)
    obuf.fill_(7.0)   # (a recognisable pattern: the only-output form must leave all of it)
    qbuf, q = KB.guarded(GM, GN, U8, DEV)
    assert a8.shape[0] == GM and b8.shape[0] == GN
    (tb, tsd), (ab, am) = _slot(ts), _slot(am0)
    pre = torch.empty(GM, GN, dtype=BF16, device=DEV) if preact else None
    K.gemm_nt_fp8(a8, sa, b8, sb, out, preact=pre, q8out=q, q8_scale=tsd, q8_amax=am, store_out=store_out, **kw)
    torch.cuda.synchronize()
    KB.check_guards(qbuf, GM, GN, "gemm q8out")
    assert _slot_ok(tb) and _slot_ok(ab)
    if store_out:
        assert bool((obuf[GM:] == 7.0).all()) and bool((obuf[:GM, GN:] == 7.0).all()), "gemm out guards"
    else:
        assert bool((obuf == 7.0).all()), "store_out=False wrote the bf16 buffer"
    return out.cpu(), q.cpu(), float(am)


def test_gemm_epilogue_copy_meets_the_ladder_through_the_bias(K):
    """The e4m3-copy forms of tvts_gemm_nt_fp8 refuse a residual (-22: they exist for the GELU and gate epilogues only), so the
    values enter through the bias: with an all-zero a8 the accumulator is 0 and out = gelu(bias), and erf-GELU is the identity in
    fp32 from 8 upwards (the test asserts out == bias).  The positive half of the ladder times 2^14, under tscale = 2^14, in
    column chunks of 264; every row of the 257 carries the same values, so a wrong byte offset in any tile row shows.  Both
    store_out settings give the encoder's bytes (the fp32 results are bf16 values: no second rounding) and the exact amax."""
    ts = 2.0 ** 14
    pos = LADDER[BF16][(LADDER[BF16].double() > 2.0 ** -11) & (LADDER[BF16].double() < 1e30)]   # (from just under the first tie)
    vals = FC.scaled(pos, ts).float()
    assert float(vals.min()) >= 8.0
    a8 = torch.zeros(GM, GK, dtype=U8, device=DEV)
    g = torch.Generator().manual_seed(3)
    b8 = _e4m3_bytes(torch.randn(GN, GK, generator=g)).to(DEV)
    sa, sb = torch.ones(1, device=DEV), torch.ones(1, device=DEV)
    seen = set()
    for c0 in range(0, vals.numel(), GN):
        chunk = vals[c0:c0 + GN]
        bias = torch.cat([chunk, vals[:GN - chunk.numel()]])
        want_row = FC.encode_e4m3(bias, FC.inv_of(ts))
        seen |= set(want_row.tolist())
        for store_out in (True, False):
            what = f"gemm q8out bias ladder chunk {c0} store_out={store_out}"
            out, q, am = _gemm_run(K, a8, sa, b8, sb, dict(bias=bias.to(DEV), act="gelu"), ts, 0.0, store_out)
            if store_out:
                assert torch.equal(out.float(), bias[None, :].expand(GM, GN)), what + ": gelu(bias) is not the bias"
            KB.assert_equal_bits(q, want_row[None, :].expand(GM, GN).contiguous(), what)
            assert am == float(bias.max()), (what, am)
    assert seen == set(range(0, 0x7F)), "the chunks do not reach every positive code"


@pytest.mark.parametrize("Kd", [128, 512])
@pytest.mark.parametrize("form", ["gelu", "quick_gelu", "gate_gelu", "gate_quick_gelu"])
def test_gemm_epilogue_copy_is_the_encoder_on_the_stored_result(K, form, Kd):
    """every e4m3-copy instantiation at the edge shape (K = 128: the short contraction whose fragments are decoded to bf16; K = 512:
    the scaled-MFMA loop) on ordinary operands, under a power-of-two scale that makes the bytes
    hold a saturated code, a subnormal code and a zero (asserted).  store_out=True: the bytes equal encode_e4m3 of the stored
    bf16, amax is its exact maximum.  store_out=False (the copy is quantised from the fp32 result, no bf16 tensor is written and
    the buffer keeps its pattern): within one e4m3 code of that, and every byte lies between the encoder's bytes of the two ends
    of the interval of fp32 values that round to the stored bf16 -- a byte that differs belongs to a value whose bf16 rounding
    moved it across a code boundary; amax rounds to the stored form's.  The accumulator from every start value, scale 0 / -1."""
    g = torch.Generator().manual_seed(11)
    a8 = _e4m3_bytes(torch.randn(GM, Kd, generator=g) * torch.logspace(-3, 1, GM)[:, None]).to(DEV)
    a8[5] = 0   # a zero row: out = act(bias) / exactly 0 in the gate forms
    b8 = _e4m3_bytes(torch.randn(GN, Kd, generator=g)).to(DEV)
    sa, sb = torch.tensor([1.0], device=DEV), torch.tensor([2.0 ** -6], device=DEV)
    if form.startswith("gate"):
        h = (torch.randn(GM, GN, generator=g) * 1.5).bfloat16().to(DEV)
        kw = dict(gate_h=LC.put(h), gate_act=form[5:])
    else:
        kw = dict(bias=(torch.randn(GN, generator=g) * 0.01).to(DEV), act=form)
        kw["bias"][::7] = 0.0   # zero row x zero bias: act(0) = 0
    ts = 2.0 ** -9
    what = f"gemm q8out {form} K={Kd}"
    out, q, am = _gemm_run(K, a8, sa, b8, sb, kw, ts, 0.0, True, preact=not form.startswith("gate"))
    want = FC.encode_e4m3(out, FC.inv_of(ts))
    assert _kinds(want) == (True, True, True), (what, _kinds(want))
    KB.assert_equal_bits(q, want, what)
    m = _exact_max(out)
    assert am == m, (what, am, m)
    for start, r in _preloads(m):
        _, q2, am2 = _gemm_run(K, a8, sa, b8, sb, kw, ts, start, True)
        assert am2 == r, (what, start, am2, r)
        KB.assert_equal_bits(q2, want, what + f" amax from {start}")
    for s in (0.0, -1.0):
        for store_out in (True, False):
            out1, q2, _ = _gemm_run(K, a8, sa, b8, sb, kw, s, 0.0, store_out)
            if store_out:
                KB.assert_equal_bits(out1, out, what)
                KB.assert_equal_bits(q2, FC.encode_e4m3(out, 1.0), what + f" scale {s}")
    # the only-output form
    _, q2, am2 = _gemm_run(K, a8, sa, b8, sb, kw, ts, 0.0, False)
    o64 = out.double()
    ulp = torch.exp2(torch.floor(torch.log2(o64.abs().clamp_min(2.0 ** -126))) - 7)   # bf16 spacing at the stored value
    lo, hi = (o64 - ulp / 2).float(), (o64 + ulp / 2).float()                          # fp32 values that can round to it
    d_lo, d_hi = KB.decode_e4m3(FC.encode_e4m3(lo, FC.inv_of(ts))), KB.decode_e4m3(FC.encode_e4m3(hi, FC.inv_of(ts)))
    d1, d2 = KB.decode_e4m3(want), KB.decode_e4m3(q2)
    assert bool(torch.isfinite(d2).all())
    bad = (d2 < d_lo) | (d2 > d_hi)
    assert not bool(bad.any()), (what, "store_out=False bytes outside the bf16 rounding interval", int(bad.sum()),
                                 torch.nonzero(bad)[0].tolist())
    spacing = torch.exp2(torch.floor(torch.log2(torch.maximum(d1.abs(), d2.abs()).clamp_min(2.0 ** -6))) - 3)
    KB.assert_within(d2, d1, spacing, what + " store_out=False (one e4m3 code)")
    assert float(torch.tensor(am2).bfloat16()) == m, (what, am2, m)
    for start, r in _preloads(am2):
        _, _, am3 = _gemm_run(K, a8, sa, b8, sb, kw, ts, start, False)
        assert am3 == r, (what, "store_out=False", start, am3, r)


# ------------------------------------------------------------------------------------------------ fused divided attention
SPACE = [("space", 2, n) for n in (15, 16, 47, 96, 111)]          # MT 1 full; MT 2, one row in its last tile; MT 3 full; MT 7 ragged / full
TIME = [("time", T, n) for T in (15, 16, 19, 20, 31) for n in (5, 29)]  # MT 1 full; the 20-row form (twice); the 32-row form; the limit
ATTN = SPACE + TIME                                                 # n = 29: two TIME chunks, the second of one patch


def _attn_case(mode, T, n, dh, seed):
    B, heads = 2, 2
    S, W = 1 + T * n, heads * dh
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3 * W, generator=g).bfloat16().to(DEV)
    dO = torch.randn(B * S, W, generator=g).bfloat16().to(DEV)
    return B, heads, S, W, qkv, dO


def _attn_fwd(K, mode, T, n, dh, qkv, B, heads, S, W, ts, am0, q8_only=False):
    obuf, out = KB.guarded(B * S, W, BF16, DEV)
    obuf.fill_(7.0)
    qbuf, q = KB.guarded(B * S, W, U8, DEV)
    lse = torch.full((B * S, heads), NAN, device=DEV)
    ws = torch.full((B * heads * max(T, -(-n // 28)) * (dh + 2),), NAN, device=DEV)
    (tb, tsd), (ab, am) = _slot(ts), _slot(am0)
    K.attn_fwd_divided(mode, qkv, out, lse, ws, B=B, heads=heads, S=S, T=T, n=n, head_dim=dh, q8out=q, q8_scale=tsd, q8_amax=am,
                       q8_only=q8_only)
    torch.cuda.synchronize()
    KB.check_guards(qbuf, B * S, W, "attention fwd q8")
    assert bool((obuf[B * S:] == 7.0).all()) and bool((obuf[:B * S, W:] == 7.0).all()) and _slot_ok(tb) and _slot_ok(ab)
    return out, q.cpu(), float(am), lse, ws


def _attn_bwd(K, mode, T, n, dh, qkv, dO, O, lse, B, heads, S, W, ts, am0, q8_only=False):
    dbuf, dqkv = KB.guarded(B * S, 3 * W, BF16, DEV)
    dbuf.fill_(7.0)
    qbuf, q = KB.guarded(B * S, 3 * W, U8, DEV)
    delta = torch.full((B * S, heads), NAN, device=DEV)
    parts = max(T, -(-n // 28))
    acc = torch.full((B, heads, parts, 3, dh), NAN, device=DEV)
    (tb, tsd), (ab, am) = _slot(ts), _slot(am0)
    K.attn_bwd(mode, qkv, dO, O, lse, delta, dqkv, B=B, heads=heads, S=S, T=T, n=n, cls_acc=acc, head_dim=dh, q8out=q, q8_scale=tsd,
               q8_amax=am, q8_only=q8_only)
    torch.cuda.synchronize()
    KB.check_guards(qbuf, B * S, 3 * W, "attention bwd q8")
    assert bool((dbuf[B * S:] == 7.0).all()) and bool((dbuf[:B * S, 3 * W:] == 7.0).all()) and _slot_ok(tb) and _slot_ok(ab)
    return dqkv, q.cpu(), float(am), delta, acc


@pytest.mark.parametrize("mode,T,n", ATTN, ids=[f"{m}-T{T}-n{n}" for m, T, n in ATTN])
@pytest.mark.parametrize("dh", [64, 80])
def test_fused_attention_copies_at_every_instantiation(K, mode, T, n, dh):
    """the smallest geometry of every instantiation of the fused divided kernels (SPACE by MT = ceil((n + 1) / 16), TIME by
    MT = ceil((T + 1) / 16) and the 20-row store form), forward and backward, both head dimensions, B = 2, 2 heads.  The bytes of
    every row -- the CLS rows come from the one-byte sites of attn_cls_merge_kernel / attn_cls_finalize_kernel -- equal
    encode_e4m3 of the stored bf16 result under a scale that saturates part of it and under one that reaches the subnormal
    codes; amax is the exact maximum.  With q8_only the same bytes and maximum, the CLS rows of the bf16 buffer as in the other
    run, its patch rows untouched, and lse2 / delta / the CLS accumulators bit-equal."""
    B, heads, S, W, qkv, dO = _attn_case(mode, T, n, dh, seed=T * 1000 + n + dh)
    what = f"attention {mode} T={T} n={n} dh={dh}"
    cls = torch.arange(B, device=DEV) * S
    patch = torch.ones(B * S, dtype=torch.bool, device=DEV); patch[cls] = False
    O = None
    for ts, kinds in ((2.0 ** -10, (True, False, False)), (2.0 ** 3, (False, True, True))):
        out, q, am, lse, ws = _attn_fwd(K, mode, T, n, dh, qkv, B, heads, S, W, ts, 0.0)
        o = out.cpu()
        want = FC.encode_e4m3(o, FC.inv_of(ts))
        got_kinds = _kinds(want)
        assert all(g or not k for g, k in zip(got_kinds, kinds)), (what, "forward edge coverage", ts, got_kinds)
        KB.assert_equal_bits(q, want, what + f" forward, scale {ts:g}")
        assert am == _exact_max(o), (what, am, _exact_max(o))
        out2, q2, am2, lse2, ws2 = _attn_fwd(K, mode, T, n, dh, qkv, B, heads, S, W, ts, 0.0, q8_only=True)
        KB.assert_equal_bits(q2, q, what + " forward q8_only bytes")
        assert am2 == am, (what, am2, am)
        KB.assert_equal_bits(out2[cls], out[cls], what + " forward q8_only CLS rows")
        assert bool((out2[patch] == 7.0).all()), what + ": q8_only wrote bf16 patch rows"
        KB.assert_equal_bits(lse2, lse, what + " lse2"); KB.assert_equal_bits(ws2, ws, what + " cls workspace")
        O, L = out, lse
        dqkv, q, am, delta, acc = _attn_bwd(K, mode, T, n, dh, qkv, dO, O, L, B, heads, S, W, ts, 0.0)
        d = dqkv.cpu()
        want = FC.encode_e4m3(d, FC.inv_of(ts))
        got_kinds = _kinds(want)
        assert all(g or not k for g, k in zip(got_kinds, kinds)), (what, "backward edge coverage", ts, got_kinds)
        KB.assert_equal_bits(q, want, what + f" backward, scale {ts:g}")
        assert am == _exact_max(d), (what, am, _exact_max(d))
        dqkv2, q2, am2, delta2, acc2 = _attn_bwd(K, mode, T, n, dh, qkv, dO, O, L, B, heads, S, W, ts, 0.0, q8_only=True)
        KB.assert_equal_bits(q2, q, what + " backward q8_only bytes")
        assert am2 == am, (what, am2, am)
        KB.assert_equal_bits(dqkv2[cls], dqkv[cls], what + " backward q8_only CLS rows")
        assert bool((dqkv2[patch] == 7.0).all()), what + ": q8_only wrote bf16 patch rows of dqkv"
        KB.assert_equal_bits(delta2, delta, what + " delta"); KB.assert_equal_bits(acc2, acc, what + " cls accumulators")


@pytest.mark.parametrize("mode,T,n,dh", [("space", 2, 16, 64), ("time", 16, 29, 80)])
def test_fused_attention_accumulator_and_zero_scale(K, mode, T, n, dh):
    """the running maximum from every start value, forward and backward (patch kernels and the CLS merge / finalize kernels publish
    into the same slot), and scale slots 0.0 / -1.0: the bytes of the encoder under 1.0, CLS rows included"""
    B, heads, S, W, qkv, dO = _attn_case(mode, T, n, dh, seed=77)
    out, _, m, lse, _ = _attn_fwd(K, mode, T, n, dh, qkv, B, heads, S, W, 0.01, 0.0)
    dqkv, _, md, _, _ = _attn_bwd(K, mode, T, n, dh, qkv, dO, out, lse, B, heads, S, W, 0.01, 0.0)
    assert m == _exact_max(out.cpu()) and md == _exact_max(dqkv.cpu())
    for start, r in _preloads(m):
        assert _attn_fwd(K, mode, T, n, dh, qkv, B, heads, S, W, 0.01, start)[2] == r, ("forward", start)
    for start, r in _preloads(md):
        assert _attn_bwd(K, mode, T, n, dh, qkv, dO, out, lse, B, heads, S, W, 0.01, start)[2] == r, ("backward", start)
    big_q, big_d = (qkv.float() * 1).bfloat16(), (dO.float() * 64).bfloat16()
    big_q[:, 2 * W:] = (big_q[:, 2 * W:].float() * 64).bfloat16()   # V times 64: outputs of a few tens, codes far from zero under 1.0
    for s in (0.0, -1.0):
        o, q, _, l, _ = _attn_fwd(K, mode, T, n, dh, big_q, B, heads, S, W, s, 0.0)
        KB.assert_equal_bits(q, FC.encode_e4m3(o.cpu(), 1.0), f"attention {mode} forward scale {s}")
        d, q, _, _, _ = _attn_bwd(K, mode, T, n, dh, big_q, big_d, o, l, B, heads, S, W, s, 0.0)
        KB.assert_equal_bits(q, FC.encode_e4m3(d.cpu(), 1.0), f"attention {mode} backward scale {s}")
        assert len(set(q.flatten().tolist())) > 60
    # the one-byte sites at their clamp: under 2^-9 the CLS rows of these results reach +-448 (asserted)
    ts = 2.0 ** -9
    cls = (torch.arange(B) * S).tolist()
    o, q, _, l, _ = _attn_fwd(K, mode, T, n, dh, big_q, B, heads, S, W, ts, 0.0)
    want = FC.encode_e4m3(o.cpu(), FC.inv_of(ts))
    assert _kinds(want[cls])[0], "no CLS output saturates"
    KB.assert_equal_bits(q, want, f"attention {mode} forward, saturating CLS rows")
    d, q, _, _, _ = _attn_bwd(K, mode, T, n, dh, big_q, big_d, o, l, B, heads, S, W, ts, 0.0)
    want = FC.encode_e4m3(d.cpu(), FC.inv_of(ts))
    assert _kinds(want[cls])[0], "no CLS gradient saturates"
    KB.assert_equal_bits(q, want, f"attention {mode} backward, saturating CLS rows")


# ------------------------------------------------------------------------------------------------ non-finite inputs
def _nonfinite_checks(stored, q, am, what):
    """+Inf -> 0x7E, -Inf -> 0xFE, NaN -> 0xFE wherever the stored value is one of them; the rest as the encoder; the running
    maximum is +Inf (a NaN never enters it: fmaxf(m, |NaN|) is m)"""
    s = stored.cpu().double()
    q = q.cpu()
    assert bool(torch.isposinf(s).any()) and bool(torch.isneginf(s).any()) and bool(torch.isnan(s).any()), what + ": an input did not arrive"
    assert bool((q[torch.isposinf(s)] == 0x7E).all()), what + ": +Inf"
    assert bool((q[torch.isneginf(s)] == 0xFE).all()), what + ": -Inf"
    assert bool((q[torch.isnan(s)] == FC.NAN_BYTE).all()), (what + ": NaN", sorted(set(q[torch.isnan(s)].tolist())))
    if am is not None:
        assert am == INF, (what, am)


def _with_nonfinite(x):
    x = x.clone()
    x[0, 1], x[1, 6], x[2, 3] = INF, -INF, NAN
    x[-1, -1], x[-1, 0], x[-2, 4] = -INF, NAN, INF
    return x


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_non_finite_inputs_of_the_quantisers(K, dtype):
    s = 2.0 ** -3
    x = _with_nonfinite(FC.fill_cyclic(9, 264, FC.scaled(INRANGE[dtype], s), offset=3))
    want = FC.encode_e4m3(x, FC.inv_of(s))
    (ab, am) = _slot(FC.fl32(448.0 * s))
    q, sc = K.quantize_fp8(_view_of(x), amax=am, amax_given=True)
    assert float(sc) == s
    _bytes_eq(q, want, f"quant_fp8 {dtype} non-finite")
    _nonfinite_checks(x, q, None, f"quant_fp8 {dtype}")
    ab, am = _slot(0.0)
    _lib_amax(K, _view_of(x), am)
    assert float(am) == INF                                          # tvts_amax: +Inf; a NaN is skipped
    xn = x.clone(); xn[torch.isinf(xn)] = 1.0
    _lib_amax(K, _view_of(xn), am)
    assert float(am) == 448.0 * s, float(am)
    if dtype == BF16:
        for mode in ("tensor",):
            ab, am = _slot(0.0)
            q, _ = K.quantize_fp8_rows(_view_of(x), tscale=_slot(s)[1], amax=am)
            _bytes_eq(q, want, "quant_fp8_rows non-finite")
            _nonfinite_checks(x, q, float(am), "quant_fp8_rows")
    else:  # tvts_quant_fp8_multi derives its scale from the master: the non-finite values enter through the bf16 shadow
        w = FC.fill_cyclic(24, 16, FC.scaled(INRANGE[F32], s), offset=1)
        wt = _with_nonfinite(w.t().contiguous().bfloat16())
        scal = torch.full((3,), NAN, device=DEV)
        q8, qt = torch.empty(24, 16, dtype=U8, device=DEV), torch.empty(16, 24, dtype=U8, device=DEV)
        table, n = K.quantize_fp8_multi_table([(w.to(DEV), q8, wt.to(DEV), qt, scal[0:1], scal[1:2], scal[2:3])], DEV)
        K.quantize_fp8_multi(table, n)
        assert float(scal[1]) == s and float(scal[0]) == 448.0 * s
        _bytes_eq(qt, FC.encode_e4m3(wt, FC.inv_of(s)), "quant_fp8_multi shadow non-finite")
        _nonfinite_checks(wt, qt, None, "quant_fp8_multi shadow")


def test_non_finite_inputs_of_the_gemm_epilogue(K):
    """through the per-row scale of the a8 operand in the gate form: acc = 128 (every operand byte is e4m3 1.0), gelu'(10) = 1 in
    fp32, so out[m, :] = 128 * sa[m]: rows of +Inf, -Inf and NaN beside finite ones.  (+Inf also through the bias of the GELU
    form: gelu(+Inf) = +Inf.)  Both store_out settings."""
    a8 = torch.full((GM, GK), 0x38, dtype=U8, device=DEV)
    b8 = torch.full((GN, GK), 0x38, dtype=U8, device=DEV)
    sa = torch.logspace(-3, 1, GM)
    sa[0], sa[100], sa[255], sa[256] = INF, -INF, NAN, -INF
    h = torch.full((GM, GN), 10.0, dtype=BF16, device=DEV)
    ts = 2.0 ** 3
    for store_out in (True, False):
        out, q, am = _gemm_run(K, a8, sa.to(DEV), b8, torch.ones(1, device=DEV), dict(gate_h=h, gate_act="gelu"), ts, 0.0, store_out)
        stored = (128.0 * sa)[:, None].expand(GM, GN).bfloat16()
        if store_out:
            assert torch.equal(torch.isnan(out), torch.isnan(stored)) and torch.equal(torch.nan_to_num(out.double()), torch.nan_to_num(stored.double()))
        seen = stored if store_out else (128.0 * sa)[:, None].expand(GM, GN)   # (alone, the copy is made of the fp32 result)
        KB.assert_equal_bits(q, FC.encode_e4m3(seen, FC.inv_of(ts)).contiguous(), f"gemm non-finite bytes store_out={store_out}")
        _nonfinite_checks(stored, q, am, f"gemm gate store_out={store_out}")
    bias = torch.linspace(16, 600, GN)
    bias[3], bias[GN - 1] = INF, INF
    for store_out in (True, False):
        _, q, am = _gemm_run(K, torch.zeros(GM, GK, dtype=U8, device=DEV), torch.ones(1, device=DEV), b8, torch.ones(1, device=DEV),
                             dict(bias=bias.to(DEV), act="gelu"), 1.0, 0.0, store_out)
        assert am == INF and bool((q[:, 3] == 0x7E).all()) and bool((q[:, GN - 1] == 0x7E).all())


def test_non_finite_inputs_of_the_layernorm_forms(K):
    """forward: +-Inf through beta (y = +-Inf in those columns), rows of x that hold +Inf / -Inf / NaN (every element of such a row
    is NaN: the mean is not finite); backward: +-Inf / NaN elements of the residual under dy = 0, and a row of dy that holds +Inf
    (NaN throughout)"""
    ts = 2.0 ** -3
    for xdt, W in ((F32, 260), (BF16, 264)):
        M = 9
        x, gamma, beta = _ln_inputs(M, W, xdt, ts, seed=W)
        x[2, 5], x[4, W - 1], x[6, 0] = INF, -INF, NAN
        beta[3], beta[W - 3] = INF, -INF
        for with_y in ((True, False) if xdt == BF16 else (True,)):
            ybuf, y = LC.out_mat(M, W, BF16, DEV)
            qbuf, q = LC.out_mat(M, W, U8, DEV)
            ab, am = _slot(0.0)
            args = (LC.put(x.to(DEV)), LC.put_vec(gamma.to(DEV)), LC.put_vec(beta.to(DEV)), 1e-5)
            K.layernorm_fwd(*args, y, q8=q, tscale=_slot(ts)[1], amax=am)
            stored = y.cpu()
            if not with_y:
                ab, am = _slot(0.0)
                qbuf, q = LC.out_mat(M, W, U8, DEV)
                K.layernorm_fwd(*args, None, q8=q, tscale=_slot(ts)[1], amax=am)
            what = f"ln fwd {xdt} y={with_y} non-finite"
            assert bool(torch.isnan(stored[[2, 4, 6]]).all()), what
            _bytes_eq(q, FC.encode_e4m3(stored, FC.inv_of(ts)), what)
            _nonfinite_checks(stored, q, float(am), what)
            KB.check_guards(qbuf, M, W, what)
    # backward, fp32 x with an fp32 residual
    M, W = 9, 260
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, W, generator=g)
    xin, gamma = LC.put(x.to(DEV)), LC.put_vec(torch.ones(W, device=DEV))
    mean, rstd = LC.out_vec(M, DEV), LC.out_vec(M, DEV)
    K.layernorm_fwd(xin, gamma, LC.put_vec(torch.zeros(W, device=DEV)), 1e-5, torch.empty(M, W, device=DEV), mean, rstd)
    res = _with_nonfinite(FC.fill_cyclic(M, W, FC.scaled(INRANGE[BF16], ts), offset=3).float())
    dy = torch.zeros(M, W)
    dy[5, 7] = INF
    bbuf, dxb = LC.out_mat(M, W, BF16, DEV)
    qbuf, q = LC.out_mat(M, W, U8, DEV)
    ab, am = _slot(0.0)
    K.layernorm_bwd(LC.put(dy.bfloat16().to(DEV)), xin, mean, rstd, gamma, None, dx_bf16=dxb, res1=LC.put(res.to(DEV)), q8=q,
                    tscale=_slot(ts)[1], amax=am)
    stored = dxb.cpu()
    keep = torch.ones(M, dtype=torch.bool); keep[5] = False
    assert torch.equal(torch.nan_to_num(stored[keep].double(), nan=-7.0), torch.nan_to_num(res[keep].double(), nan=-7.0))
    _bytes_eq(q, FC.encode_e4m3(stored, FC.inv_of(ts)), "ln bwd non-finite")
    _nonfinite_checks(stored, q, float(am), "ln bwd")


# ------------------------------------------------------------------------------------------------ the refusal baselines run
def test_every_refusal_baseline_is_a_valid_call(K):
    """each baseline of fp8_cases.BASELINES launches and returns 0, so a refusal of tests/test_fp8_cases_cpu.py cannot pass because
    some other argument of its call was wrong as well"""
    from tvts_amd import _lib
    lib, protos = _lib.load(), _lib.prototypes()
    keep = []

    def alloc(m):
        if isinstance(m, str):   # a table of two small weights
            ents = []
            for _ in range(2):
                t = [torch.randn(4, 8, device=DEV), torch.empty(4, 8, dtype=U8, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)]
                keep.extend(t)
                ents.append((t[0], t[1], None, None, t[2], t[3], None))
            t, _ = K.quantize_fp8_multi_table(ents, DEV)
        else:
            t = m.tensor(DEV, seed=len(keep))
        keep.append(t)
        return ctypes.c_void_p(t.data_ptr())

    for name in FC.BASELINES:
        rc = FC.call(lib, protos, name, alloc, stream=K._stream())
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
