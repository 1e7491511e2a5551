"""The GEMM kernels at their tile edges, on strided views, per element (run with -m gpu).

tests/test_kernels_gpu.py holds the GEMMs to kernel_bounds.gemm_bound at the training step's own sizes: N a multiple of 256 on
the 256 x 256 NT kernel, three row tails, contiguous operands.  Here the same form loops (tests/gemm_cases.py) run at the
smallest shapes that reach each edge path -- fewer rows than a wave tile, one row, rows and columns one off a wave-tile or tile
boundary, K shorter than the ring and one stage longer, contraction ranges of a single row -- with every operand and side input a
view inside a NaN-poisoned buffer (leading dimension != width) and every output inside NaN / 0xFF guards.  Every case asserts the
kernel or form it ran on (tvts_gemm_nt_select / tvts_gemm_tn_select, STREAMK_TAKEN, a ring form not refused)."""
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

# (M, N, K).  128 x 128 kernel and ring forms, wave tile 64 x 64: one row; one short of / one past a wave tile; one short of / one
# past the tile; several tiles.  K = 64 / 128 / 192 are shorter than the ring's stages in flight, K = 320 one stage longer.
NT_128 = [(1, 4, 64), (63, 60, 64), (65, 68, 128), (127, 124, 192), (129, 132, 64), (385, 260, 320)]
NT_RING = NT_128 + [(193, 132, 192), (257, 4, 320)]  # ... and across the 192- and 256-row tiles of ring3 / ring4
# 256 x 256 kernel, wave tile 128 rows x 64 columns: the second row of wave tiles wholly outside (M < 128), one row, one off
NT_256 = [(1, 8, 64), (127, 56, 128), (129, 72, 192), (255, 248, 128), (257, 264, 320), (385, 520, 64)]
NT_FP8 = [(1, 8, 128), (129, 72, 256), (257, 264, 384), (385, 248, 128)]


# ------------------------------------------------------------------------------------------------ NT bf16
@pytest.mark.parametrize("tile", ["128noring", "ring2", "ring3", "ring4"])
@pytest.mark.parametrize("M,N,K_", NT_RING)
def test_gemm_nt_128_and_ring_edges_within_the_bound(K, M, N, K_, tile):
    """the double-buffered 128 kernel and the three ring forms, each through check_gemm on its own (not only bit-compared with one
    another): no ring form may refuse one of these shapes (nt_ring_fits only refuses operands past 4 GiB)"""
    GC.expect_kernel(K, M, N, tile)
    a, b, bias, res, h = GC.nt_operands(M, N, K_, seed=M + N + K_, device=DEV)
    worst, taken = GC.nt_forms(K, a, b, bias, res, h, forms=[dict(tile=tile)], act_forms=[dict(tile=tile)], must_take={tile}, edge=True)
    assert taken == {tile}
    KB.bound_line(f"gemm_nt_edges[{tile},{M},{N},{K_}]", worst)


@pytest.mark.parametrize("M,N,K_", NT_256)
def test_gemm_nt_256_edges_within_the_bound(K, M, N, K_):
    """the column-edge code of the 256 x 256 kernel (n >= N predicates, the N - 4 / N - 8 clamps of side-input loads, the non-FULL
    epilogues, the choice between the bf16-first and the generic patch) and its row tails; ldc, ldp, ldh multiples of 8"""
    GC.expect_kernel(K, M, N, 256)
    a, b, bias, res, h = GC.nt_operands(M, N, K_, seed=M + N + K_, device=DEV)
    assert h.stride(0) % 8 == 0
    worst, taken = GC.nt_forms(K, a, b, bias, res, h, forms=[dict(tile=256)], act_forms=[dict(tile=256)], must_take={"256"}, edge=True)
    KB.bound_line(f"gemm_nt_edges[256,{M},{N},{K_}]", worst)


def test_gemm_nt_output_pitch_the_256_kernel_cannot_take_runs_on_the_128_kernel(K):
    """[65 535, 256] is a result the dispatcher gives the 256 kernel (256 of its tiles); with ldc = 260 (ldc % 8 != 0: no 16-byte
    epilogue accesses) and no forced tile the entry point runs it on the 128 x 128 kernel instead -- 1024 tiles, where its cost
    model prefers the double-buffered kernel to the ring -- and the result is still right.  tvts_gemm_nt_select does not see ldc,
    so the landing is asserted by what can be observed: select reports 256 for the shape, the same call under a forced tile=256
    is refused (the entry point knows the 256 kernel cannot take it), and the bits are those of a forced tile=128 launch."""
    M, N, K_ = 65535, 256, 64
    assert K.gemm_nt_select(M, N) == 256
    a, b, bias, res, h = GC.nt_operands(M, N, K_, seed=7, device=DEV)
    worst, _ = GC.nt_forms(K, a, b, bias, res, h, forms=[dict(tile=None)], act_forms=[dict(tile=None)], cols=4)
    for dt in (torch.bfloat16, torch.float32):
        (_, o0), (_, o1), (_, o2) = (KB.guarded(M, N, dt, DEV, cols=4) for _ in range(3))
        K.gemm_nt(a, b, o0, bias=bias)
        K.gemm_nt(a, b, o1, bias=bias, tile=128)
        KB.assert_equal_bits(o0, o1, f"unforced against tile=128, {dt}")
        with pytest.raises(K.HipError):
            K.gemm_nt(a, b, o2, bias=bias, tile=256)
    KB.bound_line(f"gemm_nt_edges[ldc%8,{M},{N},{K_}]", worst)


def test_gemm_nt_forced_256_with_n_not_a_multiple_of_8_takes_the_128_kernel(K):
    """documented behaviour (include/tvts_hip.h, TVTS_GEMM_TILE_256): a result with N % 8 != 0 is not the 256 kernel's to take; a
    forced tile=256 runs it on the 128 x 128 kernel (tvts_gemm_nt_select says so) and the result is right"""
    M, N, K_ = 65, 68, 128
    assert K.gemm_nt_select(M, N, tile=256) == 128
    a, b, bias, res, h = GC.nt_operands(M, N, K_, seed=3, device=DEV)
    worst, taken = GC.nt_forms(K, a, b, bias, res, h, forms=[dict(tile=256)], act_forms=[dict(tile=256)], must_take={"256"}, edge=True)
    KB.bound_line(f"gemm_nt_edges[256->128,{M},{N},{K_}]", worst)


@pytest.mark.parametrize("M,N,K_", [(520, 1016, 320), (520, 1016, 192)])
def test_gemm_nt_streamk_edges_within_the_bound(K, M, N, K_):
    """the stream-K walk on 3 x 4 tiles ragged on both sides: 5 stages, and 3 -- the shortest K the plan accepts (12 tiles leave
    the emptiest XCD one tile: min_units = nk, on a grid of 8 blocks, and min_units / (sk_grid / 8) >= 3 asks for nk >= 3).  Every
    launch must have taken the walk (STREAMK_TAKEN), and the arrival counters are zero afterwards"""
    GC.expect_kernel(K, M, N, 256)
    a, b, bias, res, h = GC.nt_operands(M, N, K_, seed=M + N + K_, device=DEV)
    sk0 = K.STREAMK_TAKEN[0]
    worst, taken = GC.nt_forms(K, a, b, bias, res, h, forms=[dict(streamk=True)], act_forms=[dict(streamk=True)], must_take={"streamk"},
                               edge=True)
    assert K.STREAMK_TAKEN[0] == sk0 + 14  # 5 plain / residual launches, 2 x 2 x 2 activation and gate launches, the bf16 residual stream
    ws = K._nt_workspace(a.device)
    torch.cuda.synchronize()
    assert int(ws[:65536].view(torch.int32).abs().sum()) == 0
    KB.bound_line(f"gemm_nt_edges[streamk,{M},{N},{K_}]", worst)


def test_gemm_nt_streamk_refuses_one_k_stage(K):
    """K = 64 is one stage (nk < 2): nothing to split, the forced walk is refused and nothing is written"""
    M, N, K_ = 520, 1016, 64
    a, b, bias, _, _ = GC.nt_operands(M, N, K_, seed=5, device=DEV)
    buf, out = KB.guarded(M, N, torch.bfloat16, DEV)
    sk0 = K.STREAMK_TAKEN[0]
    with pytest.raises(K.HipError):
        K.gemm_nt(a, b, out, bias=bias, streamk=True)
    assert K.STREAMK_TAKEN[0] == sk0 and bool(torch.isnan(buf).all())


# ------------------------------------------------------------------------------------------------ NT fp8
def _fp8_ops(K, M, N, K_, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(M, K_, generator=g, device=DEV) * torch.logspace(-3, 1, M, device=DEV)[:, None]
    b = torch.randn(N, K_, generator=g, device=DEV) * K_ ** -0.5
    bias, res = torch.randn(N, generator=g, device=DEV), torch.randn(M, N, generator=g, device=DEV)
    b8, sb = K.quantize_fp8(b)
    return g, a, GC.place(b8), sb, GC.place(bias), GC.place(res)


@pytest.mark.parametrize("M,N,K_", NT_FP8)
def test_gemm_nt_fp8_edges_within_the_bound(K, M, N, K_):
    """the fp8 entry points always take the 256 x 256 kernel: its column and row edges on e4m3 operands (strided, poisoned with the
    e4m3 NaN), tensor and row scales, the forms of test_gemm_fp8_forms_within_the_bound.

    K = 128 / 256 / 384 are contractions the e4m3 matrix instructions cannot hold inside gemm_bound: they leave up to 2^-11.9 of an
    element's largest |product| whatever K is (the bf16 MFMA 2^-20.8 on the same decoded values), which at (385, 248, 128) put 102
    of 95 480 fp32 results outside the bound, worst 1.9.  Under 512 the entry points decode the fragments to bf16 and multiply on
    the bf16 MFMA (gemm_nt256.h, FP8_EXACT_BELOW); these shapes hold that path to the bound."""
    g, a, b8, sb, bias, res = _fp8_ops(K, M, N, K_, seed=M + N)
    worst = GC.fp8_nt_forms(K, a, b8, sb, bias, res, g, put=GC.place)
    KB.bound_line(f"gemm_fp8_edges[{M},{N},{K_}]", worst)


@pytest.mark.parametrize("form", ["gelu", "gate"])
def test_gemm_nt_fp8_e4m3_copy_at_the_edges_is_quantize_fp8_rows_of_the_output(K, form):
    """q8out on (257, 264, 384): with the bf16 result stored, the bytes equal quantize_fp8_rows(out, tscale) and amax is exact (the
    statement of test_gemm_nt_fp8_e4m3_copy_is_quantize_fp8_rows_of_the_output); the guard bytes of q8out stay 0xFF"""
    M, N, K_ = 257, 264, 384
    g = torch.Generator(device=DEV).manual_seed(8)
    a8, sa = K.quantize_fp8_rows(torch.randn(M, K_, generator=g, device=DEV).bfloat16())
    b8, sb = K.quantize_fp8(torch.randn(N, K_, generator=g, device=DEV) * K_ ** -0.5)
    a8, b8 = GC.place(a8), GC.place(b8)
    ad, bd, scale = KB.decode_e4m3(a8), KB.decode_e4m3(b8), sa.double() * sb.double()
    bias = GC.place(torch.randn(N, generator=g, device=DEV))
    h = GC.place((torch.randn(M, N, generator=g, device=DEV) * 1.5).bfloat16())
    kw = dict(bias=bias, act="gelu") if form == "gelu" else dict(gate_h=h, gate_act="gelu")
    ts = torch.tensor([2.0 / 448.0], device=DEV)
    obuf, out = KB.guarded(M, N, torch.bfloat16, DEV)
    pbuf, pre = KB.guarded(M, N, torch.bfloat16, DEV) if form == "gelu" else (None, None)
    qbuf, q = KB.guarded(M, N, torch.uint8, DEV)
    am = torch.zeros(1, device=DEV)
    K.gemm_nt_fp8(a8, sa, b8, sb, out, preact=pre, q8out=q, q8_scale=ts, q8_amax=am, **kw)
    if form == "gelu":
        w = KB.check_gemm(out, ad, bd, scale=scale, bias=bias, act="gelu", preact=pre, what="fp8 q8out gelu")
        KB.check_guards(pbuf, M, N, "fp8 q8out gelu preact")
    else:
        w = KB.check_gemm(out, ad, bd, scale=scale, gate_h=h, gate_act="gelu", what="fp8 q8out gate")
    KB.check_guards(obuf, M, N, f"fp8 q8out {form} out")
    KB.check_guards(qbuf, M, N, f"fp8 q8out {form} bytes")
    am_ref = torch.zeros(1, device=DEV)
    q_ref, _ = K.quantize_fp8_rows(out, tscale=ts, amax=am_ref)
    KB.assert_equal_bits(q.contiguous(), q_ref, f"fp8 q8out {form} bytes")
    assert float(am) == float(out.float().abs().max()) == float(am_ref), (float(am), float(am_ref))
    KB.bound_line(f"gemm_fp8_edges[q8out {form},{M},{N},{K_}]", w)


# ------------------------------------------------------------------------------------------------ TN
TN_M = [1, 31, 33, 63, 64, 65, 129]
TN_WIDTHS = [(8, 8), (120, 136), (248, 264), (264, 520)]


def _tn_ops(M, Na, Nb, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(M, Na, generator=g, device=DEV).bfloat16()
    q = torch.randn(M, Nb, generator=g, device=DEV).bfloat16()
    init = torch.randn(Na, Nb, generator=g, device=DEV)
    cs_init = torch.randn(Na, generator=g, device=DEV)
    p, q = GC.place_pair(p, q)
    return p, q, init, cs_init


@pytest.mark.parametrize("Na,Nb", TN_WIDTHS)
@pytest.mark.parametrize("M", TN_M)
def test_gemm_tn_edges_within_the_bound(K, M, Na, Nb):
    """short contractions (M < 64: one stage with a tail; 64: none; 65 / 129: a range of one row) on both tiles, accumulate, with
    and without the workspace, forced range counts 1 / 2 / 4 (renormalised to whole 64-row stages: tn_ranges), the fused reduce
    wherever there is more than one range, each with and without the fused bias gradient.  P and Q are column slices of one
    poisoned buffer (ldp = ldq != Na), the output is guarded (ldo > Nb).  Nothing may be refused."""
    p, q, init, cs_init = _tn_ops(M, Na, Nb, seed=M + Na)
    assert p.stride(0) == q.stride(0) != Na
    kws = []
    for tile in (128, 256):
        assert K.gemm_tn_select(M, Na, Nb, tile=tile) == tile
        for splits in (1, 2, 4):
            for ws in (True, False):
                kws.append(dict(tile=tile, splits=splits, workspace=ws))
            if GC.tn_ranges(M, splits)[0] > 1:
                kws.append(dict(tile=tile, splits=splits, fused=True))
    if M == 129:
        assert GC.tn_ranges(M, 4) == (3, 1) and GC.tn_ranges(M, 2) == (2, 1)  # the last range is a single row
    worst, fused_runs = GC.tn_forms(K, p, q, init, kws, may_refuse=lambda kw: False, cs_init=cs_init)
    assert fused_runs == 4 * sum(1 for kw in kws if kw.get("fused"))  # accumulate off / on, colsum off / on
    KB.bound_line(f"gemm_tn_edges[{M},{Na},{Nb}]", worst)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("tile", [128, 256])
def test_gemm_tn_with_a_workspace_gives_the_same_bits_twice(K, tile, fused):
    """the fixed order of the split partials and of the bias gradient's: three ranges (the last of one row), two runs, same bits"""
    M, Na, Nb = 129, 120, 136
    p, q, init, cs_init = _tn_ops(M, Na, Nb, seed=11)
    runs = []
    for _ in range(2):
        buf, out = KB.guarded(Na, Nb, torch.float32, DEV)
        out.copy_(init)
        cs = cs_init.clone()
        K.gemm_tn(p, q, out, accumulate=True, colsum=cs, tile=tile, splits=4, fused=fused)
        KB.check_guards(buf, Na, Nb)
        runs.append((out.clone(), cs))
    KB.assert_equal_bits(runs[0][0], runs[1][0], "tn out, second run")
    KB.assert_equal_bits(runs[0][1], runs[1][1], "tn colsum, second run")
    w = KB.check_gemm(runs[0][0], p.t(), q.t(), residual=init, K=M, what="tn ordered")
    KB.bound_line(f"gemm_tn_edges[ordered,{tile},{fused}]", w)


@pytest.mark.parametrize("M,Na,Nb", [(1, 16, 16), (65, 48, 272), (129, 272, 48)])
def test_gemm_tn_fp8_edges_within_the_bound(K, M, Na, Nb):
    """the e4m3 weight gradient with one token, one past half a stage and one past a stage, strided operands (ldp = ldq, multiples
    of 16 bytes), accumulate off and on, with the workspace and without, guarded output.

    Contractions this short run with the e4m3 fragments decoded to bf16 (gemm_tn8_kernel<true>, under FP8_EXACT_BELOW = 512
    tokens): on the e4m3 matrix instruction M = 65 left 1720 of 13 056 elements outside the bound (worst 8.06), M = 129 60 (1.98) --
    the instruction's own 2^-12 of the largest |product|, see test_gemm_nt_fp8_edges_within_the_bound."""
    g = torch.Generator(device=DEV).manual_seed(M + Na)
    p8, sp = K.quantize_fp8(torch.randn(M, Na, generator=g, device=DEV))
    q8, sq = K.quantize_fp8(torch.randn(M, Nb, generator=g, device=DEV))
    init = torch.randn(Na, Nb, generator=g, device=DEV)
    p8, q8 = GC.place_pair(p8, q8)
    assert p8.stride(0) % 16 == 0 and p8.stride(0) != Na
    worst = GC.fp8_tn_forms(K, p8, sp, q8, sq, init, guard=True)
    KB.bound_line(f"gemm_tn_fp8_edges[{M},{Na},{Nb}]", worst)


# ------------------------------------------------------------------------------------------------ the refusal table's baselines
@pytest.mark.parametrize("name", sorted(GC.BASELINES))
def test_every_baseline_of_the_refusal_table_launches(K, name):
    """tests/test_gemm_args_cpu.py derives every refused call from one of these by changing ONE argument; each is a valid call:
    it returns 0, runs, and leaves finite results"""
    from tvts_amd import _lib
    lib, protos = _lib.load(), _lib.prototypes()
    keep = {}

    def alloc(m):
        if m == GC.NT_WS:
            ws = K._nt_workspace(torch.device(DEV))
            return ctypes.c_void_p(ws.data_ptr()), ws.numel()
        t = m.tensor(DEV, seed=len(keep))
        keep[id(m)] = t
        return ctypes.c_void_p(t.data_ptr())

    rc = GC.call(lib, protos, name, alloc, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    _, base = GC.BASELINES[name]
    for an in ("out", "preact", "colsum"):
        m = base.get(an)
        if isinstance(m, GC.Mat):
            assert bool(torch.isfinite(keep[id(m)].float()).all()), (name, an)
    if name == "nt_streamk":
        assert int(K._nt_workspace(torch.device(DEV))[:65536].view(torch.int32).abs().sum()) == 0
