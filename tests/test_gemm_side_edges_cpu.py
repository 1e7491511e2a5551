"""The gates of tests/test_gemm_side_edges_gpu.py can fail (CPU, no kernel): fp32 torch emulations of the four side kernels at the
smallest shapes of that module, summed in the kernels' own order, stay below HALF of their derived bound (kernel_bounds.gemm_bound /
sum_bound), and the same emulation with ONE fault of the kind each kernel can make at an edge of its launch geometry exceeds it:
a wave of rows_linear that loses its last 32-deep step, a colsum without its last row range, a float4 of the strided weight-gradient
reduce written at the dense offset, a gemm_small stage that zero-fills its last partial float4 along K."""
import torch

import gemm_cases as GC
import kernel_bounds as KB

torch.set_num_threads(min(8, torch.get_num_threads()))
NAN = float("nan")


def fails(fn, *words):
    try:
        fn()
    except AssertionError as e:
        msg = str(e)
        for w in words:
            assert w in msg, (w, msg)
        return msg
    raise AssertionError("the fault passed the check")


def test_case_tables_reach_the_edges_they_are_written_for():
    """the geometry facts the GPU module's docstrings state, from the tables themselves"""
    cdiv = lambda x, y: -(-x // y)  # noqa: E731
    assert [cdiv(M, GC.COLSUM_RANGE_ROWS) for M in GC.COLSUM_M] == [1, 1, 1, 1, 2, 3]
    assert cdiv(4097, 2) == 2049 and cdiv(8193, 3) == 2731
    assert all(N % 8 == 0 for N in GC.COLSUM_N) and [N % 64 for N in GC.COLSUM_N] == [8, 8, 8]
    # rows_linear: wave w takes the 32-deep steps w, w + 4, ...; its four-step loop runs while k + 384 < K from k = 32 w
    steps = {Kd: [len(range(w * 32, Kd, 128)) for w in range(4)] for Kd in GC.ROWS_LINEAR_K}
    assert steps[32] == [1, 0, 0, 0] and steps[64] == [1, 1, 0, 0] and steps[96] == [1, 1, 1, 0] and steps[160] == [2, 1, 1, 1]
    unrolled = {Kd: [w * 32 + 384 < Kd for w in range(4)] for Kd in GC.ROWS_LINEAR_K}
    assert unrolled[416] == [True, False, False, False] and unrolled[512] == [True] * 4 and unrolled[544] == [True] * 4
    assert not any(unrolled[128]) and steps[544][0] == 5  # 544: wave 0 takes the loop once and one step behind it
    # gemm_small: which (shape, pattern) pairs the dispatcher stages with 16-byte loads
    vec = [s for s in GC.SMALL_SHAPES if GC.small_vec_eligible(*s, (s[2], 1), (s[1], 1))]
    assert vec == [(32, 32, 16), (64, 64, 32), (64, 64, 64), (36, 40, 20)]
    # grouped: ranges per member and item totals
    assert GC.tn_group_ranges(1040, 2) == GC.tn_ranges(1040, 2) == (2, 464) and GC.tn_group_ranges(520, 2) == (2, 200)
    assert GC.tn_group_ranges(300, 2) == (1, 300) != GC.tn_ranges(300, 2) and GC.tn_group_ranges(65, 2) == (1, 65)
    items = {k: GC.tn_group_items(spec, sp) for k, (sp, spec) in GC.TN_GROUPS.items()}
    assert items["trio"] == 18 and items["few_items"] == 4 and items["mixed_m"] == 16 and items["one_strided"] == 2
    for sp, spec in GC.TN_GROUPS.values():
        assert 1 <= len(spec) <= 64 and all(Na % 8 == 0 and Nb % 8 == 0 for (_, Na, Nb, *_) in spec)
    split_dense = [m for sp, spec in GC.TN_GROUPS.values() for m in spec if not m[5] and GC.tn_group_ranges(m[0], sp)[0] > 1]
    split_strided = [m for sp, spec in GC.TN_GROUPS.values() for m in spec if m[5] and GC.tn_group_ranges(m[0], sp)[0] > 1]
    assert split_dense and split_strided  # both branches of the reduce's element pass run


def test_gemm_tn_grouped_refuses_every_record_the_single_entry_point_refuses():
    """tvts_gemm_tn_bf16_grouped with ONE field of one valid record changed (the record test_gemm_tn_grouped_refusals launches
    unchanged on the GPU): -22 before any HIP call, here without a GPU on dummy host buffers no refused call reads.  The entry
    point used to check the divisibility of a record only: a row pitch below the row (rows that overlap), a null operand and
    an empty extent went through to the launch."""
    import ctypes

    from tvts_amd import _lib, hip
    lib = _lib.load()
    dummy = [ctypes.create_string_buffer(64) for _ in range(6)]
    addr = [ctypes.addressof(d) for d in dummy]
    base = dict(P=addr[0], ldp=144, Q=addr[1], ldq=72, M=520, Na=136, Nb=72, out=addr[2], ldo=76, accumulate=0, colsum=None)
    nbytes = lib.tvts_gemm_tn_grouped_table_bytes(1)
    host = ctypes.create_string_buffer(nbytes)

    def rc(**change):
        recs = (hip.TnGroup._Rec * 1)()
        for k, v in {**base, **change}.items():
            setattr(recs[0], k, v)
        return lib.tvts_gemm_tn_bf16_grouped(ctypes.cast(recs, ctypes.c_void_p), 1, ctypes.c_void_p(addr[3]), ctypes.cast(host, ctypes.c_void_p),
                                             nbytes, 1, ctypes.c_void_p(addr[4]), 1 << 20, 2 << 8, None)

    for change in (dict(M=0), dict(Na=0), dict(Nb=0), dict(Na=-8), dict(P=None), dict(Q=None), dict(out=None), dict(ldp=128), dict(ldq=64),
                   dict(ldo=68), dict(Na=132), dict(Nb=68), dict(ldp=148), dict(ldq=76), dict(ldo=78)):
        assert rc(**change) == -22, change


def test_rows_linear_emulation_is_inside_half_the_bound_and_a_dropped_wave_step_is_not():
    """K = 160: five 32-deep steps, wave 0 takes steps 0 and 4, waves 1 .. 3 one each; the partials meet as ((w0 + w1) + w2) + w3,
    then bias and residual.  Fault: wave 0 ends one step early (its loop condition one step short)."""
    R, N, Kd = 17, 16, 160
    g = torch.Generator().manual_seed(160)
    a = torch.randn(R, Kd, generator=g).bfloat16()
    w = (torch.randn(N, Kd, generator=g) * Kd ** -0.5).bfloat16()
    bias, res = torch.randn(N, generator=g), torch.randn(R, N, generator=g)

    def emulate(drop_last_step_of_wave=None):
        part = []
        for wave in range(4):
            ks = list(range(wave * 32, Kd, 128))
            if wave == drop_last_step_of_wave:
                ks = ks[:-1]
            acc = torch.zeros(R, N)
            for k in ks:
                acc = acc + a[:, k:k + 32].float() @ w[:, k:k + 32].float().t()
            part.append(acc)
        return (((part[0] + part[1]) + part[2]) + part[3]) + bias + res

    assert KB.check_gemm(emulate(), a, w, bias=bias, residual=res, what="rows_linear emulation") <= 0.5
    for wave in range(4):
        fails(lambda: KB.check_gemm(emulate(wave), a, w, bias=bias, residual=res, what="rows_linear"), "outside the bound")


def test_colsum_emulation_is_inside_half_the_bound_and_a_dropped_last_range_is_not():
    """M = 4097: two ranges of 2049 and 2048 rows; inside a range 32 row lanes stride the rows and meet in lane order; the range
    partials are added to the output in range order.  Fault: the last range is left out (one range too few in the grid)."""
    M, N = 4097, 8
    g = torch.Generator().manual_seed(4097)
    x = torch.randn(M, N, generator=g).bfloat16()
    init = torch.randn(N, generator=g)
    rows = -(-M // 2)

    def emulate(ranges=2):
        t = init.clone()
        for y in range(ranges):
            xr = x[y * rows:min(M, (y + 1) * rows)].float()
            lanes = [xr[rl::32].cumsum(0)[-1] if xr[rl::32].shape[0] else torch.zeros(N) for rl in range(32)]
            s = torch.zeros(N)
            for v in lanes:
                s = s + v
            t = t + s
        return t

    ref = x.double().sum(0) + init.double()
    bound = KB.sum_bound(x.double().abs().sum(0), M, init=init)
    assert KB.assert_within(emulate(), ref, bound, "colsum emulation") <= 0.5
    fails(lambda: KB.assert_within(emulate(ranges=1), ref, bound, "colsum"), "outside the bound")


def test_strided_reduce_emulation_is_inside_half_the_bound_and_a_float4_at_the_dense_offset_is_not():
    """(M, Na, Nb) = (130, 136, 72), two ranges (128 rows and 2), output with ldo = Nb + 4 inside NaN guards, accumulating: element
    e = a Nb + b of the partial planes belongs at a ldo + b.  Fault: ONE float4 of the element pass is written at offset e of the
    output (the dense branch's address) -- its own place keeps the initial value, and the float4 lands on other elements or
    in the guard columns."""
    M, Na, Nb = 130, 136, 72
    ldo = Nb + 4
    assert GC.tn_ranges(M, 2) == (2, 2)
    g = torch.Generator().manual_seed(130)
    p, q = torch.randn(M, Na, generator=g).bfloat16(), torch.randn(M, Nb, generator=g).bfloat16()
    init = torch.randn(Na, Nb, generator=g)
    planes = [p[:128].float().t() @ q[:128].float(), p[128:].float().t() @ q[128:].float()]
    val = (init + planes[0]) + planes[1]

    def emulate(misplaced=None):
        buf = torch.full((Na + 3, ldo), NAN)
        buf[:Na, :Nb] = init
        flat = buf.view(-1)
        for i in range(Na * Nb // 4):
            e = 4 * i
            a_, b_ = divmod(e, Nb)
            o = e if i == misplaced else a_ * ldo + b_
            flat[o:o + 4] = val[a_, b_:b_ + 4]
        return buf

    buf = emulate()
    KB.check_guards(buf, Na, Nb)
    assert KB.check_gemm(buf[:Na, :Nb], p.t(), q.t(), residual=init, K=M, what="strided reduce emulation") <= 0.5
    # a float4 of row 0 sits at the same place in both layouts: no fault there.  Row 1 on: another element, or a guard column
    assert torch.equal(emulate(misplaced=Nb // 4 - 1)[:Na, :Nb], buf[:Na, :Nb])
    for i in (Nb // 4, Nb // 4 + 17, Na * Nb // 4 - 1):
        bad = emulate(misplaced=i)
        fails(lambda: KB.check_gemm(bad[:Na, :Nb], p.t(), q.t(), residual=init, K=M, what="strided reduce"), "outside the bound")
    # the first float4 of row 1 has the dense offset Nb: the guard columns of row 0
    fails(lambda: KB.check_guards(emulate(misplaced=Nb // 4), Na, Nb, "strided reduce"), "columns past")


def test_gemm_small_emulation_is_inside_half_the_bound_and_a_zero_filled_last_float4_is_not():
    """(33, 65, 17) and (65, 63, 33), fp32 operands (c = 6): K ends one element into a float4.  Fault: the staging treats that
    partial float4 as out of range and zero-fills it (the vector load's extent test applied to a K that is no multiple of 4)."""
    for (M, N, Kd) in ((33, 65, 17), (65, 63, 33)):
        g = torch.Generator().manual_seed(M + Kd)
        a, b = torch.randn(M, Kd, generator=g), torch.randn(N, Kd, generator=g)
        bias = torch.randn(N, generator=g)
        init = torch.randn(M, N, generator=g)

        def emulate(k_end):
            acc = torch.zeros(M, N)
            for k0 in range(0, k_end, 32):  # 32-deep stages, one fma chain inside each
                acc = acc + a[:, k0:min(k_end, k0 + 32)] @ b[:, k0:min(k_end, k0 + 32)].t()
            return 0.5 * acc + bias

        assert KB.check_gemm(emulate(Kd), a, b, scale=0.5, bias=bias, c=6, what="gemm_small emulation") <= 0.5
        assert KB.check_gemm(init + emulate(Kd), a, b, scale=0.5, bias=bias, residual=init, c=6, what="gemm_small emulation") <= 0.5
        fails(lambda: KB.check_gemm(emulate(Kd // 4 * 4), a, b, scale=0.5, bias=bias, c=6, what="gemm_small"), "outside the bound")
        fails(lambda: KB.check_gemm(init + emulate(Kd // 4 * 4), a, b, scale=0.5, bias=bias, residual=init, c=6, what="gemm_small"),
              "outside the bound")
