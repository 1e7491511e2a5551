"""Per-(row, head) checks of the fused divided space-time site kernels (run with -m gpu): attn_fwd_space_fused_kernel<1..7>,
attn_fwd_time_fused_kernel<1 | 2 | 2,20>, their two backward kernels, attn_cls_merge_kernel and attn_cls_finalize_kernel, through
tvts_attn_fwd_divided and tvts_attn_bwd under attn_fused=True -- at both edges of every tile class and at every block / wave layout
of the launches (tests/attn_fused_cases.py), where the whole-tensor gates of test_kernels_gpu.py were the only check so far.

Forward: `out` per (row, head) against float64 (kernel_bounds.divided_fwd_ref) at ATTN_ROW_TOL, the CLS rows also as their own group;
`lse2` of every row, the CLS row the merge kernel writes included, absolutely at LSE2_TOL.
Backward: per (row, head) against float64 evaluated on what the kernels READ (kernel_bounds.attn_bwd_same_inputs): qkv, dO, the lse2
the forward just stored, and for D = rowsum(dO o O) the exact output in the patch rows (the fused kernels form D in registers from
the unrounded output) and the bf16 `out` in the CLS rows (attn_delta_kernel): kernel_bounds.divided_mixed_o_read.  That reference is
itself within half of ATTN_ROW_TOL of float64 autograd at the smallest geometries, for the very inputs used here
(tests/test_kernel_bounds_cpu.py), so no geometry and no row is held to less than the others.
qkv, dO, out and dqkv live in guarded buffers (leading dimension N + 8, NaN guard rows and columns): a write outside the result fails
check_guards, a read past row B * S that reaches a result is a non-finite slice.  cls_ws and cls_acc have exactly the documented
minimum size, are filled with NaN, and a NaN tail behind every scratch buffer must stay untouched.  Every case prints its worst
slice of every quantity ("BOUND" lines; profiles/r26_attention_fused_rows_bounds.txt is their table per kernel instantiation)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_fused_cases as FC  # noqa: E402
import kernel_bounds as KB  # noqa: E402

DEV = "cuda:0"
B, HEADS = FC.B, FC.HEADS
BF16 = torch.bfloat16
NAN = float("nan")
TAIL = 64


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def scratch(elems):
    """fp32 scratch of exactly `elems` elements, NaN, with a NaN tail behind it -> (whole buffer, the view a call gets)"""
    buf = torch.full((elems + TAIL,), NAN, device=DEV)
    return buf, buf[:elems]


def tail_untouched(buf, elems, what):
    assert bool(torch.isnan(buf[elems:]).all()), f"{what}: the {TAIL} elements behind its {elems} were written"


def on_device(qkv_cpu, dO_cpu):
    """the inputs in guarded buffers: a row past B * S or a column past the width that is read is NaN"""
    M = qkv_cpu.shape[0]
    qbuf, qkv = KB.guarded(M, qkv_cpu.shape[1], BF16, DEV)
    gbuf, dO = KB.guarded(M, dO_cpu.shape[1], BF16, DEV)
    qkv.copy_(qkv_cpu); dO.copy_(dO_cpu)
    return (qbuf, gbuf), qkv, dO


class Site:
    """one forward + backward of a divided site through the fused entry points, every buffer guarded"""

    def __init__(self, K, mode, T, n, dh, qkv, dO, *, ws_elems=None, acc_elems=None, backward=True, cls_from=None):
        S, W = 1 + T * n, HEADS * dh
        M = B * S
        parts = FC.parts_of(mode, T, n)
        self.what = f"{mode} T {T} n {n} dh {dh}"
        self.M, self.S, self.W = M, S, W
        geo = dict(B=B, heads=HEADS, S=S, T=T, n=n, head_dim=dh)
        self.ws_elems = B * HEADS * parts * (dh + 2) if ws_elems is None else ws_elems
        self.acc_elems = B * HEADS * parts * 3 * dh if acc_elems is None else acc_elems
        with K.options(attn_fused=True):
            self.obuf, self.out = KB.guarded(M, W, BF16, DEV)
            self.lbuf, lse = scratch(M * HEADS)
            self.lse = lse.view(M, HEADS)
            self.wbuf, ws = scratch(self.ws_elems)
            K.attn_fwd_divided(mode, qkv, self.out, self.lse, ws, **geo)
            if backward:
                if cls_from is not None:  # (test_one_group_of_nan_...: CLIP 0's CLS row of an earlier run's out / lse2, and no other)
                    self.cls0_forward = self.out[0].clone(), self.lse[0].clone()
                    self.out[0], self.lse[0] = cls_from.out[0], cls_from.lse[0]
                self.dbuf, self.dqkv = KB.guarded(M, 3 * W, BF16, DEV)
                self.ebuf, delta = scratch(M * HEADS)
                self.abuf, acc = scratch(self.acc_elems)
                K.attn_bwd(mode, qkv, dO, self.out, self.lse, delta.view(M, HEADS), self.dqkv, cls_acc=acc, **geo)
        torch.cuda.synchronize()
        KB.check_guards(self.obuf, M, W, self.what + " out")
        tail_untouched(self.lbuf, M * HEADS, self.what + " lse2")
        tail_untouched(self.wbuf, self.ws_elems, self.what + " cls_ws")
        if backward:
            KB.check_guards(self.dbuf, M, 3 * W, self.what + " dqkv")
            tail_untouched(self.ebuf, M * HEADS, self.what + " delta")
            tail_untouched(self.abuf, self.acc_elems, self.what + " cls_acc")

    def results(self):
        return (("out", self.out), ("lse2", self.lse), ("dqkv", self.dqkv))

    def took_the_fused_kernels(self):
        """The evidence a caller has that the fused kernels ran, with the partial count attn_fused_cases.parts_of states: the fused
        forward writes every one of the B * heads * parts * (dh + 2) elements of cls_ws and the ordered backward every one of the
        B * heads * parts * 3 * dh of cls_acc (finite inputs: no NaN is left), while the streaming forward does not touch cls_ws and
        a dispatch that expected MORE partials than this scratch holds would have fallen back to it / to the atomics, which leave
        all of cls_acc behind the first B * heads * 3 * dh elements NaN (with one partial the two backward forms cannot be told
        apart this way)"""
        assert not bool(torch.isnan(self.wbuf[:self.ws_elems]).any()), f"{self.what}: cls_ws is not fully written (fused forward not taken?)"
        assert not bool(torch.isnan(self.abuf[:self.acc_elems]).any()), f"{self.what}: cls_acc is not fully written (ordered partials not taken?)"


def inputs_untouched(bufs, qkv, dO):
    KB.check_guards(bufs[0], *qkv.shape, "qkv"); KB.check_guards(bufs[1], *dO.shape, "dO")


def gate_site(tag, site, qkv, dO, mode, T, n, dh, ref=None, backward=True):
    """the gates of the sweep on one Site -> {quantity: worst}; ref: a forward reference computed before (shared, left unchanged)"""
    ro, rl = FC.forward_ref(qkv, mode, T, n, dh) if ref is None else ref
    w = FC.gate_forward(tag, site.out, site.lse, ro, rl, site.S)
    if backward:
        rd = FC.backward_ref(qkv, dO, ro, site.out, site.lse, mode, T, n, dh)
        FC.gate_backward(tag, site.dqkv, rd, site.S, w)
    return w


def _sweep(K, family, mode, T, n, dh):
    qkv_cpu, dO_cpu = (FC.plain_inputs if family == "sweep" else FC.stress_inputs)(mode, T, n, dh)
    bufs, qkv, dO = on_device(qkv_cpu, dO_cpu)
    site = Site(K, mode, T, n, dh, qkv, dO)
    inputs_untouched(bufs, qkv, dO)
    site.took_the_fused_kernels()
    return gate_site(f"attn_fused {family}[{FC.instantiation(mode, T, n)}, T {T}, n {n}, dh {dh}]", site, qkv, dO, mode, T, n, dh)


# ------------------------------------------------------------------------------------------------ 1. geometry sweep
@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("mode,T,n", FC.SWEEP_CASES)
def test_fused_divided_site_per_row(K, mode, T, n, dh):
    """forward and backward of one site per (row, head), N(0, 1) inputs, at every tile class and launch layout of the fused kernels"""
    _sweep(K, "sweep", mode, T, n, dh)


# ------------------------------------------------------------------------------------------------ 5. scores that stress the merges
@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("mode,T,n", FC.STRESS_CASES)
def test_fused_divided_site_per_row_with_a_dominating_partial_and_a_uniform_head(K, mode, T, n, dh):
    """the same gates on the second input family (attn_fused_cases.stress_inputs): one group's CLS partial more than 2^24 above the
    others, one-key softmaxes in patch rows, and a head with q = k = 0"""
    _sweep(K, "stress", mode, T, n, dh)


# ------------------------------------------------------------------------------------------------ 3. group isolation, bit for bit
@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("mode,T,n,sub", [("space", 3, 17, 1), ("time", 16, 30, 29)])
def test_one_group_of_nan_changes_no_bit_outside_it(K, mode, T, n, sub, dh):
    """Every q, k, v and dO value of ONE group of clip 0 (SPACE: frame 1; TIME: patch position 29, the second wave of the second
    chunk) becomes NaN: every row of out, lse2 and dqkv outside that group and outside clip 0's CLS row keeps the bits of the clean
    run, clip 1 keeps every bit.  (Clip 0's CLS query attends the NaN keys, so its output and log-sum-exp are NaN by the definition
    of the operation -- asserted, so the poison did reach the merge; the second backward therefore reads CLIP 0's CLS row of the
    first run's out / lse2, that one row and no other -- otherwise the CLS query's share would carry the NaN into dK / dV of every
    key of the clip, in any implementation.  Clip 1's CLS row is what the second run's merge and finalize kernels wrote: a NaN
    partial of clip 0 merged into another (clip, head) at weight 0 would show there.)  A second clean run with re-poisoned scratch
    reproduces every bit (ordered partials)."""
    S = 1 + T * n
    qkv_cpu, dO_cpu = FC.plain_inputs(mode, T, n, dh)
    bufs, qkv, dO = on_device(qkv_cpu, dO_cpu)
    first = Site(K, mode, T, n, dh, qkv, dO)
    again = Site(K, mode, T, n, dh, qkv, dO)
    for (nm, a), (_, b) in zip(first.results(), again.results()):
        KB.assert_equal_bits(b, a, f"{first.what}: {nm} of a second run")
    gate_site(f"attn_fused isolation[{mode}, T {T}, n {n}, dh {dh}]", first, qkv, dO, mode, T, n, dh)
    rows = torch.arange(S, device=DEV)
    grp = ((rows >= 1 + sub * n) & (rows < 1 + (sub + 1) * n)) if mode == "space" else ((rows >= 1) & ((rows - 1) % n == sub))
    assert int(grp.sum()) == (n if mode == "space" else T)
    poisoned = torch.zeros(B * S, dtype=torch.bool, device=DEV)
    poisoned[:S] = grp
    qkv[poisoned], dO[poisoned] = NAN, NAN
    second = Site(K, mode, T, n, dh, qkv, dO, cls_from=first)
    assert all(bool(torch.isnan(t).all()) for t in second.cls0_forward), f"{first.what}: clip 0's CLS row did not see the NaN group"
    keep = ~poisoned
    keep[0] = False
    assert bool(keep[S:].all()) and int((~keep).sum()) == int(grp.sum()) + 1
    for (nm, a), (_, b) in zip(first.results(), second.results()):
        KB.assert_equal_bits(b[keep].contiguous(), a[keep].contiguous(), f"{first.what}: {nm} outside the NaN group")


# ------------------------------------------------------------------------------------------------ 4. CLS partial forms, scratch thresholds
@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("mode,T,n", [("space", 3, 48), ("time", 8, 57)])
def test_cls_partial_forms_at_the_scratch_thresholds(K, mode, T, n, dh):
    """cls_acc: room for the ordered partials -> within the gates and reproducible bit for bit; one element short of it, and the
    B * heads * 3 * dh minimum -> within the same gates through the fp32 atomics; one element below the minimum -> -22, nothing
    written.  cls_ws: one element short of B * heads * G * (dh + 2) -> the streaming kernels, within the gates; exactly that -> the
    fused kernels (the bits of a call with ample scratch)."""
    S, W = 1 + T * n, HEADS * dh
    parts = FC.parts_of(mode, T, n)
    assert parts == 3
    qkv_cpu, dO_cpu = FC.plain_inputs(mode, T, n, dh)
    bufs, qkv, dO = on_device(qkv_cpu, dO_cpu)
    ref = FC.forward_ref(qkv, mode, T, n, dh)
    tag = f"attn_fused scratch[{mode}, T {T}, n {n}, dh {dh}]"
    ordered, minimum = B * HEADS * parts * 3 * dh, B * HEADS * 3 * dh
    exact = Site(K, mode, T, n, dh, qkv, dO)
    assert exact.acc_elems == ordered
    gate_site(tag + " ordered", exact, qkv, dO, mode, T, n, dh, ref)
    again = Site(K, mode, T, n, dh, qkv, dO)
    for (nm, a), (_, b) in zip(exact.results(), again.results()):
        KB.assert_equal_bits(b, a, f"{tag}: {nm} of a second run, ordered partials")
    for elems, nm in ((ordered - 1, "one short of ordered"), (minimum, "minimum")):
        s = Site(K, mode, T, n, dh, qkv, dO, acc_elems=elems)
        gate_site(f"{tag} atomic ({nm})", s, qkv, dO, mode, T, n, dh, ref)
        assert bool(torch.isnan(s.abuf[minimum:]).all()), f"{tag}: the atomic form wrote behind the first {minimum} elements of cls_acc"
    # ---- below the minimum: refused before anything is launched
    dbuf, dqkv = KB.guarded(B * S, 3 * W, BF16, DEV)
    delta = torch.full((B * S, HEADS), NAN, device=DEV)
    abuf, acc = scratch(minimum - 1)
    geo = dict(B=B, heads=HEADS, S=S, T=T, n=n, head_dim=dh)
    with pytest.raises(K.HipError, match="-22"):
        K.attn_bwd(mode, qkv, dO, exact.out, exact.lse, delta, dqkv, cls_acc=acc, **geo)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dbuf).all()) and bool(torch.isnan(delta).all()) and bool(torch.isnan(abuf).all()), f"{tag}: a refused call wrote"
    # ---- forward scratch
    need = B * HEADS * parts * (dh + 2)
    assert exact.ws_elems == need
    short = Site(K, mode, T, n, dh, qkv, dO, ws_elems=need - 1, backward=False)
    gate_site(tag + " cls_ws one short (streaming)", short, qkv, dO, mode, T, n, dh, ref, backward=False)
    assert bool(torch.isnan(short.wbuf).all()), f"{tag}: the streaming path wrote cls_ws"
    ample = Site(K, mode, T, n, dh, qkv, dO, ws_elems=4 * need, backward=False)
    KB.assert_equal_bits(exact.out, ample.out, tag + ": out at the exact cls_ws size against ample scratch")
    KB.assert_equal_bits(exact.lse, ample.lse, tag + ": lse2 at the exact cls_ws size against ample scratch")
    assert not bool(torch.isnan(exact.wbuf[:need]).any()), f"{tag}: the fused forward left a partial unwritten"
    inputs_untouched(bufs, qkv, dO)


@pytest.mark.parametrize("dh", [64, 80])
def test_refusals_of_the_site_entry_points(K, dh):
    """an e4m3 copy on a split geometry (SPACE n = 112: only the fused kernels write it), asked of the forward and also of the
    backward (tvts_attn_bwd_q8 refuses it the same way), and mode = "cls" to the backward: -22, no result written"""
    T, n = 2, 112
    S, W = 1 + T * n, HEADS * dh
    qkv_cpu, dO_cpu = FC.plain_inputs("space", T, n, dh)
    qkv, dO = qkv_cpu.to(DEV), dO_cpu.to(DEV)
    geo = dict(B=B, heads=HEADS, S=S, T=T, n=n, head_dim=dh)
    ts, am = torch.tensor([1.5 / 448.0], device=DEV), torch.zeros(1, device=DEV)
    out, lse = torch.full((B * S, W), NAN, dtype=BF16, device=DEV), torch.full((B * S, HEADS), NAN, device=DEV)
    ws = torch.full((B * HEADS * 4 * (dh + 2),), NAN, device=DEV)
    q8 = torch.full((B * S, W), 0xFF, dtype=torch.uint8, device=DEV)
    with pytest.raises(K.HipError, match="-22"):
        K.attn_fwd_divided("space", qkv, out, lse, ws, q8out=q8, q8_scale=ts, q8_amax=am, **geo)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(lse).all()) and bool((q8 == 0xFF).all()) and float(am) == 0.0
    K.attn_fwd_divided("space", qkv, out, lse, ws, **geo)
    dqkv, delta = torch.full((B * S, 3 * W), NAN, dtype=BF16, device=DEV), torch.full((B * S, HEADS), NAN, device=DEV)
    acc = torch.full((B * HEADS * T * 3 * dh,), NAN, device=DEV)
    q8d = torch.full((B * S, 3 * W), 0xFF, dtype=torch.uint8, device=DEV)
    with pytest.raises(K.HipError, match="-22"):
        K.attn_bwd("space", qkv, dO, out, lse, delta, dqkv, cls_acc=acc, q8out=q8d, q8_scale=ts, q8_amax=am, **geo)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv).all()) and bool((q8d == 0xFF).all()) and float(am) == 0.0
    with pytest.raises(K.HipError, match="-22"):
        K.attn_bwd("cls", qkv, dO, out, lse, delta, dqkv, cls_acc=acc, **geo)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv).all()) and bool(torch.isnan(delta).all())
