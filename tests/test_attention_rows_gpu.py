"""Per-(row, head) checks of the attention entry points the whole-tensor gates of test_kernels_gpu.py / test_v1_gpu.py still carried
alone (run with -m gpu): the streaming FULL kernels (block-shared and per-wave), the kv_len forms and their dropout pair, the
query-subset forms on the MODE_CLS kernels (tail, one row) and the split divided backward.

Forward: `out` per (row, head) against float64 (kernel_bounds.attn_fwd_ref) at ATTN_ROW_TOL, `lse2` per element to 1e-3.
Backward: per (row, head) against float64 evaluated on what the kernel READ -- the bf16 output and the log-sum-exp the forward
kernel just wrote (kernel_bounds.attn_bwd_same_inputs; float64 autograd is the wrong yardstick where delta = rowsum(dO o bf16(O))
cancels: tests/test_kernel_bounds_cpu.py::test_delta_from_the_bf16_output_limits_dq_where_a_query_has_few_keys).
Sizes sit on both sides of every tile edge of the kernels: 16-row waves, 64-query blocks, 64-key tiles, 32-key halves.
Outputs live in guarded buffers (leading dimension N + 8, NaN guard rows and columns); rows an entry point must not write are NaN
before the call and after it, rows the caller zeroes stay exactly zero.  Every case prints its worst slice ("BOUND" lines)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
from oracle import tvts_v1_oracle as V  # noqa: E402  (checker only: the dropout mask generator)

DEV = "cuda:0"
TOL = KB.ATTN_ROW_TOL
HEADS = 3  # an odd count: a wrong head-column stride cannot land on another head's slice of the same row
BF16 = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def inputs(B, S, dh, seed, scale=1.0):
    """bf16 qkv [B * S, 3W] and dO [B * S, W] on the device, drawn on the host (the same values on every machine)"""
    g = torch.Generator().manual_seed(seed)
    W = HEADS * dh
    qkv = (torch.randn(B * S, 3 * W, generator=g) * scale).bfloat16().to(DEV)
    return qkv, torch.randn(B * S, W, generator=g).bfloat16().to(DEV)


def nan_rows(M, cols):
    return torch.full((M, cols), NAN, device=DEV)


class Worst(dict):
    """worst slice per quantity over the variants of one case"""

    def up(self, k, v):
        self[k] = max(self.get(k, 0.0), float(v))

    def report(self, tag):
        for k, v in self.items():
            KB.bound_line(f"{tag} {k}" + ("" if "(" in k else " (per-row rel)"), v)


def check_fwd(w, what, out, lse, ro, rl, rows=None):
    """out [M, W] (bf16) and lse [M, heads] against the float64 reference on the rows `rows` (bool [M]; default: all).  The rows
    left out take the reference's own values, so that a failure names the TOKEN row (and with it the tile edge), not an index
    into the subset"""
    if rows is not None:
        out, lse = torch.where(rows[:, None], out.double(), ro), torch.where(rows[:, None], lse.double(), rl)
    w.up("out", KB.assert_rows_within(out, ro, TOL["out"], groups=HEADS, what=what + " out", out_dtype=BF16))
    w.up("lse2 (|err| / 1e-3)", KB.assert_within(lse, rl, KB.LSE2_TOL, what + " lse2"))


def check_bwd(w, what, dqkv, rd, W, suffix=""):
    """dqkv [M, 3W] (bf16) against the float64 reference [M, 3W], every (row, head) slice of every third"""
    for i, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(i * W, (i + 1) * W)
        w.up(nm + suffix, KB.assert_rows_within(dqkv[:, sl], rd[:, sl], TOL[nm], groups=HEADS, what=f"{what} {nm}{suffix}", out_dtype=BF16))


# ------------------------------------------------------------------------------------------------ FULL, streaming kernels
@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [16, 17, 32, 33, 63, 64, 65, 96, 97, 128, 129, 197])
def test_full_streaming_attention_per_row(K, S, causal, dh):
    """attn_fwd_shared / bwd_dq_shared / bwd_dkv_shared (default) and attn_fwd / bwd_dq / bwd_dkv (attn_shared=False), with and
    without the transposing LDS reads.  S <= 32 reaches them under attn_fused=False.  Causal cases draw N(0, 1) inputs; the others
    N(0, 1/4) for q / k / v, at which float64 autograd is a usable second reference (attn_conditioning < tol / 3 is asserted)."""
    B, W = 2, HEADS * dh
    qkv, dO = inputs(B, S, dh, seed=1000 + S, scale=1.0 if causal else 0.5)
    q3, d3 = qkv.view(B, S, 3 * W), dO.view(B, S, W)
    ro, rl, _ = KB.attn_fwd_ref(q3, HEADS, dh, causal=causal)
    ro, rl = ro.reshape(B * S, W), rl.reshape(B * S, HEADS)
    auto = None
    if not causal and S >= 33:
        cond = KB.attn_conditioning(q3, d3, HEADS, dh)
        for nm, e in cond.items():
            assert float(e.max()) < TOL[nm] / 3, f"unsuitable inputs: conditioning of {nm} is {float(e.max()):.3g}"
        auto = KB.attn_autograd(q3, d3, HEADS, dh)[1].reshape(B * S, 3 * W)
    w = Worst()
    for shared in (True, False):
        for tr in (True, False):
            what = f"full[S {S}, causal {causal}, dh {dh}, shared {shared}, tr {tr}]"
            with K.options(attn_shared=shared, attn_tr=tr, attn_fused=S > 32):
                obuf, out = KB.guarded(B * S, W, BF16, DEV)
                lse, delta = nan_rows(B * S, HEADS), nan_rows(B * S, HEADS)
                K.attn_fwd("full", qkv, out, lse, B=B, heads=HEADS, S=S, causal=causal, head_dim=dh)
                dbuf, dqkv = KB.guarded(B * S, 3 * W, BF16, DEV)
                K.attn_bwd("full", qkv, dO, out, lse, delta, dqkv, B=B, heads=HEADS, S=S, causal=causal, head_dim=dh)
            torch.cuda.synchronize()
            KB.check_guards(obuf, B * S, W, what + " out"); KB.check_guards(dbuf, B * S, 3 * W, what + " dqkv")
            check_fwd(w, what, out, lse, ro, rl)
            rd = KB.attn_bwd_same_inputs(q3, d3, out.view(B, S, W), lse.view(B, S, HEADS), HEADS, dh, causal=causal)
            check_bwd(w, what, dqkv, rd.reshape(B * S, 3 * W), W)
            if auto is not None:
                check_bwd(w, what, dqkv, auto, W, " vs autograd")
    w.report(f"attn_rows full[S {S}, causal {int(causal)}, dh {dh}]")


# ------------------------------------------------------------------------------------------------ kv_len forms, dropout pair
LEN_CASES = {"S130": (130, [1, 2, 63, 64, 65, 128, 129, 130]), "S50": (50, [1, 16, 17, 32, 33, 49, 50]),
             "S50_len0": (50, [0, 16, 17, 32, 33, 49, 50])}  # a length of 0 behaves as 1 (the clamp in decode)


def _len_case(case, dh, seed):
    S, lens = LEN_CASES[case]
    B, W = len(lens), HEADS * dh
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    valid = torch.arange(S, device=DEV)[None, :] < kv.clamp(1, S)[:, None]          # [B, S]
    qkv, dO = inputs(B, S, dh, seed=seed)
    dO = dO * valid.reshape(-1, 1).to(dO.dtype)  # no gradient arrives at padded query rows in the model
    return B, S, W, kv, valid, qkv, dO


def _run_len(K, fwd, bwd, B, S, W, dh, kv, qkv, dO, **kw):
    obuf, out = KB.guarded(B * S, W, BF16, DEV)
    lse, delta = nan_rows(B * S, HEADS), nan_rows(B * S, HEADS)
    fwd(qkv, kv, out, lse, B=B, heads=HEADS, S=S, head_dim=dh, **kw)
    dbuf, dqkv = KB.guarded(B * S, 3 * W, BF16, DEV)
    bwd(qkv, kv, dO, out, lse, delta, dqkv, B=B, heads=HEADS, S=S, head_dim=dh, **kw)
    torch.cuda.synchronize()
    KB.check_guards(obuf, B * S, W, "kv_len out"); KB.check_guards(dbuf, B * S, 3 * W, "kv_len dqkv")
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()  # padded query rows are rows too: never read, but finite
    return out, lse, dqkv


def _check_len(w, what, B, S, W, dh, kv, valid, qkv, dO, out, lse, dqkv, **ref_kw):
    q3, d3, vr = qkv.view(B, S, 3 * W), dO.view(B, S, W), valid.reshape(-1)
    ro, rl, _ = KB.attn_fwd_ref(q3, HEADS, dh, kv_len=kv, **ref_kw)
    check_fwd(w, what, out, lse, ro.reshape(B * S, W), rl.reshape(B * S, HEADS), rows=vr)
    rd = KB.attn_bwd_same_inputs(q3, d3, out.view(B, S, W), lse.view(B, S, HEADS), HEADS, dh, kv_len=kv, q_rows=valid, **ref_kw)
    check_bwd(w, what, dqkv, rd.reshape(B * S, 3 * W), W)
    assert (dqkv[~vr] == 0).all(), f"{what}: the dQ / dK / dV rows of padded positions are not exactly zero"


@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("case", list(LEN_CASES))
def test_kv_len_attention_per_row(K, case, dh):
    """tvts_attn_fwd_len / bwd_len with every length on a tile edge: out / lse2 of the rows < kv_len[b], dqkv of every row (the
    padded positions' rows: zeroed by the wrapper, left exactly zero by the kernels)"""
    B, S, W, kv, valid, qkv, dO = _len_case(case, dh, seed=2000 + dh)
    out, lse, dqkv = _run_len(K, K.attn_fwd_len, K.attn_bwd_len, B, S, W, dh, kv, qkv, dO)
    w = Worst()
    _check_len(w, f"kv_len[{case}, dh {dh}]", B, S, W, dh, kv, valid, qkv, dO, out, lse, dqkv)
    w.report(f"attn_rows kv_len[{case}, dh {dh}]")


def _seed_tensor(v):
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("case", ["S130", "S50"])
def test_attention_probability_dropout_per_row(K, case, p, dh):
    """tvts_attn_fwd_len_drop / bwd_len_drop at two call sites against float64 with the v1 oracle's mask; lse2 is that of the
    undropped scores; p = 0 through the dropout entry points gives the bits of the plain pair"""
    B, S, W, kv, valid, qkv, dO = _len_case(case, dh, seed=3000 + dh)
    seed = 0xF00DF00DF00DF00D
    sd = _seed_tensor(seed)
    w = Worst()
    for site in (1, 4):
        out, lse, dqkv = _run_len(K, K.attn_fwd_len_drop, K.attn_bwd_len_drop, B, S, W, dh, kv, qkv, dO, p=p, seed=sd, site=site)
        mask = V.drop_mask(seed, site, (B, HEADS, S, S), p).to(DEV)
        _check_len(w, f"kv_len_drop[{case}, p {p}, dh {dh}, site {site}]", B, S, W, dh, kv, valid, qkv, dO, out, lse, dqkv,
                   drop_mask=mask, p=p)
    w.report(f"attn_rows kv_len_drop[{case}, p {p}, dh {dh}]")
    plain = _run_len(K, K.attn_fwd_len, K.attn_bwd_len, B, S, W, dh, kv, qkv, dO)
    drop0 = _run_len(K, K.attn_fwd_len_drop, K.attn_bwd_len_drop, B, S, W, dh, kv, qkv, dO, p=0.0, seed=sd, site=1)
    vr = valid.reshape(-1)
    for nm, a, b in zip(("out", "lse2", "dqkv"), drop0, plain):
        KB.assert_equal_bits(a[vr].contiguous(), b[vr].contiguous(), f"p = 0 through the dropout entry points: {nm}")


# ------------------------------------------------------------------------------------------------ query-subset forms (MODE_CLS kernels)
def _delta_check(what, delta, dO, out, rows, dh):
    """delta of the query rows = rowsum(dO o O) per head, within the fp32 summation bound of dh products"""
    a, c = dO[rows].double().reshape(-1, HEADS, dh), out[rows].double().reshape(-1, HEADS, dh)
    n = (dh + 2) * KB.U32
    return KB.assert_within(delta[rows], (a * c).sum(-1), (a * c).abs().sum(-1) * (n / (1 - n)) + 1e-30, what + " delta")


@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("S,nq", [(16, 16), (17, 1), (64, 4), (65, 16), (200, 4)])
def test_tail_query_attention_per_row(K, S, nq, dh):
    """tvts_attn_fwd_tail / bwd_tail: only the last nq rows of every sequence are queries.  out / lse2 / delta are written in the
    query rows alone, dO and O are read there alone (NaN elsewhere), the dQ third of the other rows is the caller's zero"""
    B, W = 2, HEADS * dh
    qkv, dO = inputs(B, S, dh, seed=4000 + S)
    qr = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    qr[:, S - nq:] = True
    rows = qr.reshape(-1)
    dO[~rows] = NAN
    what = f"tail[S {S}, nq {nq}, dh {dh}]"
    obuf, out = KB.guarded(B * S, W, BF16, DEV)
    lse, delta = nan_rows(B * S, HEADS), nan_rows(B * S, HEADS)
    K.attn_fwd_tail(qkv, out, lse, B=B, heads=HEADS, S=S, nq=nq, head_dim=dh)
    dbuf, dqkv = KB.guarded(B * S, 3 * W, BF16, DEV)
    dqkv.zero_()
    K.attn_bwd_tail(qkv, dO, out, lse, delta, dqkv, B=B, heads=HEADS, S=S, nq=nq, head_dim=dh)
    torch.cuda.synchronize()
    KB.check_guards(obuf, B * S, W, what + " out"); KB.check_guards(dbuf, B * S, 3 * W, what + " dqkv")
    for nm, t in (("out", out), ("lse2", lse), ("delta", delta)):
        assert torch.isnan(t[~rows]).all(), f"{what}: {nm} was written outside the query rows"
    q3 = qkv.view(B, S, 3 * W)
    ro, rl, _ = KB.attn_fwd_ref(q3, HEADS, dh)
    w = Worst()
    check_fwd(w, what, out, lse, ro.reshape(B * S, W), rl.reshape(B * S, HEADS), rows=rows)
    w.up("delta (|err| / bound)", _delta_check(what, delta, dO, out, rows, dh))
    rd = KB.attn_bwd_same_inputs(q3, dO.view(B, S, W), out.view(B, S, W), lse.view(B, S, HEADS), HEADS, dh, q_rows=qr)
    check_bwd(w, what, dqkv, rd.reshape(B * S, 3 * W), W)
    assert (dqkv[~rows, :W] == 0).all(), f"{what}: dQ was written outside the query rows"
    w.report("attn_rows " + what)


@pytest.mark.parametrize("dh", [64, 80])
def test_row_query_attention_per_row(K, dh):
    """tvts_attn_fwd_rowq / bwd_rowq: one query per sequence at qpos[b], seeing the keys 0 .. qpos[b].  dK / dV of the keys behind
    the query stay exactly zero, dQ is nonzero in the query row alone"""
    S, qpos = 77, [0, 1, 15, 16, 63, 64, 65, 76]
    B, W = len(qpos), HEADS * dh
    qkv, dO = inputs(B, S, dh, seed=5000 + dh)
    qp = torch.tensor(qpos, dtype=torch.int32, device=DEV)
    qr = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    qr[torch.arange(B, device=DEV), qp.long()] = True
    rows = qr.reshape(-1)
    dO[~rows] = NAN
    what = f"rowq[S {S}, dh {dh}]"
    obuf, out = KB.guarded(B * S, W, BF16, DEV)
    lse, delta = nan_rows(B * S, HEADS), nan_rows(B * S, HEADS)
    K.attn_fwd_rowq(qkv, qp, out, lse, B=B, heads=HEADS, S=S, head_dim=dh)
    dbuf, dqkv = KB.guarded(B * S, 3 * W, BF16, DEV)
    K.attn_bwd_rowq(qkv, qp, dO, out, lse, delta, dqkv, B=B, heads=HEADS, S=S, head_dim=dh)
    torch.cuda.synchronize()
    KB.check_guards(obuf, B * S, W, what + " out"); KB.check_guards(dbuf, B * S, 3 * W, what + " dqkv")
    for nm, t in (("out", out), ("lse2", lse), ("delta", delta)):
        assert torch.isnan(t[~rows]).all(), f"{what}: {nm} was written outside the query rows"
    q3 = qkv.view(B, S, 3 * W)
    ro, rl, _ = KB.attn_fwd_ref(q3, HEADS, dh, causal=True)
    w = Worst()
    check_fwd(w, what, out, lse, ro.reshape(B * S, W), rl.reshape(B * S, HEADS), rows=rows)
    w.up("delta (|err| / bound)", _delta_check(what, delta, dO, out, rows, dh))
    rd = KB.attn_bwd_same_inputs(q3, dO.view(B, S, W), out.view(B, S, W), lse.view(B, S, HEADS), HEADS, dh, causal=True, q_rows=qr)
    check_bwd(w, what, dqkv, rd.reshape(B * S, 3 * W), W)
    behind = (torch.arange(S, device=DEV)[None, :] > qp[:, None]).reshape(-1)
    assert (dqkv[behind, W:] == 0).all(), f"{what}: dK / dV rows behind the query are not exactly zero"
    assert (dqkv[~rows, :W] == 0).all(), f"{what}: dQ was written outside the query rows"
    # (a query at position 0 sees one key: P = 1 and dS = dP - delta = 0 up to the rounding of O, its dQ may be all zeros)
    assert (dqkv[rows, :W] != 0).any(dim=1)[1:].all(), f"{what}: dQ of a query row is all zeros"
    w.report("attn_rows " + what)


# ------------------------------------------------------------------------------------------------ split divided backward
# (mode, T, n, attn_fused, cls_acc): tvts_attn_bwd takes the split passes (delta, dQ, dK / dV, the CLS query, finalize) under
# attn_fused=False, and by size when SPACE has n + 1 > 112 or TIME has T + 1 > 32.  cls_acc: the split passes add the CLS token's
# shares with fp32 atomics into the first B * heads * 3 * dh elements whatever the size of the scratch, so every case passes that
# minimum ("atomic"); one case passes the room for the fused kernels' ordered partials ("parts": the larger buffer is not misread)
SPLIT_CASES = [("time", 8, 30, False, "atomic"), ("time", 33, 3, True, "atomic"), ("space", 2, 111, False, "atomic"),
               ("space", 2, 111, False, "parts"), ("space", 2, 112, True, "atomic"), ("space", 1, 196, True, "atomic"),
               # the first split sizes (SPACE n = 112 above, TIME T = 32); the last fused ones, n = 111 and T = 31, are held per
               # (row, head) by tests/test_attention_fused_rows_gpu.py
               ("time", 32, 3, True, "atomic")]


def _split_divided(K, tag, mode, B, T, n, heads, dh, fused, acc_kind, seed):
    S, W = 1 + T * n, heads * dh
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3 * W, generator=g).bfloat16().to(DEV)
    dO = torch.randn(B * S, W, generator=g).bfloat16().to(DEV)
    parts = max(T, -(-n // 28))
    with K.options(attn_fused=fused):
        obuf, out = KB.guarded(B * S, W, BF16, DEV)
        lse, delta = nan_rows(B * S, heads), nan_rows(B * S, heads)
        ws = torch.full((B * heads * parts * (dh + 2),), NAN, device=DEV)
        K.attn_fwd_divided(mode, qkv, out, lse, ws, B=B, heads=heads, S=S, T=T, n=n, head_dim=dh)
        dbuf, dqkv = KB.guarded(B * S, 3 * W, BF16, DEV)
        # room for one ordered partial per block of the fused kernels, or the minimum the fp32 atomics need
        acc = torch.full((B * heads * (parts if acc_kind == "parts" else 1) * 3 * dh,), NAN, device=DEV)
        K.attn_bwd(mode, qkv, dO, out, lse, delta, dqkv, B=B, heads=heads, S=S, T=T, n=n, cls_acc=acc, head_dim=dh)
    torch.cuda.synchronize()
    KB.check_guards(obuf, B * S, W, tag + " out"); KB.check_guards(dbuf, B * S, 3 * W, tag + " dqkv")
    q3 = qkv.view(B, S, 3 * W)
    ro, rl, _ = KB.divided_fwd_ref(q3, heads, dh, mode, T, n)
    w, wc = KB.rows_check(out, ro.reshape(B * S, W), TOL["out"], heads, B, S, tag + " out")
    KB.bound_line(tag + " out (per-row rel)", w); KB.bound_line(tag + " out CLS (per-row rel)", wc)
    KB.bound_line(tag + " lse2 (|err| / 1e-3)", KB.assert_within(lse, rl.reshape(B * S, heads), KB.LSE2_TOL, tag + " lse2"))
    rd = KB.divided_bwd_same_inputs(q3, dO.view(B, S, W), out.view(B, S, W), lse.view(B, S, heads), heads, dh, mode, T, n)
    rd = rd.reshape(B * S, 3 * W)
    for i, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(i * W, (i + 1) * W)
        w, wc = KB.rows_check(dqkv[:, sl], rd[:, sl], TOL[nm], heads, B, S, f"{tag} {nm}")
        KB.bound_line(f"{tag} {nm} (per-row rel)", w); KB.bound_line(f"{tag} {nm} CLS (per-row rel)", wc)


@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("mode,T,n,fused,acc_kind", SPLIT_CASES)
def test_split_divided_backward_per_row(K, mode, T, n, fused, acc_kind, dh):
    """the whole backward of one divided site through the split passes, against float64 on the forward's bf16 output and lse2;
    the CLS rows (cross-group sums through cls_acc) are their own group"""
    tag = f"attn_rows split[{mode}, T {T}, n {n}, dh {dh}, fused opt {int(fused)}, cls_acc {acc_kind}]"
    _split_divided(K, tag, mode, 2, T, n, HEADS, dh, fused, acc_kind, seed=6000 + 7 * T + n)


def test_split_divided_backward_per_row_at_the_b16_time_geometry(K):
    """The case test_divided_attention_per_row_at_the_step_geometry's note was about: B/16 time groups (9 keys per query) through
    the split backward.  Against float64 autograd its dQ is off by up to 0.12 per slice -- for ANY backward that takes delta from
    the bf16 output (tests/test_kernel_bounds_cpu.py); against the same inputs it is held to ATTN_ROW_TOL like every other case."""
    c = KB.DIVIDED["B16"]
    _split_divided(K, "attn_rows split[B16 time, B 2]", "time", 2, c["T"], c["n"], c["heads"], c["dh"], False, "parts", seed=5)
