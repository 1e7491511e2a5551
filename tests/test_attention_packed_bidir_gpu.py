"""The BIDIRECTIONAL packed attention kernels of the v1 text tower under arch["text_unpadded"] (DESIGN.md 8b "v1"):
tvts_attn_fwd_packed_bidir / tvts_attn_bwd_packed_bidir with and without dropout, the one-query form tvts_attn_fwd_packed_first and
tvts_dropout_rows_packed.

Forward and backward are held per (row, head) to the bound functions tests/test_attention_rows_gpu.py applies to
tvts_attn_*_len(_drop) (kernel_bounds.ATTN_ROW_TOL, LSE2_TOL, the float64 backward on what the kernel READ), the dropout mask being the
counter rule evaluated on the host: the oracle's drop_mask over the PADDED index space [N, heads, L_pad, L_pad].  The mask rule itself
is checked exactly (one-hot V, equal scores), against the padded kernels' rule at two values of L_pad."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
from oracle import tvts_v1_oracle as V  # noqa: E402  (checker only: the dropout mask generator)

DEV = "cuda:0"
BF16 = torch.bfloat16
HEADS = 2
TOL = KB.ATTN_ROW_TOL
SEED = 0xF00DF00DF00DF00D
SITE = 3


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def _is_prime(n):
    return n > 1 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def _rand_prime(n, seed):
    lens = torch.randint(1, 81, (n,), generator=torch.Generator().manual_seed(seed)).tolist()
    for last in range(1, 81):
        lens[-1] = last
        if _is_prime(sum(lens)):
            return lens
    raise AssertionError("no prime M within one caption's reach")


LENGTH_SETS = {
    # every tile-class edge (classes 1-16, 17-32, 33-48, 49-80), unsorted
    "edges": [33, 1, 80, 16, 2, 49, 15, 64, 17, 79, 31, 32, 50, 47, 48, 5],
    "all_equal_24": [24] * 16,
    "prime_M": _rand_prime(16, 5),
}
assert _is_prime(sum(LENGTH_SETS["prime_M"]))
assert set([1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 79, 80]) <= set(LENGTH_SETS["edges"])


def _seed_tensor(v=SEED):
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v], dtype=torch.int64, device=DEV)


def _seq_start(lens):
    s = torch.zeros(len(lens) + 1, dtype=torch.int32)
    s[1:] = torch.tensor(lens).cumsum(0)
    return s.to(DEV)


def _by_length(lens):
    """{L: (sequence indices [count], row indices [count, L])}"""
    d, s = {}, 0
    for i, n in enumerate(lens):
        d.setdefault(n, ([], []))
        d[n][0].append(i)
        d[n][1].append(s)
        s += n
    return {n: (torch.tensor(idx), torch.tensor(st, device=DEV)[:, None] + torch.arange(n, device=DEV)[None, :]) for n, (idx, st) in d.items()}


def _flat_nan(rows, cols, guard=3):
    buf = torch.full(((rows + guard) * cols,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[:rows * cols].view(rows, cols)


def _host_mask(N, L_pad, p, seed=SEED, site=SITE):
    """the counter rule on the host: keep / (1 - p) of every (caption, head, query, key) of the PADDED index space"""
    return V.drop_mask(seed, site, (N, HEADS, L_pad, L_pad), p)


def _inputs(lens, seed):
    M, W = sum(lens), HEADS * 64
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(M, 3 * W, generator=g).bfloat16().to(DEV)
    dO = torch.randn(M, W, generator=g).bfloat16().to(DEV)
    return qkv, dO


_REFS = {}


def _case(name, p, L_pad):
    """inputs and the float64 forward reference of a length set, made once per (set, p)"""
    key = (name, p, L_pad)
    if key not in _REFS:
        lens = LENGTH_SETS[name]
        N, M, W = len(lens), sum(lens), HEADS * 64
        qkv, dO = _inputs(lens, 100 + len(name))
        mask = _host_mask(N, L_pad, p) if p > 0 else None
        ro = torch.empty(M, W, dtype=torch.float64, device=DEV)
        rl = torch.empty(M, HEADS, dtype=torch.float64, device=DEV)
        for L, (idx, rows) in _by_length(lens).items():
            m = None if mask is None else mask[idx][:, :, :L, :L].to(DEV)
            o, l2, _ = KB.attn_fwd_ref(qkv[rows.reshape(-1)].view(-1, L, 3 * W), HEADS, 64, drop_mask=m, p=p)
            ro[rows.reshape(-1)], rl[rows.reshape(-1)] = o.reshape(-1, W), l2.reshape(-1, HEADS)
        _REFS[key] = dict(lens=lens, N=N, M=M, W=W, qkv=qkv, dO=dO, ss=_seq_start(lens), mask=mask, ro=ro, rl=rl)
    return _REFS[key]


def _fwd(K, c, p, L_pad, with_lse=True, max_len=None):
    M, W = c["M"], c["W"]
    obuf, out = KB.guarded(M, W, BF16, DEV)
    lbuf, lse = _flat_nan(M, HEADS)
    K.attn_fwd_packed_bidir(c["qkv"], c["ss"], out, lse if with_lse else None, N=c["N"], heads=HEADS,
                            max_len=max(c["lens"]) if max_len is None else max_len, L_pad=L_pad, p=p, seed=_seed_tensor(), site=SITE)
    torch.cuda.synchronize()
    KB.check_guards(obuf, M, W, "bidirectional packed attention out")
    assert bool(torch.isnan(lbuf[M * HEADS:]).all()), "lse2 written past its rows"
    return out, lse


def _bwd(K, c, p, L_pad, out, lse, max_len=None):
    M, W = c["M"], c["W"]
    buf, dqkv = KB.guarded(M, 3 * W, BF16, DEV)  # poisoned: NaN everywhere
    dbuf, delta = _flat_nan(M, HEADS)
    K.attn_bwd_packed_bidir(c["qkv"], c["ss"], c["dO"], out, lse, delta, dqkv, N=c["N"], heads=HEADS,
                            max_len=max(c["lens"]) if max_len is None else max_len, L_pad=L_pad, p=p, seed=_seed_tensor(), site=SITE)
    torch.cuda.synchronize()
    KB.check_guards(buf, M, 3 * W, "bidirectional packed attention backward dqkv")
    assert bool(torch.isnan(dbuf[M * HEADS:]).all()), "delta written past its rows"
    return dqkv, delta


# ------------------------------------------------------------------------------------------------ forward and backward against float64
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_bidir_forward_and_backward_per_row(K, name, p):
    L_pad = max(LENGTH_SETS[name])  # the padded step's L: the longest caption
    c = _case(name, p, L_pad)
    lens, N, M, W = c["lens"], c["N"], c["M"], c["W"]
    what = f"bidirectional packed attention [{name}, p {p}]"
    out, lse = _fwd(K, c, p, L_pad)
    wo = KB.assert_rows_within(out, c["ro"], TOL["out"], groups=HEADS, what=what + " out", out_dtype=BF16)
    wl = KB.assert_within(lse.double(), c["rl"], KB.LSE2_TOL, what + " lse2")
    nolse, _ = _fwd(K, c, p, L_pad, with_lse=False)
    KB.assert_equal_bits(nolse, out, what + ": out of the call without lse2")
    # backward: float64 on what the kernel read (its own bf16 output and log-sum-exp), the mask from the host rule
    ref = torch.full((M, 3 * W), float("nan"), dtype=torch.float64, device=DEV)
    for L, (idx, rows) in _by_length(lens).items():
        r = rows.reshape(-1)
        m = None if c["mask"] is None else c["mask"][idx][:, :, :L, :L].to(DEV)
        ref[r] = KB.attn_bwd_same_inputs(c["qkv"][r].view(-1, L, 3 * W), c["dO"][r].view(-1, L, W), out[r].view(-1, L, W),
                                         lse[r].view(-1, L, HEADS), HEADS, 64, drop_mask=m, p=p).reshape(-1, 3 * W)
    dqkv, delta = _bwd(K, c, p, L_pad, out, lse)
    assert not bool(torch.isnan(dqkv).any()), what + ": a row of a valid sequence kept the poison in one of the three thirds"
    worst = {}
    for i, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(i * W, (i + 1) * W)
        worst[nm] = KB.assert_rows_within(dqkv[:, sl], ref[:, sl], TOL[nm], groups=HEADS, what=f"{what} {nm}", out_dtype=BF16)
    print(f"{what}: worst per-(row, head) relative error out {wo:.3e} dq {worst['dq']:.3e} dk {worst['dk']:.3e} dv {worst['dv']:.3e} "
          f"(gates {TOL['out']}, {TOL['dq']}, {TOL['dk']}, {TOL['dv']}); lse2 |err| / 1e-3 {wl:.3e}")
    dref = (c["dO"].double() * out.double()).view(M, HEADS, 64)
    KB.assert_within(delta.double(), dref.sum(-1), KB.sum_bound(dref.abs().sum(-1), 64), what + " delta")
    again, delta2 = _bwd(K, c, p, L_pad, out, lse)
    KB.assert_equal_bits(again, dqkv, what + ": second run")
    KB.assert_equal_bits(delta2, delta, what + ": delta, second run")
    if max(lens) <= 48 and p == 0.0:  # more tile classes launched, nothing changed (L_pad has no part in a call with p = 0)
        more, lse_more = _fwd(K, c, p, 80, max_len=80)
        KB.assert_equal_bits(more, out, what + ": max_len 80")
        KB.assert_equal_bits(_bwd(K, c, p, 80, more, lse_more, max_len=80)[0], dqkv, what + ": backward, max_len 80")


def test_p0_ignores_seed_and_l_pad(K):
    """p == 0 runs the kernels without generator work: no seed needed, L_pad without influence"""
    c = _case("edges", 0.0, 80)
    out, lse = _fwd(K, c, 0.0, 80)
    _, o2 = KB.guarded(c["M"], c["W"], BF16, DEV)
    K.attn_fwd_packed_bidir(c["qkv"], c["ss"], o2, None, N=c["N"], heads=HEADS, max_len=80, L_pad=200, p=0.0, seed=None, site=9)
    KB.assert_equal_bits(o2, out, "p = 0 without a seed")


# ------------------------------------------------------------------------------------------------ the mask rule, exactly
MASK_LENS = [64, 1, 17, 33, 49, 16, 50, 2, 32, 48]


@pytest.mark.parametrize("L_pad", [64, 77])
def test_mask_rule_exact(K, L_pad):
    """q = k = 0 and one-hot V rows (V[j] = e_j inside every head): every probability is 1 / len, so out[q, k] is
    keep(q, k) / (len * (1 - p)) to the rounding of one bf16: within one bf16 step (unit in the last place) of that value.  The
    kernel keeps the padded kernels' arithmetic -- fl(1 / (1 - p)) is rounded to bf16 as the MFMA operand, the result to bf16 again,
    two round-to-nearest steps of half a unit each; measured worst |err| = 1.05 * 2^-8 |value|.  Its pattern of exact
    zeros is the host rule's over the index ((i * heads + h) * L_pad + q) * L_pad + k, for L_pad = the longest length and a larger one."""
    p, lens = 0.1, MASK_LENS
    N, M, W = len(lens), sum(lens), HEADS * 64
    qkv = torch.zeros(M, 3 * W, dtype=BF16, device=DEV)
    s = 0
    for n in lens:
        for h in range(HEADS):
            qkv[s:s + n, 2 * W + h * 64:2 * W + h * 64 + n] = torch.eye(n, dtype=BF16, device=DEV)
        s += n
    c = dict(lens=lens, N=N, M=M, W=W, qkv=qkv, ss=_seq_start(lens))
    out, _ = _fwd(K, c, p, L_pad)
    mask = _host_mask(N, L_pad, p)  # keep / (1 - p), float32
    want = torch.zeros(M, W, dtype=torch.float64)
    s = dropped = 0
    for i, n in enumerate(lens):
        for h in range(HEADS):
            want[s:s + n, h * 64:h * 64 + n] = (mask[i, h, :n, :n] != 0).double() / (n * (1.0 - p))
            dropped += int((mask[i, h, :n, :n] == 0).sum())
        s += n
    want = want.to(DEV)
    assert bool(((out == 0) == (want == 0)).all()), f"L_pad {L_pad}: the pattern of dropped probabilities is not the host rule's"
    assert 0.05 < dropped / (HEADS * sum(n * n for n in lens)) < 0.15  # (the rule drops what p says)
    ulp = torch.where(want > 0, torch.exp2(torch.floor(torch.log2(want.clamp_min(1e-300))) - 7), torch.zeros_like(want))
    w = KB.assert_within(out.double(), want, ulp + 1e-300, f"mask rule, L_pad {L_pad}")
    print(f"mask rule, L_pad {L_pad}: worst |err| / (one bf16 step) {w:.3f}; worst relative error "
          f"{float(((out.double() - want).abs() / want.clamp_min(1e-300)).max()):.3e} (2^-8 = {2.0 ** -8:.3e})")


@pytest.mark.parametrize("L_pad", [64, 77])
def test_mask_rule_in_the_backward(K, L_pad):
    """the backward regenerates the forward's mask: with q = k = 0, one-hot V rows and dO = e_0 in every head, dV[k, 0] is
    sum_q P_drop[q, k] = (kept queries of key k) / (len * (1 - p)): zero exactly where the host rule drops every query"""
    p, lens = 0.5, [3, 1, 20, 2, 64]
    N, M, W = len(lens), sum(lens), HEADS * 64
    qkv = torch.zeros(M, 3 * W, dtype=BF16, device=DEV)
    s = 0
    for n in lens:
        for h in range(HEADS):
            qkv[s:s + n, 2 * W + h * 64:2 * W + h * 64 + n] = torch.eye(n, dtype=BF16, device=DEV)
        s += n
    dO = torch.zeros(M, W, dtype=BF16, device=DEV)
    dO[:, 0::64] = 1.0
    c = dict(lens=lens, N=N, M=M, W=W, qkv=qkv, dO=dO, ss=_seq_start(lens))
    out, lse = _fwd(K, c, p, L_pad)
    dqkv, _ = _bwd(K, c, p, L_pad, out, lse)
    mask = _host_mask(N, L_pad, p)
    want = torch.zeros(M, HEADS, dtype=torch.float64)
    s = 0
    for i, n in enumerate(lens):
        want[s:s + n] = ((mask[i, :, :n, :n] != 0).double().sum(1) / (n * (1.0 - p))).T
        s += n
    got = dqkv[:, 2 * W::64].double()  # dV[:, head column 0]
    want = want.to(DEV)
    assert bool(((got == 0) == (want == 0)).all()), "dV: the keys whose every query was dropped are not the host rule's"
    assert int((want == 0).sum()) > 0
    # (P = 1 / len is rounded to bf16 for the MFMA, the fp32 sum of up to 64 such terms times 1 / (1 - p) = 2 once more for the
    # output: two roundings of KB.U_OUT[bf16] each)
    KB.assert_within(got, want, 2 * KB.U_OUT[BF16] * want.abs() + 1e-300, f"dV column sums, L_pad {L_pad}")


def test_forward_gives_the_bits_of_the_padded_kernel(K):
    """sequences of up to 64 rows are ONE key tile of tvts_attn_fwd_len_drop, and the packed kernel keeps that kernel's arithmetic
    operation for operation: on the same (seed, site) and L_pad = S the packed call gives the padded call's out at every valid row,
    bit for bit (the log-sum-exp to 1e-5: the two kernels' m + log2(l) differ in the last place of a few rows)"""
    p, lens, S = 0.1, MASK_LENS, 64
    N, M, W = len(lens), sum(lens), HEADS * 64
    qkv, _ = _inputs(lens, 77)
    c = dict(lens=lens, N=N, M=M, W=W, qkv=qkv, ss=_seq_start(lens))
    rows = torch.cat([i * S + torch.arange(n) for i, n in enumerate(lens)]).to(DEV)
    qp = torch.zeros(N * S, 3 * W, dtype=BF16, device=DEV)
    qp[rows] = qkv
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for pp in (p, 0.0):
        out, lse = _fwd(K, c, pp, S)
        op, lp = torch.empty(N * S, W, dtype=BF16, device=DEV), torch.empty(N * S, HEADS, device=DEV)
        if pp > 0:
            K.attn_fwd_len_drop(qp, kv, op, lp, B=N, heads=HEADS, S=S, p=pp, seed=_seed_tensor(), site=SITE)
        else:
            K.attn_fwd_len(qp, kv, op, lp, B=N, heads=HEADS, S=S)
        KB.assert_equal_bits(out.contiguous(), op[rows], f"packed against padded forward, p {pp}: out")
        KB.assert_within(lse.double(), lp[rows].double(), 1e-5, f"packed against padded forward, p {pp}: lse2")


# ------------------------------------------------------------------------------------------------ tvts_dropout_rows_packed
@pytest.mark.parametrize("L_pad", [50, 61])
def test_dropout_rows_packed_bit_equal(K, L_pad):
    """against tvts_dropout_rows on the padded copy, at the valid positions: bit-equal in every output form; rows and columns
    outside stay untouched"""
    lens = [50, 1, 17, 33, 2, 49, 16]
    N, M, cols, p = len(lens), sum(lens), 328, 0.1
    g = torch.Generator().manual_seed(7)
    x, res = torch.randn(M, cols, generator=g).to(DEV), torch.randn(M, cols, generator=g).to(DEV)
    ss, sd = _seq_start(lens), _seed_tensor()
    rows = torch.cat([i * L_pad + torch.arange(n) for i, n in enumerate(lens)]).to(DEV)  # padded row of every packed row
    xp, rp = torch.zeros(N * L_pad, cols, device=DEV), torch.zeros(N * L_pad, cols, device=DEV)
    xp[rows], rp[rows] = x, res
    wantf, wantb = torch.empty_like(xp), torch.empty(N * L_pad, cols, dtype=BF16, device=DEV)
    K.dropout_rows(xp, p=p, seed=sd, site=4, residual=rp, out=wantf, out_bf16=wantb)
    fbuf, outf = KB.guarded(M, cols, torch.float32, DEV)
    bbuf, outb = KB.guarded(M, cols, BF16, DEV)
    K.dropout_rows_packed(x, ss, N=N, L_pad=L_pad, p=p, seed=sd, site=4, residual=res, out=outf, out_bf16=outb)
    torch.cuda.synchronize()
    KB.check_guards(fbuf, M, cols, "dropout_rows_packed out"); KB.check_guards(bbuf, M, cols, "dropout_rows_packed out_bf16")
    KB.assert_equal_bits(outf, wantf[rows], "dropout_rows_packed out")
    KB.assert_equal_bits(outb, wantb[rows], "dropout_rows_packed out_bf16")
    # the backward call: no residual, bf16 only; and against the oracle's restatement of the generator
    K.dropout_rows(xp, p=p, seed=sd, site=6, out_bf16=wantb)
    _, ob = KB.guarded(M, cols, BF16, DEV)
    K.dropout_rows_packed(x, ss, N=N, L_pad=L_pad, p=p, seed=sd, site=6, out_bf16=ob)
    KB.assert_equal_bits(ob, wantb[rows], "dropout_rows_packed out_bf16 alone")
    mask = V.drop_mask(SEED, 6, (N * L_pad, cols), p).to(DEV)[rows]
    KB.assert_equal_bits(ob, torch.where(mask != 0, x * mask, torch.zeros_like(x)).bfloat16(), "dropout_rows_packed against the host rule")
    assert 0.05 < float((ob == 0).float().mean()) < 0.15


# ------------------------------------------------------------------------------------------------ the one-query form
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_first_row_form(K, name):
    c = _case(name, 0.0, max(LENGTH_SETS[name]))
    N, M, W = c["N"], c["M"], c["W"]
    obuf, out = KB.guarded(M, W, BF16, DEV)
    K.attn_fwd_packed_first(c["qkv"], c["ss"], out, N=N, heads=HEADS, max_len=max(c["lens"]))
    torch.cuda.synchronize()
    KB.check_guards(obuf, M, W, "first-row form")
    first = c["ss"][:-1].long()
    other = torch.ones(M, dtype=torch.bool, device=DEV)
    other[first] = False
    assert bool(torch.isnan(out[other]).all()), "first-row form: a row that is no sequence's first one was written"
    w = KB.assert_rows_within(out[first], c["ro"][first], TOL["out"], groups=HEADS, what=f"first-row form [{name}]", out_dtype=BF16)
    print(f"first-row form [{name}]: worst per-(row, head) relative error {w:.3e} (gate {TOL['out']})")


# ------------------------------------------------------------------------------------------------ malformed descriptors
MALFORMED = {  # descriptors over M = 137 rows (lengths 20, 5, 33, 70, 9 when well formed)
    "length_0": [0, 20, 20, 58, 128, 137],
    "length_81": [0, 20, 101, 110, 128, 137],
    "start_beyond_M": [0, 20, 25, 58, 140, 137],
}


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("bad", list(MALFORMED))
def test_malformed_sequence_is_left_untouched(K, bad, p):
    M, W, st = 137, HEADS * 64, MALFORMED[bad]
    seqs = [(a, b - a) for a, b in zip(st, st[1:]) if 0 <= a and b <= M and 1 <= b - a <= 80]
    assert len(seqs) in (3, 4)
    covered = torch.zeros(M, dtype=torch.bool, device=DEV)
    for a, n in seqs:
        covered[a:a + n] = True
    qkv, dO = _inputs([M], 31 + len(bad))
    c = dict(lens=[80], N=5, M=M, W=W, qkv=qkv, dO=dO, ss=torch.tensor(st, dtype=torch.int32, device=DEV))
    out, lse = _fwd(K, c, p, 80)
    first = torch.full((M, W), float("nan"), dtype=BF16, device=DEV)
    K.attn_fwd_packed_first(qkv, c["ss"], first, N=5, heads=HEADS, max_len=80)
    dqkv, delta = _bwd(K, c, p, 80, out, lse)
    what = f"bidirectional packed attention, {bad}, p {p}"
    assert bool(torch.isnan(out[~covered]).all()) and bool(torch.isnan(lse[~covered]).all()), what + ": the forward wrote skipped rows"
    assert bool(torch.isnan(first[~covered]).all()), what + ": the first-row form wrote skipped rows"
    assert bool(torch.isnan(dqkv[~covered]).all()) and bool(torch.isnan(delta[~covered]).all()), what + ": the backward wrote skipped rows"
    assert not bool(torch.isnan(out[covered]).any()) and not bool(torch.isnan(dqkv[covered]).any())
    assert int(torch.isfinite(first).all(1).sum()) == len(seqs)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(K):
    c = _case("edges", 0.0, 80)
    N, M, W, sd = c["N"], c["M"], c["W"], _seed_tensor()
    out, lse = _fwd(K, c, 0.0, 80)

    def fwd(max_len=80, L_pad=80, p=0.1, seed=sd, ld_extra=8):
        buf = torch.full((M, W + ld_extra), float("nan"), dtype=BF16, device=DEV)
        with pytest.raises(K.HipError, match="-22"):
            K.attn_fwd_packed_bidir(c["qkv"], c["ss"], buf[:, :W], None, N=N, heads=HEADS, max_len=max_len, L_pad=L_pad, p=p, seed=seed, site=1)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()), "a refused call launched a kernel"

    def bwd(max_len=80, L_pad=80, p=0.1, seed=sd, ld_extra=8, lse2=lse, dO=c["dO"]):
        buf = torch.full((M, 3 * W + ld_extra), float("nan"), dtype=BF16, device=DEV)
        _, delta = _flat_nan(M, HEADS)
        with pytest.raises(K.HipError, match="-22"):
            K.attn_bwd_packed_bidir(c["qkv"], c["ss"], dO, out, lse2, delta, buf[:, :3 * W], N=N, heads=HEADS, max_len=max_len,
                                    L_pad=L_pad, p=p, seed=seed, site=1)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()) and bool(torch.isnan(delta).all()), "a refused call launched a kernel"

    for call in (fwd, bwd):
        call(max_len=81, L_pad=81)       # as the causal entries
        call(ld_extra=4)                 # ldo / lddq no multiple of 8
        call(L_pad=79)                   # L_pad < max_len
        call(p=1.0)
        call(p=-0.1)
        call(p=float("nan"))
        call(seed=None)                  # p > 0 needs the seed
    bwd(lse2=None)

    def first(max_len=80, ld_extra=8):
        buf = torch.full((M, W + ld_extra), float("nan"), dtype=BF16, device=DEV)
        with pytest.raises(K.HipError, match="-22"):
            K.attn_fwd_packed_first(c["qkv"], c["ss"], buf[:, :W], N=N, heads=HEADS, max_len=max_len)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all())
    first(max_len=81)
    first(ld_extra=4)

    x = torch.randn(M, 64, device=DEV)

    def drop(p=0.1, seed=sd, L_pad=80, give_out=True):
        o = torch.full((M, 64), float("nan"), device=DEV)
        with pytest.raises(K.HipError, match="-22"):
            K.dropout_rows_packed(x, c["ss"], N=N, L_pad=L_pad, p=p, seed=seed, site=0, out=o if give_out else None)
        torch.cuda.synchronize()
        assert bool(torch.isnan(o).all())
    drop(p=1.0)
    drop(p=-0.5)
    drop(L_pad=0)
    drop(give_out=False)
