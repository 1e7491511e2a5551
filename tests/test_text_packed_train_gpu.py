"""Training on PACKED captions (arch["text_packed"]): the _lse forward entries, tvts_attn_bwd_packed and its last-row
form against float64 on what the kernels read, tvts_text_embed_bwd_packed against float64 sums, and the engine's packed text tower
against the oracle's padded step and against the padded engine on the same batch."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
from oracle import tvts_oracle as O  # noqa: E402  (checker only)

DEV = "cuda:0"
BF16 = torch.bfloat16
EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 76, 77]
ARGS = types.SimpleNamespace(local_rank=0, rank=0, world_size=1)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def _is_prime(n):
    return n > 1 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def _rand_prime(n, seed):
    """n lengths uniform in [1, 77], unsorted, the last one moved until M is prime"""
    lens = torch.randint(1, 78, (n,), generator=torch.Generator().manual_seed(seed)).tolist()
    for last in range(1, 78):
        lens[-1] = last
        if _is_prime(sum(lens)):
            return lens
    raise AssertionError("no prime M within one caption's reach")


def _shuffled(lens, seed):
    return [lens[i] for i in torch.randperm(len(lens), generator=torch.Generator().manual_seed(seed)).tolist()]


LENGTH_SETS = {
    "edges_sorted": sorted(EDGES),
    "edges_shuffled": _shuffled(EDGES, 1),
    "edges_descending": sorted(EDGES, reverse=True),
    "one_of_1": [1],
    "one_of_77": [77],
    "all_equal_24": [24] * 50,
    "any_300_prime_M": _rand_prime(300, 3),
}
assert _is_prime(sum(LENGTH_SETS["any_300_prime_M"]))
HEADS = [3, 8]  # an odd count: a wrong head stride cannot land in another head of the same row


def _seq_start(lens):
    s = torch.zeros(len(lens) + 1, dtype=torch.int32)
    s[1:] = torch.tensor(lens).cumsum(0)
    return s.to(DEV)


def _seqs(lens):
    out, s = [], 0
    for n in lens:
        out.append((s, n))
        s += n
    return out


def _by_length(seqs):
    """{L: row indices [count, L]} of the (start, length) sequences"""
    d = {}
    for s, n in seqs:
        d.setdefault(n, []).append(s)
    return {n: (torch.tensor(st, device=DEV)[:, None] + torch.arange(n, device=DEV)[None, :]) for n, st in d.items()}


def _flat_nan(rows, cols, guard=3):
    """a contiguous fp32 [rows, cols] (lse2 / delta have no leading dimension) with NaN guard rows behind it -> (buffer, view)"""
    buf = torch.full(((rows + guard) * cols,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[:rows * cols].view(rows, cols)


def _tail_untouched(buf, rows, cols, what):
    assert bool(torch.isnan(buf[rows * cols:]).all()), f"{what}: written past its {rows} rows"


_CASES = {}


def _case(K, name, heads):
    """inputs, the packed forward's outputs (with and without lse2) and the float64 forward reference of a length set, made once"""
    key = (name, heads)
    if key in _CASES:
        return _CASES[key]
    lens = LENGTH_SETS[name]
    N, M, W = len(lens), sum(lens), heads * 64
    g = torch.Generator(device=DEV).manual_seed(1000 + 7 * N + heads)
    qkv = torch.randn(M, 3 * W, generator=g, device=DEV).bfloat16()
    dO = torch.randn(M, W, generator=g, device=DEV).bfloat16()
    ss = _seq_start(lens)
    _, plain = KB.guarded(M, W, BF16, DEV)
    K.attn_fwd_packed(qkv, ss, plain, N=N, heads=heads, max_len=max(lens))
    obuf, out = KB.guarded(M, W, BF16, DEV)
    lbuf, lse = _flat_nan(M, heads)
    K.attn_fwd_packed(qkv, ss, out, N=N, heads=heads, max_len=max(lens), lse2=lse)
    torch.cuda.synchronize()
    KB.check_guards(obuf, M, W, "packed attention out (lse form)")
    _tail_untouched(lbuf, M, heads, "packed attention lse2")
    ref_lse = torch.empty(M, heads, dtype=torch.float64, device=DEV)
    for L, rows in _by_length(_seqs(lens)).items():
        _, l2, _ = KB.attn_fwd_ref(qkv[rows.reshape(-1)].view(-1, L, 3 * W), heads, 64, causal=True)
        ref_lse[rows.reshape(-1)] = l2.reshape(-1, heads)
    c = _CASES[key] = dict(lens=lens, N=N, M=M, W=W, qkv=qkv, dO=dO, ss=ss, plain=plain, out=out, lse=lse, ref_lse=ref_lse)
    return c


def _bwd_ref(qkv, dO, O_read, lse_read, seqs, heads, last_only=False):
    """float64 dqkv [M, 3W] of the valid (start, length) sequences from what the kernel read, evaluated per length as a [count, L]
    rectangular causal problem (kernel_bounds.attn_bwd_same_inputs); rows of no valid sequence are NaN.  -> (ref, covered rows)"""
    M, W = qkv.shape[0], qkv.shape[1] // 3
    ref = torch.full((M, 3 * W), float("nan"), dtype=torch.float64, device=DEV)
    covered = torch.zeros(M, dtype=torch.bool, device=DEV)
    for L, rows in _by_length(seqs).items():
        r = rows.reshape(-1)
        q_rows = None
        if last_only:
            q_rows = torch.zeros(rows.shape, dtype=torch.bool, device=DEV)
            q_rows[:, -1] = True
        d = KB.attn_bwd_same_inputs(qkv[r].view(-1, L, 3 * W), dO[r].view(-1, L, W), O_read[r].view(-1, L, W),
                                    lse_read[r].view(-1, L, heads), heads, 64, causal=True, q_rows=q_rows)
        ref[r] = d.reshape(-1, 3 * W)
        covered[r] = True
    return ref, covered


def _check_thirds(got, ref, rows, heads, what, dq_rows=None, one_token=False):
    """the three thirds of dqkv at `rows` per (row, head) under ATTN_ROW_TOL (dq at dq_rows when the form has fewer queries).
    one_token: every sequence has ONE token -- softmax over one key is constant, so dS, dQ and dK are identically zero in exact
    arithmetic and the relative gate has no denominator.  The kernel forms dS = P (dP - delta) from two fp32 dot products of the same
    64 products (dP = dO . v, delta = dO . O with O = v): each is within gamma_64 sum|dO_d v_d| of the exact value (u = 2^-24), P <= 1
    up to the 1e-3 of its lse2, so |dS| <= 2.1 gamma_64 sum|dO v| / 8 and |dQ_d| <= |dS| |k_d|, |dK_d| <= |dS| |q_d|; the bf16 rounding
    of the result adds 2^-8 of that.  dV = P^T dO keeps its relative gate."""
    W = got.shape[1] // 3
    worst = {}
    for i, nm in enumerate(("dq", "dk", "dv")):
        rr = dq_rows if (nm == "dq" and dq_rows is not None) else rows
        g, r = got[rr][:, i * W:(i + 1) * W], ref[rr][:, i * W:(i + 1) * W]
        if one_token and nm != "dv":
            worst[nm] = 0.0
            continue
        worst[nm] = KB.assert_rows_within(g, r, KB.ATTN_ROW_TOL[nm], groups=heads, what=f"{what} {nm}", out_dtype=BF16)
    return worst


def _one_token_bound(c, heads):
    """per-element bound on |dQ| and |dK| of one-token sequences (see _check_thirds) -> (bq, bk) [M, W]"""
    W = c["W"]
    q, k, v = (c["qkv"][:, i * W:(i + 1) * W].double() for i in range(3))
    s = (c["dO"].double().abs() * v.abs()).view(-1, heads, 64).sum(-1)  # [M, heads]
    gam = 64 * 2.0 ** -24 / (1 - 64 * 2.0 ** -24)
    ds = (2.1 * gam * s / 8.0).repeat_interleave(64, dim=1) * (1 + 2.0 ** -8)
    return ds * k.abs() + 1e-30, ds * q.abs() + 1e-30


# ------------------------------------------------------------------------------------------------ 1. the _lse forward entries
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_lse_forms(K, name, heads):
    c = _case(K, name, heads)
    N, M, W = c["N"], c["M"], c["W"]
    what = f"packed attention with lse2 [{name}, {heads} heads]"
    KB.assert_equal_bits(c["out"], c["plain"], what + ": out against the entry without lse2")
    err = float((c["lse"].double() - c["ref_lse"]).abs().max())
    print(f"{what}: worst |lse2 - float64| {err:.3e} (gate {KB.LSE2_TOL})")
    assert torch.isfinite(c["lse"]).all() and err < KB.LSE2_TOL, err
    # the one-query form: its N rows of out and lse2, and nothing else
    last = (c["ss"][1:] - 1).long()
    _, plain = KB.guarded(M, W, BF16, DEV)
    K.attn_fwd_packed(c["qkv"], c["ss"], plain, N=N, heads=heads, max_len=max(c["lens"]), last_only=True)
    obuf, out = KB.guarded(M, W, BF16, DEV)
    lbuf, lse = _flat_nan(M, heads)
    K.attn_fwd_packed(c["qkv"], c["ss"], out, N=N, heads=heads, max_len=max(c["lens"]), last_only=True, lse2=lse)
    torch.cuda.synchronize()
    KB.check_guards(obuf, M, W, what + " (last)")
    _tail_untouched(lbuf, M, heads, what + " (last)")
    KB.assert_equal_bits(out, plain, what + " (last): out against the entry without lse2")
    other = torch.ones(M, dtype=torch.bool, device=DEV)
    other[last] = False
    assert bool(torch.isnan(lse[other]).all()), what + " (last): lse2 written at a row that is no sequence's last one"
    err = float((lse[last].double() - c["ref_lse"][last]).abs().max())
    print(f"{what} (last): worst |lse2 - float64| {err:.3e}")
    assert err < KB.LSE2_TOL, err


# ------------------------------------------------------------------------------------------------ 2. attn_bwd_packed
def _run_bwd(K, c, heads, ss=None, max_len=None, last_only=False, O=None, lse=None, dO=None, N=None):
    M, W = c["M"], c["W"]
    buf, dqkv = KB.guarded(M, 3 * W, BF16, DEV)
    dbuf, delta = _flat_nan(M, heads)
    K.attn_bwd_packed(c["qkv"], c["ss"] if ss is None else ss, c["dO"] if dO is None else dO, c["out"] if O is None else O,
                      c["lse"] if lse is None else lse, delta, dqkv, N=c["N"] if N is None else N, heads=heads,
                      max_len=max(c["lens"]) if max_len is None else max_len, last_only=last_only)
    torch.cuda.synchronize()
    KB.check_guards(buf, M, 3 * W, "packed attention backward dqkv")
    _tail_untouched(dbuf, M, heads, "packed attention backward delta")
    return dqkv, delta


@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_attn_bwd_packed(K, name, heads):
    c = _case(K, name, heads)
    M, W = c["M"], c["W"]
    what = f"packed attention backward [{name}, {heads} heads]"
    ref, covered = _bwd_ref(c["qkv"], c["dO"], c["out"], c["lse"], _seqs(c["lens"]), heads)
    assert bool(covered.all())
    dqkv, delta = _run_bwd(K, c, heads)
    assert not bool(torch.isnan(dqkv).any()), what + ": a NaN of the fill survived in a valid sequence's rows"
    rows = torch.arange(M, device=DEV)
    one = max(c["lens"]) == 1
    w = _check_thirds(dqkv, ref, rows, heads, what, one_token=one)
    if one:
        bq, bk = _one_token_bound(c, heads)
        KB.assert_within(dqkv[:, :W].double(), torch.zeros_like(bq), bq, what + " dq (one token: absolute)")
        KB.assert_within(dqkv[:, W:2 * W].double(), torch.zeros_like(bk), bk, what + " dk (one token: absolute)")
    print(f"{what}: worst per-(row, head) relative error dq {w['dq']:.3e} dk {w['dk']:.3e} dv {w['dv']:.3e} "
          f"(gates {KB.ATTN_ROW_TOL['dq']}, {KB.ATTN_ROW_TOL['dk']}, {KB.ATTN_ROW_TOL['dv']})")
    dref = (c["dO"].double() * c["out"].double()).view(M, heads, 64)
    KB.assert_within(delta.double(), dref.sum(-1), KB.sum_bound(dref.abs().sum(-1), 64), what + " delta")
    again, delta2 = _run_bwd(K, c, heads)
    KB.assert_equal_bits(again, dqkv, what + ": second run")
    KB.assert_equal_bits(delta2, delta, what + ": delta, second run")
    if max(c["lens"]) < 77:  # more tile classes launched, nothing changed
        more, _ = _run_bwd(K, c, heads, max_len=77)
        KB.assert_equal_bits(more, dqkv, what + ": max_len 77")


MALFORMED = {  # descriptors over M = 137 rows (lengths 20, 5, 33, 70, 9 when well formed)
    "length_0": [0, 20, 20, 58, 128, 137],
    "length_81": [0, 20, 101, 110, 128, 137],
    "start_beyond_M": [0, 20, 25, 58, 140, 137],
}


@pytest.mark.parametrize("last_only", [False, True], ids=["full", "last"])
@pytest.mark.parametrize("bad", list(MALFORMED))
def test_attn_bwd_packed_skips_a_malformed_sequence(K, bad, last_only):
    heads, M = 3, 137
    W = heads * 64
    st = MALFORMED[bad]
    seqs = [(a, b - a) for a, b in zip(st, st[1:]) if 0 <= a and b <= M and 1 <= b - a <= 80]
    assert len(seqs) in (3, 4) and len(seqs) < len(st) - 1
    g = torch.Generator(device=DEV).manual_seed(31 + len(bad))
    qkv = torch.randn(M, 3 * W, generator=g, device=DEV).bfloat16()
    dO = torch.randn(M, W, generator=g, device=DEV).bfloat16()
    ss = torch.tensor(st, dtype=torch.int32, device=DEV)
    _, out = KB.guarded(M, W, BF16, DEV)
    _, lse = _flat_nan(M, heads)
    K.attn_fwd_packed(qkv, ss, out, N=5, heads=heads, max_len=80, lse2=lse, last_only=last_only)
    c = dict(M=M, W=W, N=5, qkv=qkv, dO=dO, ss=ss, out=out, lse=lse, lens=[80])
    dqkv, delta = _run_bwd(K, c, heads, last_only=last_only)
    ref, covered = _bwd_ref(qkv, dO, out, lse, seqs, heads, last_only=last_only)
    what = f"packed attention backward, {bad}, last_only={last_only}"
    assert bool(torch.isnan(dqkv[~covered]).all()) and bool(torch.isnan(delta[~covered]).all()), what + ": the skipped rows were written"
    assert bool(torch.isnan(out[~covered]).all()) and bool(torch.isnan(lse[~covered]).all()), what + ": the forward wrote skipped rows"
    assert not bool(torch.isnan(dqkv[covered]).any())
    rows = torch.nonzero(covered).reshape(-1)
    lastr = torch.tensor([s + n - 1 for s, n in seqs], device=DEV)
    _check_thirds(dqkv, ref, rows, heads, what, dq_rows=lastr if last_only else None)


# ------------------------------------------------------------------------------------------------ 3. the one-query form
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_attn_bwd_packed_last(K, name, heads):
    c = _case(K, name, heads)
    N, M, W = c["N"], c["M"], c["W"]
    what = f"packed last-row attention backward [{name}, {heads} heads]"
    last = (c["ss"][1:] - 1).long()
    other = torch.ones(M, dtype=torch.bool, device=DEV)
    other[last] = False
    # what the last block holds in training: out, lse2 and dO exist at the last rows only (NaN elsewhere)
    _, out = KB.guarded(M, W, BF16, DEV)
    _, lse = _flat_nan(M, heads)
    K.attn_fwd_packed(c["qkv"], c["ss"], out, N=N, heads=heads, max_len=max(c["lens"]), last_only=True, lse2=lse)
    dO = torch.full((M, W), float("nan"), dtype=BF16, device=DEV)
    dO[last] = c["dO"][last]
    ref, covered = _bwd_ref(c["qkv"], dO, out, lse, _seqs(c["lens"]), heads, last_only=True)
    dqkv, delta = _run_bwd(K, c, heads, last_only=True, O=out, lse=lse, dO=dO)
    assert not bool(torch.isnan(dqkv).any()), what + ": a NaN of the fill survived in a valid sequence's rows"
    assert bool(torch.isnan(delta[other]).all()) and bool(torch.isfinite(delta[last]).all())
    assert float(dqkv[other][:, :W].float().abs().max() if bool(other.any()) else 0.0) == 0.0, what + ": dQ of a row that is no query"
    one = max(c["lens"]) == 1
    w = _check_thirds(dqkv, ref, torch.arange(M, device=DEV), heads, what, dq_rows=last, one_token=one)
    if one:
        cc = dict(c, dO=c["dO"])
        bq, bk = _one_token_bound(cc, heads)
        KB.assert_within(dqkv[:, :W].double(), torch.zeros_like(bq), bq, what + " dq (one token: absolute)")
        KB.assert_within(dqkv[:, W:2 * W].double(), torch.zeros_like(bk), bk, what + " dk (one token: absolute)")
    print(f"{what}: worst per-(row, head) relative error dq {w['dq']:.3e} dk {w['dk']:.3e} dv {w['dv']:.3e}")
    again, _ = _run_bwd(K, c, heads, last_only=True, O=out, lse=lse, dO=dO)
    KB.assert_equal_bits(again, dqkv, what + ": second run")


# ------------------------------------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize("last_only", [False, True], ids=["full", "last"])
def test_attn_bwd_packed_refusals(K, last_only):
    c = _case(K, "edges_sorted", 3)
    M, W, heads = c["M"], c["W"], 3

    def call(max_len=77, lse=c["lse"], ld_extra=8):
        buf = torch.full((M, 3 * W + ld_extra), float("nan"), dtype=BF16, device=DEV)
        _, delta = _flat_nan(M, heads)
        with pytest.raises(K.HipError, match="-22"):
            K.attn_bwd_packed(c["qkv"], c["ss"], c["dO"], c["out"], lse, delta, buf[:, :3 * W], N=c["N"], heads=heads, max_len=max_len,
                              last_only=last_only)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()) and bool(torch.isnan(delta).all()), "a refused call launched a kernel"
    call(max_len=81)
    call(lse=None)
    call(ld_extra=4)  # lddq = 3W + 4: no multiple of 8


# ------------------------------------------------------------------------------------------------ 5. the embedding backward
@pytest.mark.parametrize("name", ["edges_shuffled", "all_equal_24", "any_300_prime_M", "one_of_1"])
@pytest.mark.parametrize("Wt", [128, 512])
def test_text_embed_bwd_packed(K, name, Wt):
    """demb / dpos per element against float64 sums under sum_bound, from zeroed accumulators (so that the rows of unused ids and of
    the positions behind the longest caption are exactly zero), twice.  The vocabulary is small (11 body ids): with 50 captions and
    more some ids make runs of more than 64 rows (the long-run kernel), the others stay with the short one."""
    lens = LENGTH_SETS[name]
    N, M, V, ctx = len(lens), sum(lens), 40, 77
    g = torch.Generator().manual_seed(M + Wt)
    ids = torch.zeros(N, ctx, dtype=torch.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = torch.randint(1, 12, (n,), generator=g)
        ids[r, 0] = V - 2
        ids[r, n - 1] = V - 1
    pk = K.pack_captions(ids, ctx)
    assert pk["ids"].numel() == M
    if N >= 50:
        seg = pk["tok_seg"].long()
        assert int((seg[1:] - seg[:-1]).max()) > 64
    dx = torch.randn(M, Wt, generator=g)
    d, flat = dx.double(), pk["ids"].long()
    pos = torch.cat([torch.arange(n) for n in lens])
    re, se, ce = (torch.zeros(V, Wt, dtype=torch.float64) for _ in range(3))
    re.index_add_(0, flat, d); se.index_add_(0, flat, d.abs()); ce.index_add_(0, flat, torch.ones_like(d))
    rp, sp, cp = (torch.zeros(ctx, Wt, dtype=torch.float64) for _ in range(3))
    rp.index_add_(0, pos, d); sp.index_add_(0, pos, d.abs()); cp.index_add_(0, pos, torch.ones_like(d))
    dev = {k: v.to(DEV) for k, v in pk.items() if torch.is_tensor(v)}
    dxw = torch.full((M, Wt + 4), float("nan"), device=DEV)  # a row-major view with a wider leading dimension
    dxw[:, :Wt] = dx.to(DEV)
    what = f"text_embed_bwd_packed [{name}, Wt {Wt}]"
    runs = []
    for _ in range(2):
        be = torch.zeros(V + 3, Wt, device=DEV)
        bp = torch.zeros(ctx + 3, Wt, device=DEV)
        K.text_embed_bwd_packed(dxw[:, :Wt], dev["ids"], dev["seq_start"], be[:V], bp[:ctx], N=N,
                                tok_sort=(dev["tok_order"], dev["tok_seg"]), pos_sort=(dev["pos_order"], dev["pos_seg"]))
        torch.cuda.synchronize()
        assert float(be[V:].abs().max()) == 0.0 and float(bp[ctx:].abs().max()) == 0.0, what + ": rows behind the tables written"
        demb, dpos = be[:V].cpu(), bp[:ctx].cpu()
        w1 = KB.assert_within(demb, re, KB.sum_bound(se, ce), what + " demb")
        w2 = KB.assert_within(dpos, rp, KB.sum_bound(sp, cp), what + " dpos")
        unused = torch.ones(V, dtype=torch.bool)
        unused[flat] = False
        assert bool(unused.any()) and float(demb[unused].abs().max()) == 0.0, what + ": an unused id's row is not zero"
        if max(lens) < ctx:
            assert float(dpos[max(lens):].abs().max()) == 0.0, what + ": a position behind the longest caption is not zero"
        runs.append((demb, dpos))
    print(f"{what}: worst |err| / bound demb {w1:.3g} dpos {w2:.3g}")
    KB.assert_equal_bits(runs[1][0], runs[0][0], what + " demb, second run")
    KB.assert_equal_bits(runs[1][1], runs[0][1], what + " dpos, second run")


def test_text_embed_bwd_packed_ignores_ids_outside_the_vocabulary(K):
    """an id outside [0, vocab) adds nothing, to its own (non-existent) row or to any other; the positions still count the row"""
    lens, V, Wt, ctx = [5, 3, 9], 12, 128, 16
    ids = torch.zeros(3, ctx, dtype=torch.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = torch.arange(1, n + 1)
        ids[r, n - 1] = 11
    pk = K.pack_captions(ids, ctx)
    bad = pk["ids"].clone()
    bad[1], bad[6] = 12, -3
    order, seg = K.token_sort(bad)
    M = bad.numel()
    dx = torch.randn(M, Wt, generator=torch.Generator().manual_seed(5))
    be, bp = torch.zeros(V + 3, Wt, device=DEV), torch.zeros(ctx, Wt, device=DEV)
    K.text_embed_bwd_packed(dx.to(DEV), bad.to(DEV), pk["seq_start"].to(DEV), be[:V], bp, N=3, tok_sort=(order.to(DEV), seg.to(DEV)),
                            pos_sort=(pk["pos_order"].to(DEV), pk["pos_seg"].to(DEV)))
    torch.cuda.synchronize()
    ok = (bad >= 0) & (bad < V)
    re = torch.zeros(V, Wt, dtype=torch.float64).index_add_(0, bad[ok].long(), dx[ok].double())
    assert float(be[V:].abs().max()) == 0.0
    assert float((be[:V].cpu().double() - re).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ 6 - 9. the engine
def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def min_cos(a, b):
    a, b = a.detach().double().cpu().reshape(a.shape[0], -1), b.detach().double().cpu().reshape(b.shape[0], -1)
    return float(torch.nn.functional.cosine_similarity(a, b, dim=1).min())


def build(arch, seed, **flags):
    """(model, oracle arch, oracle parameters); flags: engine switches the oracle does not know (text_packed, ...)"""
    from tvts_amd.model._common import TVTSv2Base
    oarch = O.tiny_arch(**arch)
    P = O.synth_params(oarch, seed=seed)
    m = TVTSv2Base(ARGS, arch=dict(arch, **flags))
    m.load_state_dict(P, strict=True)
    return m, oarch, P


def oracle_step(P, batch, oarch):
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    l1, l2, te, ve, pred = O.step_losses(leaves, batch, oarch)
    (l1 + l2).backward()
    grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    return float(l1.detach()), float(l2.detach()), te.detach(), ve.detach(), None if pred is None else pred.detach(), grads


def engine_step(m, batch):
    from tvts_amd.engine import LossHead
    m._fresh_shadows(); m._sync_requires_grad()
    eng = m.engine
    pb = eng.prepare_batch(batch)
    m.store.grad.zero_()
    te, ve, pred = eng.forward(pb)
    head = LossHead(m.store.device)
    loss1, dv, dt = head.contrastive(ve, te)
    loss2, dpred = (head.sorting(pred, batch["label"].reshape(-1).to(torch.int32).to(DEV)) if pred is not None else (None, None))
    eng.backward(dt, dv, dpred)
    torch.cuda.synchronize()
    return float(loss1), (float(loss2) if loss2 is not None else 0.0), te.clone(), ve.clone(), pred, m.store, pb


def check_grads(store, grads, gn_tol=0.01, cos_tol=0.995):
    """the gates of tests/test_model_gpu.py::check_grads: total gradient norm within 1 %, every tensor that carries more than 1e-3 of
    it at cosine > 0.995"""
    tot_ref = sum(float(g.norm()) ** 2 for g in grads.values()) ** 0.5
    tot, worst = 0.0, []
    for k, g in grads.items():
        mine = store.g(k).detach().cpu()
        assert torch.isfinite(mine).all(), k
        tot += float(mine.norm()) ** 2
        if float(g.norm()) > 1e-3 * tot_ref:
            c = float(torch.nn.functional.cosine_similarity(mine.double().flatten(), g.double().flatten(), dim=0))
            worst.append((c, k, float(mine.norm()), float(g.norm())))
    tot = tot ** 0.5
    worst.sort()
    assert abs(tot - tot_ref) < gn_tol * tot_ref, (tot, tot_ref, worst[:5])
    assert worst[0][0] > cos_tol, worst[:8]


def ragged_batch(oarch, B, T, seed, forced, lo=3, n_trans=None):
    """captions of different lengths in [lo, context], `forced` among them, zero-padded behind their end token"""
    ctx = oarch["context"]
    batch = O.synth_batch(oarch, B=B, T=T, seed=seed, caption_len=ctx, n_trans=n_trans)
    N = batch["text"].shape[0]
    lens = torch.randint(lo, ctx + 1, (N,), generator=torch.Generator().manual_seed(seed + 1))
    lens[:len(forced)] = torch.tensor(forced)
    lens = lens[torch.randperm(N, generator=torch.Generator().manual_seed(seed + 2))]
    for r, n in enumerate(lens.tolist()):
        batch["text"][r, n - 1] = oarch["vocab"] - 1
        batch["text"][r, n:] = 0
    assert (batch["text"].argmax(-1) == lens - 1).all()
    return batch, lens.tolist()


FORCED = [77, 3, 16, 17, 48, 49]  # every tile class and both of its edges
_ORACLE = {}


def _oracle(kind):
    """the oracle's PADDED step on the ragged batch (it needs no packed mode), once per architecture"""
    if kind not in _ORACLE:
        from tvts_amd import arch as A
        arch = (A.small_arch if kind == "small" else A.small_arch_h)(context=77)
        oarch = O.tiny_arch(**arch)
        P = O.synth_params(oarch, seed=13)
        batch, lens = ragged_batch(oarch, B=6, T=3, seed=15, forced=FORCED)
        _ORACLE[kind] = (arch, oarch, P, batch, lens, oracle_step(P, batch, oarch))
    return _ORACLE[kind]


@pytest.mark.parametrize("kind,used_rows", [("small", True), ("small", False), ("small_h", True)])
def test_packed_engine_against_the_oracle(K, kind, used_rows):
    arch, oarch, P, batch, lens, (r1, r2, rte, rve, rpred, grads) = _oracle(kind)
    assert arch["text_width"] // arch["text_heads"] == 64  # (small_arch_h keeps the B text side: head dim 64, so it runs packed)
    m, _, _ = build(arch, 13, text_packed=True, text_used_rows_only=used_rows)
    assert m.engine.text_packed and m.engine.text_used_rows_only == used_rows
    l1, l2, te, ve, pred, store, pb = engine_step(m, batch)
    assert pb["M"] == sum(lens) and pb["max_len"] == 77 and pb["ids"].numel() == pb["M"] < len(lens) * 77
    print(f"packed engine [{kind}, used rows {used_rows}]: M {pb['M']} of {len(lens) * 77} padded rows; text cos {min_cos(te, rte):.6f} "
          f"rel {rel(te, rte):.3e}; losses {l1:.4f} / {r1:.4f}, {l2:.4f} / {r2:.4f}")
    assert min_cos(te, rte) > 0.9995 and rel(te, rte) < 0.02, (min_cos(te, rte), rel(te, rte))
    assert min_cos(ve, rve) > 0.9995 and rel(ve, rve) < 0.02
    assert abs(l1 - r1) < 1e-2 and abs(l2 - r2) < 1e-2, (l1, r1, l2, r2)
    check_grads(store, grads)
    demb, rdemb = store.g("text_token_embedding.weight").cpu(), grads["text_token_embedding.weight"]
    assert float(rdemb[0].abs().max()) == 0.0 and float(demb[0].abs().max()) == 0.0  # the padding token learns nothing
    # (the longest caption fills the context; the all-equal batch below holds dpos behind the longest caption at zero)


def test_packed_against_padded_engine(K):
    """the same batch through the same weights with text_packed on and off: the attention kernels differ, so no bit equality --
    losses within 1e-2, every gradient tensor at check_grads' gates against the PADDED engine's gradients; two packed steps agree
    bit for bit in every gradient tensor"""
    arch, oarch, P, batch, lens, (r1, r2, *_rest, grads) = _oracle("small")
    mp, _, _ = build(arch, 13)
    p1, p2, pte, pve, _, pstore, ppb = engine_step(mp, batch)
    assert "M" not in ppb and not mp.engine.text_packed
    pgrads = {k: pstore.g(k).detach().cpu().clone() for k in grads}
    m, _, _ = build(arch, 13, text_packed=True)
    l1, l2, te, ve, _, store, _ = engine_step(m, batch)
    assert abs(l1 - p1) < 1e-2 and abs(l2 - p2) < 1e-2, (l1, p1, l2, p2)
    assert min_cos(te, pte) > 0.9995 and rel(te, pte) < 0.02
    check_grads(store, pgrads)
    first = store.grad.detach().clone()
    engine_step(m, batch)
    KB.assert_equal_bits(store.grad.detach(), first, "packed step: the flat gradient buffer of a second step")


@pytest.mark.parametrize("equal", [False, True], ids=["ragged", "all_equal"])
def test_packed_webvid_batch(K, equal):
    """NT = 1 (no sort head: pred None, pred_model without gradient); and a batch whose captions all have one length -- packed
    with no row saved, and dpos behind the longest caption exactly zero"""
    from tvts_amd import arch as A
    arch = A.small_arch(context=77)
    m, oarch, P = build(arch, 4, text_packed=True)
    if equal:
        batch = O.synth_batch(oarch, B=4, T=3, seed=6, n_trans=1, caption_len=19)
    else:
        batch, _ = ragged_batch(oarch, B=4, T=3, seed=6, forced=[33, 5], n_trans=1)
    r1, r2, rte, rve, rpred, grads = oracle_step(P, batch, oarch)
    l1, l2, te, ve, pred, store, pb = engine_step(m, batch)
    assert pred is None and rpred is None and pb["NT"] == 1
    if equal:
        assert pb["M"] == 4 * 19 == pb["N"] * pb["L"]
        assert float(store.g("text_positional_embedding")[19:].abs().max()) == 0.0
    assert min_cos(te, rte) > 0.9995 and rel(te, rte) < 0.02
    assert min_cos(ve, rve) > 0.9995 and abs(l1 - r1) < 1e-2
    check_grads(store, grads)
    assert float(store.g("pred_model.head.weight").abs().max()) == 0.0


def test_packed_refusals(K):
    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base
    with pytest.raises(NotImplementedError, match="head dim 64"):
        TVTSv2Base(ARGS, arch=A.small_arch(context=77, text_packed=True, text_width=160, text_heads=2))
    with pytest.raises(ValueError, match="v1"):
        from tvts_amd.engine_v1 import EngineV1, ParamStore
        EngineV1(ParamStore(A.small_arch_v1(text_packed=True), torch.device(DEV)))
    m, oarch, _ = build(A.small_arch(context=16), 2, text_packed=True)
    long = O.synth_batch(oarch, B=2, T=2, seed=3, caption_len=16)
    long["text"] = torch.cat([long["text"], torch.zeros_like(long["text"][:, :1])], 1)  # 17 columns for a context of 16
    with pytest.raises(IndexError):
        m.engine.prepare_batch(long)


def test_packed_env_switch(K, monkeypatch):
    """TVTS_TEXT_PACKED switches the option on where no arch dict carries the key (the reference entrypoint builds none); the key wins"""
    from tvts_amd import arch as A
    monkeypatch.setenv("TVTS_TEXT_PACKED", "1")
    assert build(A.small_arch(context=77), 2)[0].engine.text_packed
    assert not build(A.small_arch(context=77), 2, text_packed=False)[0].engine.text_packed
    monkeypatch.setenv("TVTS_TEXT_PACKED", "0")
    assert not build(A.small_arch(context=77), 2)[0].engine.text_packed
    monkeypatch.delenv("TVTS_TEXT_PACKED")
    assert not build(A.small_arch(context=77), 2)[0].engine.text_packed


def test_packed_optimizer_steps_track_the_oracle(K, monkeypatch):
    """5 optimizer steps of the product path (StepRunner, fused HF-AdamW) on a fixed ragged batch with text_packed on, through the
    TVTS_TRAINER_GRAPH=1 runner: the losses track the oracle's within the tolerance of test_training_curve_tracks_oracle
    (2 % + 1e-2), and the runner captures nothing -- packed batches run eagerly by rule."""
    from tvts_amd import arch as A
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import GraphReplay, StepRunner
    a = A.small_arch(context=77)
    m, oarch, P = build(a, 7, text_packed=True)
    batch, _ = ragged_batch(oarch, B=4, T=2, seed=8, forced=[77, 3, 20, 40])
    hp = [(lr * 3, wd) for lr, wd in A.GROUP_HPARAMS]
    groups = [[], [], [], []]
    for name, p in m.named_parameters():
        gi = A.param_group_of(name, a)
        if gi < 0:
            p.requires_grad = False
        else:
            groups[gi].append(p)
    opt = FusedHFAdamW([dict(params=groups[i], lr=hp[i][0], weight_decay=hp[i][1]) for i in range(4)], m.store, model=m)
    monkeypatch.setenv("TVTS_TRAINER_GRAPH", "1")
    replay = GraphReplay(StepRunner(m, opt))
    assert replay.usable
    Pr = {k: v.clone() for k, v in P.items()}
    state, O_HP = {}, O.GROUP_HPARAMS
    O.GROUP_HPARAMS = tuple(hp)
    try:
        ref_curve, curve = [], []
        for _ in range(5):
            r1, r2, _ = O.train_step(Pr, batch, oarch, state)
            ref_curve.append(r1 + r2)
            out = replay.step(batch)
            curve.append(float(out["loss1"]) + float(out["loss2"]))
    finally:
        O.GROUP_HPARAMS = O_HP
    ref_curve, curve = np.array(ref_curve), np.array(curve)
    print("packed training curve", curve, "oracle", ref_curve)
    assert np.all(np.abs(curve - ref_curve) < 0.02 * np.abs(ref_curve) + 1e-2), (curve, ref_curve)
    assert replay.captures == 0 and replay.replays == 0 and replay.eager == 5 and replay.usable
