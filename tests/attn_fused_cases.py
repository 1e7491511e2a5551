"""The geometries, inputs, references and gates that tests/test_attention_fused_rows_gpu.py (the kernels) and
tests/test_kernel_bounds_cpu.py (the references and the gates themselves, with no kernel) share -- a plain helper module.

The fused divided site kernels of tvts_amd/csrc/attention.hip pick a template instantiation by the size of a group:
SPACE  one block per (clip, head, frame), MT = ceil((n + 1) / 16) row tiles, n + 1 <= 112;
TIME   one block per (clip, head, chunk of 28 patch positions), a wave per group; T + 1 <= 16 -> <1>, 17 .. 20 -> <2, 20>,
       21 .. 32 -> <2>.
`instantiation` and `parts_of` RESTATE that dispatch (bwd_impl / fwd_divided_impl, TIME_CHUNK): Python cannot see which template ran,
so `instantiation` is a label of the BOUND lines and of the profile table, no more.  `parts_of` is checked: the GPU tests size cls_ws and
cls_acc by it exactly and assert that every element was written, which a dispatch with another chunk size or partial count fails.
Inputs are drawn on the host, so the values are the same on every machine and in the kernel-free checks."""
import torch

import kernel_bounds as KB

B, HEADS = 2, 3  # an odd head count: a wrong head-column stride cannot land on another head's slice of the same row
TOL = KB.ATTN_ROW_TOL
TIME_CHUNK = 28

# SPACE: both edges of every MT = 1 .. 7 (the last tile full at n + 1 = 16 MT, one live row in it at n + 1 = 16 (MT - 1) + 1);
# T = 1: a single CLS partial
SPACE_N = (1, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111)
SPACE_CASES = [("space", 3, n) for n in SPACE_N] + [("space", 1, n) for n in (1, 16, 111)]
# TIME: every tile class (T + 1 = 2, 3, 16 | 17, 20 | 21, 32) x one chunk with idle waves (n = 1, 3), exactly four groups (4), a
# second round of wave 0 (5), a chunk one short of full (27), full (28), a one-position last chunk (29), three chunks (57).
# Two wishes for this sweep collide: every n with T in {1, 19, 31}, and S = 1 + T n <= 1000 for the largest case.  The size limit
# is kept, so (T 19, n 57: S = 1084), (T 20, n 57: 1141) and (T 31, n 57: 1768) are NOT run.  The consequence: three chunks -- three
# ordered CLS partials per (clip, head) -- are seen by time<1> (T = 1, 2, 15) and by time<2,20> at T = 16 only; time<2> (T = 20, 31)
# is never run with more than two (n = 29), since three chunks need n >= 57 and with T >= 20 that is S >= 1141.  The partial count is
# a property of the launch (blocks, cp[...] slot, merge / finalize loop), shared by the three instantiations, not of the tile class.
TIME_CASES = [("time", T, n) for T in (1, 2, 15, 16, 19, 20, 31) for n in (1, 3, 4, 5, 27, 28, 29, 57) if 1 + T * n <= 1000]
SWEEP_CASES = SPACE_CASES + TIME_CASES
STRESS_CASES = [("space", 3, 16), ("space", 3, 111), ("time", 19, 29), ("time", 31, 3)]
# the smallest geometries of the sweep: 2 .. 4 keys per query, where dP - delta cancels
TINY_CASES = [("space", 3, 1), ("space", 1, 1)] + [("time", 1, n) for n in (1, 3, 4, 5, 27, 28, 29, 57)] + [("time", 2, 3)]


def instantiation(mode, T, n):
    """the template instantiation of the four fused kernels a geometry takes"""
    if mode == "space":
        return f"space<{-(-(n + 1) // 16)}>"
    return "time<1>" if T + 1 <= 16 else "time<2,20>" if T + 1 <= 20 else "time<2>"


def parts_of(mode, T, n):
    """ordered CLS partials of a site: one per block of (clip, head)"""
    return T if mode == "space" else -(-n // TIME_CHUNK)


# With 2 .. 6 keys in the whole clip the CLS query's dP - delta cancels, and the bf16 rounding of the CLS output row (which its
# delta is taken from) shows through in dQ / dK for some draws: the first draw of these geometries leaves the reference itself up to
# 8e-2 from float64 autograd.  They take the first later draw at which it stays within half of ATTN_ROW_TOL
# (tests/test_kernel_bounds_cpu.py::test_fused_divided_reference_is_within_half_the_tolerance_of_autograd_at_the_tiny_geometries)
SEED_SHIFT = {("space", 3, 1, 64): 4, ("space", 1, 1, 64): 7, ("space", 1, 1, 80): 17, ("time", 1, 1, 64): 10, ("time", 1, 1, 80): 32,
              ("time", 1, 5, 64): 1, ("time", 1, 5, 80): 1}


def seed_of(mode, T, n, dh):
    return 7000 + 1000 * (mode == "time") + 31 * T + n + dh + 100000 * SEED_SHIFT.get((mode, T, n, dh), 0)


def plain_inputs(mode, T, n, dh, seed=None):
    """bf16 qkv [B * S, 3W] and dO [B * S, W] (CPU), N(0, 1)"""
    S, W = 1 + T * n, HEADS * dh
    g = torch.Generator().manual_seed(seed_of(mode, T, n, dh) if seed is None else seed)
    return torch.randn(B * S, 3 * W, generator=g).bfloat16(), torch.randn(B * S, W, generator=g).bfloat16()


def stress_row(mode, T, n, b):
    """the token row (inside its clip) of the one key that takes the direction of the CLS query in head 0: a key of the LAST
    group's last position (clip 0) / of group 1 or 0 (clip 1), so that the dominating partial is not always the first one merged"""
    S = 1 + T * n
    return S - 1 if b == 0 else (1 + min(1, n - 1) if mode == "time" else 1 + min(1, T - 1) * n)


def stress_inputs(mode, T, n, dh):
    """the second input family.  Head 0: q scaled by 8 (score spread ~ 11 in the log2 domain: patch rows with one-key softmaxes)
    and one key per clip = sqrt(dh) * the unit vector of the clip's CLS query, whose score (~ 1.44 |q_cls| ~ 90) leaves every
    other key of the CLS row more than 2^24 behind in linear scale, so one group's CLS partial dominates the merge.  Head 1:
    q = k = 0, a uniform softmax with lse2 = log2(keys) exactly.  Head 2: N(0, 1)."""
    S, W = 1 + T * n, HEADS * dh
    qkv, dO = plain_inputs(mode, T, n, dh, seed=seed_of(mode, T, n, dh) + 50000)
    x = qkv.float().view(B, S, 3 * W)
    x[:, :, 0:dh] *= 8.0
    for b in range(B):
        qc = x[b, 0, 0:dh]
        x[b, stress_row(mode, T, n, b), W:W + dh] = qc / qc.norm() * dh ** 0.5
    x[:, :, dh:2 * dh] = 0.0
    x[:, :, W + dh:W + 2 * dh] = 0.0
    return x.view(B * S, 3 * W).bfloat16(), dO


def forward_ref(qkv, mode, T, n, dh):
    """float64 (out [B * S, W], lse2 [B * S, heads]) of qkv [B * S, 3W] on its device"""
    S, W = 1 + T * n, HEADS * dh
    ro, rl, _ = KB.divided_fwd_ref(qkv.view(B, S, 3 * W), HEADS, dh, mode, T, n)
    return ro.reshape(B * S, W), rl.reshape(B * S, HEADS)


def backward_ref(qkv, dO, ro, out_kernel, lse_kernel, mode, T, n, dh):
    """float64 dqkv [B * S, 3W] from what the fused backward read: qkv, dO, the log-sum-exp the forward stored and the mixed output"""
    S, W = 1 + T * n, HEADS * dh
    o_read = KB.divided_mixed_o_read(ro.view(B, S, W), out_kernel.reshape(B, S, W))
    rd = KB.attn_bwd_same_inputs(qkv.view(B, S, 3 * W), dO.view(B, S, W), o_read, lse_kernel.reshape(B, S, HEADS), HEADS, dh,
                                 allowed=KB.divided_allowed(mode, T, n))
    return rd.reshape(B * S, 3 * W)


def gate_forward(tag, out, lse, ro, rl, S, worst=None):
    """the forward gates: every (row, head) slice of out at ATTN_ROW_TOL["out"] (the CLS rows also as their own group), every lse2
    value absolutely at LSE2_TOL.  Prints the BOUND lines -> {quantity: worst}"""
    worst = {} if worst is None else worst
    w, wc = KB.rows_check(out, ro, TOL["out"], HEADS, B, S, tag + " out")
    worst["out"] = KB.bound_line(tag + " out (per-row rel)", w)
    worst["out CLS"] = KB.bound_line(tag + " out CLS (per-row rel)", wc)
    worst["lse2"] = KB.bound_line(tag + " lse2 (|err| / 1e-3)", KB.assert_within(lse, rl, KB.LSE2_TOL, tag + " lse2"))
    return worst


def gate_backward(tag, dqkv, rd, S, worst=None):
    """the backward gates: every (row, head) slice of dq, dk, dv at ATTN_ROW_TOL, the CLS rows also as their own group"""
    worst = {} if worst is None else worst
    W = rd.shape[1] // 3
    for i, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(i * W, (i + 1) * W)
        w, wc = KB.rows_check(dqkv[:, sl], rd[:, sl], TOL[nm], HEADS, B, S, f"{tag} {nm}")
        worst[nm] = KB.bound_line(f"{tag} {nm} (per-row rel)", w)
        worst[nm + " CLS"] = KB.bound_line(f"{tag} {nm} CLS (per-row rel)", wc)
    return worst
