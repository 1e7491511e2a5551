"""The v1 fine-tuning step and its evaluation across data-parallel ranks (run with -m gpu): two ranks share the one GPU of the
test box over gloo moving device tensors, as tests/test_dist_gpu.py does for the pretraining step -- the collectives' semantics are
the backend-independent part.  Every test starts tools/dist_finetune_smoke.py as a child process with the checks it names; the
tool holds the checks themselves (tests/v1_downstream_synth.TINY, 4-frame clips, 5 classes, 2 clips per rank), with the gates of
tests/kernel_bounds.py and check_grads of tests/test_v1_gpu.py.  A rank that fails ends the child at once (the tool terminates the
other rank instead of waiting for it); the timeout is only the backstop against a hang."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_checks(*checks):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "dist_finetune_smoke.py"), *checks]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "DIST_FINETUNE_OK " + " ".join(checks) in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_identical_shards_reproduce_the_single_process_step_bit_for_bit():
    """fp32 payload, both ranks on the same 2 clips, targets and mask table, 2 updating steps: store.flat, exp_avg, exp_avg_sq, the
    bf16 shadows, grad_norm and loss as bits against FinetuneStep(data_parallel=False); clip_grad off, on, and update_freq 2"""
    out = run_checks("identical")
    for name in ("clip off", "clip on", "update_freq 2"):
        assert out.count(f"identical shards, {name}: bit-equal") == 2, name


def test_distinct_shards_equal_the_concatenated_batch():
    """2 + 2 clips: the exchanged gradient times 1 / W under check_grads against the backward over the 4 clips; grad_norm within 1 %
    of the float64 norm of the full-batch gradient; the mean of the ranks' losses against the full-batch loss"""
    run_checks("distinct")


def test_replicas_stay_identical():
    """3 steps, distinct shards, per-rank masks (rate 0.1) and Mixup plans: replicas_checksum() and the checksums of the moments
    agree across the ranks while their mask tables differ"""
    run_checks("replicas")


def test_what_travels():
    """no collective and bytes_sent == 0 on a call that only accumulates; on an updating call the ranges are disjoint, in backward
    order and cover exactly the trainable chunks, bytes_sent = 4 (fp32) / 2 (bf16) bytes per element; trainable="head" sends the
    head alone and leaves every bit of the tower"""
    out = run_checks("travel")
    for what in ("fp32 all", "bf16 all", "fp32 head"):
        assert out.count(f"travel {what}:") == 2, what


def test_bf16_payload_stays_within_the_first_step_bound():
    """identical shards, no clipping, first step: every parameter within lr * lr_scale * 2^-9 (+ the fp32 rounding of the two
    updates) of the fp32-payload run; the derivation is the tool's check_bf16"""
    out = run_checks("bf16")
    ratios = [float(l.split()[5]) for l in out.splitlines() if l.startswith("BOUND finetune bf16 payload")]
    assert len(ratios) == 2 and all(0.0 < r <= 1.0 for r in ratios), ratios


def test_start_up_broadcast_mismatch_and_seeds():
    """ranks built from different init seeds hold rank 0's parameters after construction; trainable="head" beside "all" raises on
    BOTH ranks with the agreement's message and hangs neither (the checks behind it still run in the same processes); the
    per-rank mask offset holds for a model built before the process group as for one built after, and a resumed pair
    (set_drop_seed_base) continues each rank's own sequence"""
    out = run_checks("start", "mismatch", "seeds")
    raised = [l for l in out.splitlines() if "MISMATCH_RAISED:" in l]
    assert len(raised) == 2 and {l.split("]")[0] for l in raised} == {"[rank 0", "[rank 1"}, raised
    for l in raised:
        assert "the optimizer's chunk / group table differs between the ranks" in l and "checksums by rank" in l, l


def test_validation_merges_the_meters_over_the_ranks():
    """four fixed batches (one of them short) as two per rank: acc1 / acc5 / loss within 1e-12 relative of one process over the
    four; the sample-weighted top-1 (100 / 7) is told from the batch-weighted one (25)"""
    run_checks("validation")


def test_view_merge_over_the_ranks_keeps_rank_zero_lines():
    """b0, b2 on rank 0 and b1, b3 plus duplicates of two b0 lines (other logits) on rank 1: gather().result(), the view logits and
    the summed logits behind it are the single-process merger's bits"""
    run_checks("merge")
