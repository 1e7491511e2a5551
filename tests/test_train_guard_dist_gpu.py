"""Gradient clipping and the overflow guard of the pretraining step across data-parallel ranks (run with -m gpu):
tools/dist_train_guard_smoke.py as a child process, two ranks on the one GPU of the test box over gloo, in the way
tests/test_v1_guard_dist_gpu.py runs its tool.  The tool holds the checks (fresh processes it starts and ends itself); the timeout is
only the backstop against a hang."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_ranks_nan_skips_the_step_on_both():
    """the NaN pixel is in rank 1's shard only, on step 2 of 3: both ranks report skipped == 1, equal parameter checksums after
    every step, the same grad_norm and a finite state at the end; a rank with skip_nonfinite=True beside one without raises on both"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "dist_train_guard_smoke.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "DIST_TRAIN_GUARD_OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    said = [l for l in lines if "guard: skipped 1, replicas equal after every step, same grad_norm on both ranks, finite state at the end" in l]
    assert len(said) == 2 and {l.split("]")[0] for l in said} == {"[rank 0", "[rank 1"}, said
    raised = [l for l in lines if "GUARD_MISMATCH_RAISED" in l]
    assert len(raised) == 2 and {l.split("]")[0] for l in raised} == {"[rank 0", "[rank 1"}, raised
    # grad_norm is the same number on both ranks, step by step (finite, not finite, finite)
    per_rank = {rk: [l.split("grad_norm ")[1].split(",")[0] for l in lines if l.startswith(f"[rank {rk}] step ")] for rk in (0, 1)}
    assert per_rank[0] == per_rank[1] and len(per_rank[0]) == 3, per_rank
    assert per_rank[0][1] in ("nan", "inf", "-inf") and all(x not in ("nan", "inf", "-inf") for x in (per_rank[0][0], per_rank[0][2])), per_rank
