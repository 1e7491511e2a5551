"""The micro-batched pretraining step across data-parallel ranks (run with -m gpu): tools/dist_micro_batch_smoke.py as a child
process, two ranks on the one GPU of the test box over gloo, B = 4 per rank, two chunks, in the way tests/test_train_guard_dist_gpu.py
runs its tool.  The tool holds the checks (fresh processes it starts and ends itself); the timeout is only the backstop against a hang."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_two_chunks():
    """loss1 is the single-process step's on the 8-pair batch (1e-2, the model tests' loss tolerance); parameter checksums equal
    across the ranks after every step; bytes_sent equal to the n = 1 step's (one exchange, not two); a rank built with another
    micro_batches raises on both ranks"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "dist_micro_batch_smoke.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "DIST_MICRO_BATCH_OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    said = [l for l in lines if "micro: replicas equal after every step, one exchange per step, same loss1 on both ranks" in l]
    assert len(said) == 2 and {l.split("]")[0] for l in said} == {"[rank 0", "[rank 1"}, said
    raised = [l for l in lines if "MICRO_MISMATCH_RAISED" in l]
    assert len(raised) == 2 and {l.split("]")[0] for l in raised} == {"[rank 0", "[rank 1"}, raised
    assert all("micro_batches differs between the ranks" in l for l in raised), raised
    steps = {rk: [l for l in lines if l.startswith(f"[rank {rk}] step ")] for rk in (0, 1)}
    assert len(steps[0]) == len(steps[1]) == 2
    for l in steps[0] + steps[1]:
        sent, plain = l.split("bytes_sent ")[1].split(" (n = 1: ")
        assert int(sent) == int(plain.rstrip(")")) > 0, l
    whole = [l for l in lines if l.startswith("single-process step on the 8-pair batch")]
    assert len(whole) == 1
