"""FusedTorchSGD across data-parallel ranks (run with -m gpu): tools/dist_finetune_smoke.py --opt sgd as a child process, two ranks
on the one GPU of the test box over gloo, in the way tests/test_v1_finetune_dist_gpu.py runs the tool with AdamW.  The tool holds
the checks; the timeout is only the backstop against a hang (a rank that fails ends the child at once)."""
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
    cmd = [sys.executable, os.path.join(ROOT, "tools", "dist_finetune_smoke.py"), "--opt", "sgd", *checks]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "DIST_FINETUNE_OK " + " ".join(checks) in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_sgd_replicas_probe_and_optimizer_mismatch():
    """one pair of processes: identical shards reproduce the single-process SGD step bit for bit (parameters, momentum buffer,
    shadows); 3 steps on distinct shards with per-rank masks and Mixup plans leave replicas_checksum() and the momentum buffer's
    checksum equal across the ranks; the linear probe across ranks sends the head alone and leaves every bit of the tower;
    AdamW on rank 0 beside SGD on rank 1 raises on BOTH ranks, as do two SGD ranks that differ in `nesterov`"""
    out = run_checks("identical", "replicas", "travel", "optimizers")
    for name in ("clip off", "clip on", "update_freq 2"):
        assert out.count(f"identical shards, {name}: bit-equal") == 2, name
    assert out.count("replicas: parameters and moments equal on both ranks after 3 steps") == 2
    for what in ("fp32 all", "bf16 all", "fp32 head"):
        assert out.count(f"travel {what}:") == 2, what
    for what in ("kind", "nesterov"):
        raised = [l for l in out.splitlines() if f"OPTIMIZER_MISMATCH_RAISED ({what})" in l]
        assert len(raised) == 2 and {l.split("]")[0] for l in raised} == {"[rank 0", "[rank 1"}, raised
