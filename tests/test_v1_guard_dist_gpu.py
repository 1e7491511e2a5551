"""The overflow guard across data-parallel ranks (run with -m gpu): tools/dist_finetune_smoke.py --guard as a child process, two
ranks on the one GPU of the test box over gloo, in the way tests/test_v1_sgd_dist_gpu.py runs the tool.  The tool holds the checks
(fresh processes it starts and ends itself); the timeout is only the backstop against a hang."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("opt", ["adamw", "sgd"])
def test_one_ranks_nan_skips_the_update_on_both(opt):
    """the NaN pixel is in rank 1's shard only, on call 2 of 3: both ranks report skipped == 1, equal replicas_checksum() after
    every call and an equal, finite state at the end; a rank with skip_nonfinite=True beside one with False raises on both"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "dist_finetune_smoke.py"), "--guard", "--opt", opt]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "DIST_FINETUNE_OK guard" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    said = [l for l in r.stdout.splitlines() if "guard: skipped 1, replicas equal after every call, finite state at the end" in l]
    assert len(said) == 2 and {l.split("]")[0] for l in said} == {"[rank 0", "[rank 1"}, said
    raised = [l for l in r.stdout.splitlines() if "GUARD_MISMATCH_RAISED" in l]
    assert len(raised) == 2 and {l.split("]")[0] for l in raised} == {"[rank 0", "[rank 1"}, raised
