"""ModelEma across data-parallel ranks (run with -m gpu): tools/dist_finetune_smoke.py --ema once, as a fresh child process -- two
ranks on the one GPU over gloo, the way tests/test_v1_finetune_dist_gpu.py starts the tool.  The tool's check_ema holds the
assertions on the tensors; this file reads the checksums both ranks report.  The timeout is only the backstop against a hang."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_average_is_rank_zeros_masters_after_join_and_stays_equal():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "dist_finetune_smoke.py"), "--ema"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "DIST_FINETUNE_OK ema" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    join = {int(m[1]): (int(m[2]), int(m[3]), int(m[4])) for m in
            re.finditer(r"\[rank (\d)\] EMA after _join: checksum (-?\d+) master (-?\d+) built-from (-?\d+)", r.stdout)}
    assert set(join) == {0, 1}, join
    assert join[0][2] != join[1][2], "both ranks built their average from the same weights"
    # the two checksums are equal after _join, and they equal rank 0's master checksum there (= what rank 0 was built from)
    assert join[0][0] == join[1][0] == join[0][1] == join[1][1] == join[0][2], join
    after = {int(m[1]): (int(m[2]), int(m[3])) for m in
             re.finditer(r"\[rank (\d)\] EMA after 2 updating steps: checksum (-?\d+) master (-?\d+)", r.stdout)}
    assert set(after) == {0, 1} and after[0] == after[1], after
    assert after[0][0] != join[0][0] and after[0][0] != after[0][1], (join, after)
    assert r.stdout.count("EMA_MISMATCH_RAISED") == 2
