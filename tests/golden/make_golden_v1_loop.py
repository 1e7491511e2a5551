#!/usr/bin/env python3
"""Generate tests/golden/v1_loop.npz by RUNNING THE REFERENCE's cosine_scheduler (v1/downstream/utils.py:399-416; build container only).

utils.py is loaded read-only through the `_load` / `_stub` shims of make_golden_v1.py; ``timm.utils``, ``torch._six`` and
``tensorboardX`` are stubbed (none is reached by cosine_scheduler, none is installed in the build container).  No reference file
is edited or copied; the fixture holds arrays only: per case the seven arguments and the returned float64 schedule, and for the
case the reference refuses (its length assertion) a flag.  The generator asserts that this project's cosine_scheduler returns the
same BITS on the machine that makes the fixture; tests/test_v1_loop_cpu.py allows 1 ulp (math.cos is not correctly rounded across
libms).

    python tests/golden/make_golden_v1_loop.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TVTS_REFERENCE_V1", "/root/reference/v1")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tests.golden.make_golden_v1 import _load, _stub, save  # noqa: E402

# (base_value, final_value, epochs, niter_per_ep, warmup_epochs, start_warmup_value, warmup_steps)
CASES = [(1e-3, 1e-6, 3, 5, 1, 0, -1), (1e-3, 1e-6, 3, 5, 1, 1e-6, 7), (0.05, 0.05, 2, 4, 0, 0, -1), (0.1, 1e-6, 2, 3, 0, 0, 2)]


def main():
    _stub("timm")
    _stub("timm.utils", get_state_dict=None)
    _stub("torch._six", inf=float("inf"))
    _stub("tensorboardX", SummaryWriter=object)
    utils = _load("utils", os.path.join(REF, "downstream", "utils.py"))
    from tvts_amd.downstream.finetune_v1 import cosine_scheduler
    arrays = {"cases": np.array(CASES, dtype=np.float64)}
    for i, c in enumerate(CASES):
        args = (c[0], c[1], int(c[2]), int(c[3]), int(c[4]), c[5], int(c[6]))
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                want = utils.cosine_scheduler(*args)
        except AssertionError:
            arrays[f"raises{i}"] = np.array(1)
            try:
                cosine_scheduler(*args)
            except AssertionError:
                continue
            raise SystemExit(f"case {i}: the reference raises AssertionError, this project does not")
        assert want.dtype == np.float64
        got = cosine_scheduler(*args)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64)), f"case {i}: not the reference's bits"
        arrays[f"raises{i}"], arrays[f"schedule{i}"] = np.array(0), want
    save("v1_loop", **arrays)


if __name__ == "__main__":
    main()
