"""The bits of the flat-store optimizer launches against digests recorded from an earlier tree (run with -m gpu).

tests/golden/optim_bits.npz (tests/golden/make_golden_optim_bits.py) holds the SHA-256 of p, the state buffers, the bf16 shadow and
the average after each of three steps of K.adamw_torch, K.sgd_torch and K.adamw_hf in their host-step / step_dev, momentum and
ema variants.  The other optimizer tests hold the kernels to per-element bounds and to equality BETWEEN variants; a change of
operation order that moves every variant alike passes those and fails here.  The guarded launches are tied to these by
tests/test_v1_guard_gpu.py::test_guarded_launch (bit equality with the unguarded launch)."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_optimizer_launches_keep_the_recorded_bits(golden):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip as K
    spec = importlib.util.spec_from_file_location("make_golden_optim_bits", os.path.join(HERE, "golden", "make_golden_optim_bits.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    fx = golden("optim_bits")
    want = {n.decode(): bytes(d) for n, d in zip(fx["names"], fx["digests"])}
    got = rec.record(K)
    assert list(got) == list(want), "the recorder and the fixture name other (call, step, buffer) triples"
    assert len(got) == 192  # 18 calls x 3 steps x (p, shadow, the rule's state, the average): 64 buffers per step
    for name in got:  # in the order the calls were made: the first difference is the one to look at
        assert got[name] == want[name], f"{name} (call/step/buffer): the bytes differ from the recorded ones"
