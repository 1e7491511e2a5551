"""Mixup / CutMix of the v1 fine-tuning step, host side (no GPU): tvts_amd.downstream.finetune_v1.Mixup.draw against the draws
recorded from the reference class's runs (tests/golden/v1_mixup.npz, made by tests/golden/make_golden_v1_mixup.py), the restatement
tests/v1_mixup_ref.py against the same runs' bytes, and the host-side refusals of the hip wrappers."""
import numpy as np
import pytest
import torch

import v1_mixup_ref as M

NAMES = list(M.CASES)


@pytest.fixture(scope="module")
def fx(golden):
    f = golden("v1_mixup")
    assert [str(n) for n in f["names"]] == NAMES and (int(f["B"]), int(f["img"]), int(f["T"])) == (M.B, M.IMG, M.T)
    return f


def mixup_of(f, name):
    from tvts_amd.downstream.finetune_v1 import Mixup
    return Mixup(num_classes=int(f[name + ".classes"]), **M.case_cfg(f, name))


@pytest.mark.parametrize("name", NAMES)
def test_draw_reproduces_the_reference_draw(fx, name):
    """seeded as the reference's run was, draw() makes the same np.random calls in the same order: the same table, bit for bit"""
    state = np.random.get_state()
    try:
        np.random.seed(int(fx[name + ".seed"]))
        plan = mixup_of(fx, name).draw(M.B, M.IMG)
    finally:
        np.random.set_state(state)
    assert plan.mix_i.dtype == np.int32 and plan.mix_f.dtype == np.float32
    assert plan.mix_i.tolist() == fx[name + ".mix_i"].tolist(), name
    assert plan.mix_f.tobytes() == fx[name + ".mix_f"].tobytes(), (name, plan.mix_f, fx[name + ".mix_f"])
    assert plan.smoothing == float(fx[name + ".smoothing"])
    assert M.holds(M.CASES[name][2], plan.mix_i)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_the_reference_run(fx, name):
    """tests/v1_mixup_ref.py, from the recorded table, gives the reference's mixed clip (sha256) and its soft targets (bytes)"""
    clip, labels = M.case_inputs(fx, name)
    mi, mf = fx[name + ".mix_i"], fx[name + ".mix_f"]
    assert M.sha256(M.mix_clip(clip, mi, mf)) == str(fx[name + ".sha256"])
    t = M.mix_targets(labels, mi, mf, int(fx[name + ".classes"]), float(fx[name + ".smoothing"]))
    assert t.numpy().tobytes() == fx[name + ".targets"].tobytes()


def test_fixture_holds_what_the_gpu_tests_rely_on(fx):
    boxes = [fx[n + ".mix_i"][b, 2:] for n in NAMES for b in range(M.B) if fx[n + ".mix_i"][b, 1] >= 2]
    assert any(bx[2] % 8 and bx[3] % 8 for bx in boxes) and any(M.clipped(bx) for bx in boxes)
    for mode in ("batch", "pair", "elem"):
        modes = {int(m) for n in NAMES if M.CASES[n][0]["mode"] == mode for m in fx[n + ".mix_i"][:, 1]}
        assert 1 in modes and (2 in modes or 3 in modes), (mode, modes)
    e = fx["elem_prob.mix_i"][:, 1]
    assert 0 in e and e.any()
    assert {int(fx[n + ".classes"]) for n in NAMES} == {5, 174} and {float(fx[n + ".smoothing"]) for n in NAMES} == {0.0, 0.1}


def test_odd_batch_is_refused():
    from tvts_amd.downstream.finetune_v1 import Mixup
    with pytest.raises(ValueError):
        Mixup(num_classes=5).draw(3, 32)


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_disabled_mixup_draws_nothing(mode):
    from tvts_amd.downstream.finetune_v1 import Mixup
    fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=5)
    fn.mixup_enabled = False
    state = np.random.get_state()
    plan = fn.draw(6, 32)
    after = np.random.get_state()
    assert (plan.mix_i[:, 1] == 0).all() and plan.mix_i[:, 0].tolist() == [5, 4, 3, 2, 1, 0] and not plan.mix_i[:, 2:].any()
    assert plan.mix_f.tobytes() == np.array([[1.0, 0.0]] * 6, dtype=np.float32).tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(state, after))  # (the reference makes no draw either, mixup.py:117,137)


def test_constructor_follows_the_reference():
    from tvts_amd.downstream.finetune_v1 import Mixup
    fn = Mixup()
    assert (fn.mixup_alpha, fn.cutmix_alpha, fn.cutmix_minmax, fn.mix_prob, fn.switch_prob, fn.mode, fn.correct_lam,
            fn.label_smoothing, fn.num_classes, fn.mixup_enabled) == (1., 0., None, 1.0, 0.5, "batch", True, 0.1, 1000, True)
    assert Mixup(cutmix_minmax=(0.2, 0.8)).cutmix_alpha == 1.0  # mixup.py:102-105
    with pytest.raises(ValueError):
        Mixup(mixup_alpha=0., cutmix_alpha=0.).draw(4, 32)


GOOD_I = [[1, 1, 0, 0, 0, 0], [0, 2, 3, 9, 0, 32]]
GOOD_F = [[0.25, 0.75], [0.5, 0.5]]


def test_wrappers_accept_a_valid_plan():
    from tvts_amd import hip
    mi, mf = hip.check_mix_plan(np.array(GOOD_I), np.array(GOOD_F), B=2, img=32)
    assert mi.dtype == np.int32 and mf.dtype == np.float32 and mi.tolist() == GOOD_I and mf.tolist() == GOOD_F


@pytest.mark.parametrize("col,value", [(0, 2), (0, -1), (1, 4), (1, -1), (2, -1), (2, 10), (3, 33), (4, -2), (4, 33), (5, 33)],
                         ids=lambda v: str(v))
def test_wrappers_refuse_a_bad_plan_before_any_launch(col, value):
    """partner outside [0, B), an unknown mode, a box outside 0 <= lo <= hi <= img: ValueError from the host check, in front of the
    upload (mix_table raises before it touches a device: this test runs without one)"""
    from tvts_amd import hip
    bad = np.array(GOOD_I)
    bad[1, col] = value
    with pytest.raises(ValueError):
        hip.check_mix_plan(bad, np.array(GOOD_F), B=2, img=32)
    with pytest.raises(ValueError):
        hip.mix_table(bad, np.array(GOOD_F), B=2, img=32, device="cuda")


def test_wrappers_refuse_a_misshapen_plan():
    from tvts_amd import hip
    with pytest.raises(ValueError):
        hip.check_mix_plan(np.array(GOOD_I), np.array(GOOD_F), B=3, img=32)
    with pytest.raises(ValueError):
        hip.check_mix_plan(np.array(GOOD_I, dtype=np.float32), np.array(GOOD_F), B=2, img=32)
    with pytest.raises(ValueError):
        hip.check_mix_plan(np.array(GOOD_I), np.array([[0.5, float("nan")], [1.0, 0.0]]), B=2, img=32)


def test_step_refuses_soft_targets_with_a_plan():
    """FinetuneStep._mixed_targets: with a plan the targets are integer labels (checked on the host, no launch)"""
    from tvts_amd.downstream.finetune_v1 import FinetuneStep, MixPlan
    plan = MixPlan(np.array(GOOD_I, dtype=np.int32), np.array(GOOD_F, dtype=np.float32), 0.1)
    step = FinetuneStep.__new__(FinetuneStep)
    with pytest.raises(ValueError):
        step._mixed_targets(torch.full((2, 5), 0.2), plan, 2, 5, 32, "cpu")
    with pytest.raises(IndexError):
        step._mixed_targets(torch.tensor([0, 5]), plan, 2, 5, 32, "cpu")
