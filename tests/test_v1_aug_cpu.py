"""Random-resized crop, flip and random erasing of the v1 fine-tuning step, host side (no GPU):
tvts_amd.downstream.finetune_v1.Augment.draw against the draws recorded from the reference's own run (tests/golden/v1_aug.npz, made
by tests/golden/make_golden_v1_aug.py), the restatement tests/v1_aug_ref.py against the same run's clips, the noise rule's
distribution, and the host-side refusals."""
import math
import random

import numpy as np
import pytest

import v1_aug_ref as A

NAMES = list(A.CASES)


@pytest.fixture(scope="module")
def fx(golden):
    f = golden("v1_aug")
    assert [str(n) for n in f["names"]] == NAMES and (int(f["img"]), int(f["T"])) == (A.IMG, A.T)
    return f


def seeded_draw(f, name):
    """Augment.draw under the seeds of the fixture's run (the generators' states are put back afterwards)"""
    from tvts_amd.downstream.finetune_v1 import Augment
    Bs, H0, W0 = (int(v) for v in f[name + ".shape"])
    seed = int(f[name + ".seed"])
    py_state, np_state = random.getstate(), np.random.get_state()
    try:
        random.seed(seed)
        np.random.seed(seed)
        return Augment(A.IMG, noise_seed=seed, **A.case_cfg(f, name)).draw(Bs, H0, W0)
    finally:
        random.setstate(py_state)
        np.random.set_state(np_state)


@pytest.mark.parametrize("name", NAMES)
def test_draw_reproduces_the_reference_draw(fx, name):
    """seeded as the reference's run was, draw() makes the same random / np.random calls in the same order: the same table"""
    plan = seeded_draw(fx, name)
    kwargs, Bs, H0, W0, want = A.CASES[name]
    assert plan.aug_i.dtype == np.int32 and plan.aug_i.shape == (Bs * kwargs["num_sample"], 16) and len(plan) == Bs * kwargs["num_sample"]
    assert plan.aug_i.tolist() == fx[name + ".aug_i"].tolist(), name
    assert plan.aug_i[:, 0].tolist() == [b // kwargs["num_sample"] for b in range(len(plan))]  # the collate order of the views
    assert A.holds(want, plan.aug_i, fx[name + ".fallback"], H0, W0)


def test_fixture_covers_both_num_sample_and_what_the_tests_rely_on(fx):
    assert {A.CASES[n][0]["num_sample"] for n in NAMES} == {1, 2}
    seen = dict.fromkeys(("up", "down", "fallback", "interior", "oddbox", "unerased", "flipped"), False)
    for n in NAMES:
        _, _, H0, W0, _ = A.CASES[n]
        for w in seen:
            seen[w] |= A.holds(w, fx[n + ".aug_i"], fx[n + ".fallback"], H0, W0)
    assert all(seen.values()), seen
    assert {int(m) for n in NAMES for m in fx[n + ".aug_i"][:, 6]} == {0, 1, 2, 3}


def test_noise_keys_advance_per_sample_and_leave_the_generators_alone():
    from tvts_amd.downstream.finetune_v1 import Augment, splitmix64
    fn = Augment(A.IMG, reprob=0.0, noise_seed=7)
    py_state, np_state = random.getstate(), np.random.get_state()
    try:
        random.seed(3)
        np.random.seed(3)
        keys = [A.key_of(r) for _ in range(2) for r in fn.draw(3, 20, 30).aug_i]
        after = random.random(), np.random.uniform()
        random.seed(3)
        np.random.seed(3)
        other = Augment(A.IMG, reprob=0.0, noise_seed=8)
        keys2 = [A.key_of(r) for _ in range(2) for r in other.draw(3, 20, 30).aug_i]
        assert after == (random.random(), np.random.uniform())  # another noise seed: the same draws
    finally:
        random.setstate(py_state)
        np.random.set_state(np_state)
    assert keys == [(splitmix64(7) + i) % (1 << 64) for i in range(6)] and keys2 == [(splitmix64(8) + i) % (1 << 64) for i in range(6)]
    assert splitmix64(0) == 0xE220A8397B1DCDAF  # the first output of the published splitmix64 generator seeded with 0


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_the_reference_run_outside_the_erase_box(fx, name):
    """aug_clip from the recorded table against the reference's fp32 clips: |d| <= 2e-6 outside the erase box (values are at most
    2.64 in size, fp32 ulp 2.4e-7, and the reference's path has about 6 fp32 roundings: ~1e-6); const boxes are exact zeros;
    pixel / rand boxes sit where the reference's do (inside them the reference holds torch's noise, not the picture)"""
    _, Bs, H0, W0, _ = A.CASES[name]
    frames = A.case_frames(int(fx[name + ".frame_seed"]), Bs, H0, W0)
    aug_i, ref = fx[name + ".aug_i"], fx[name + ".clips"]
    assert ref.dtype == np.float32
    plain = A.aug_clip(frames, aug_i, erase=False)
    mine = A.aug_clip(frames, aug_i)
    worst = 0.0
    for b, row in enumerate(aug_i):
        m = A.box_mask(row, A.IMG)
        assert m.any() == bool(row[6])
        worst = max(worst, float(np.abs(mine[b] - ref[b])[:, :, ~m].max()))
        assert np.array_equal(mine[b][:, :, ~m], plain[b][:, :, ~m])
        if int(row[6]) == 1:
            assert not ref[b][:, :, m].any() and not mine[b][:, :, m].any()
        elif int(row[6]):
            # the reference's box: its values there are not the resized picture's (a normal sample equals one with probability 0)
            assert (np.abs(ref[b] - plain[b])[:, :, m] > 2e-6).all()
            assert (np.abs(mine[b] - plain[b])[:, :, m] > 2e-6).mean() > 0.99
            if int(row[6]) == 2:   # rand: one value per (channel, frame) over the box, in the reference and here
                assert all((v[:, :, m] == v[:, :, m][..., :1]).all() for v in (ref[b], mine[b]))
    print(f"{name}: max |restatement - reference| outside the boxes = {worst:.3e}")
    assert worst <= 2e-6


def ks_normal(z):
    z = np.sort(z)
    n = len(z)
    cdf = 0.5 * (1.0 + np.array([math.erf(v / math.sqrt(2.0)) for v in z]))
    return max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))


@pytest.mark.parametrize("key", [1, 12345, 0xDEADBEEFCAFE])
@pytest.mark.parametrize("n", [1188, 96000])
def test_noise_rule_is_standard_normal(key, n):
    """mean, variance, Kolmogorov-Smirnov distance, lag-1 correlation and the largest value of z(key, 0 .. n - 1).  The gates are
    four standard errors (KS: the 0.1 % point of the Kolmogorov distribution, 1.95); |z| <= sqrt(-2 ln 2^-32) = 6.66 by construction"""
    z = A.noise(key, np.arange(n))
    mean, var = z.mean(), z.var()
    lag = float(np.corrcoef(z[:-1], z[1:])[0, 1])
    stats = (abs(mean) * math.sqrt(n), abs(var - 1) * math.sqrt(n / 2), ks_normal(z) * math.sqrt(n), abs(lag) * math.sqrt(n), np.abs(z).max())
    print("key %#x n %d: mean %.2f var %.2f ks %.2f lag %.2f max %.2f" % ((key, n) + stats))
    assert stats[0] < 4 and stats[1] < 4 and stats[2] < 1.95 and stats[3] < 4 and stats[4] <= 6.67


def test_rand_stream_is_separate_from_the_pixel_stream():
    a, b = A.noise(12345, np.arange(64)), A.noise(12345 + A.RAND_STREAM, np.arange(64))
    assert not np.isclose(a, b).any()


def test_recount_other_than_one_is_refused():
    from tvts_amd.downstream.finetune_v1 import Augment
    for recount in (0, 2):
        with pytest.raises(ValueError):
            Augment(A.IMG, recount=recount)
    with pytest.raises(ValueError):
        Augment(A.IMG, remode="colour")


GOOD = [[1, 2, 3, 20, 30, 0, 3, 4, 5, 6, 7, -5, 9, 0, 0, 0], [0, 0, 0, 37, 53, 1, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0]]
SHAPE = dict(Bs=2, H0=37, W0=53, img=16)


def test_wrapper_accepts_a_valid_plan():
    from tvts_amd import hip
    ai = hip.check_aug_plan(np.array(GOOD), **SHAPE)
    assert ai.dtype == np.int32 and ai.tolist() == GOOD
    assert hip.check_aug_plan(np.array([[0, 0, 0, 1, 1] + [0] * 6 + [0xFFFFFFFF, 0, 0, 0, 0]]), **SHAPE)[0, 11] == -1  # an unsigned key word


@pytest.mark.parametrize("col,value", [(0, 2), (0, -1), (1, -1), (1, 18), (2, -1), (2, 24), (3, 0), (3, 36), (4, 0), (4, 51), (5, 2), (5, -1),
                                       (6, 4), (6, -1), (7, -1), (7, 11), (8, -1), (8, 10), (9, -1), (9, 13), (10, -1), (10, 12),
                                       (11, 1 << 32), (13, 1), (14, 1), (15, -1)], ids=lambda v: str(v))
def test_wrapper_refuses_a_bad_plan_before_any_launch(col, value):
    """every column out of its range -- a crop that leaves the frame among them --: ValueError from the host check, in front of the
    upload (aug_table raises before it touches a device: this test runs without one)"""
    from tvts_amd import hip
    bad = np.array(GOOD, dtype=np.int64)
    bad[0, col] = value
    with pytest.raises(ValueError):
        hip.check_aug_plan(bad, **SHAPE)
    with pytest.raises(ValueError):
        hip.aug_table(bad, device="cuda", **SHAPE)


def test_wrapper_refuses_a_misshapen_plan():
    from tvts_amd import hip
    with pytest.raises(ValueError):
        hip.check_aug_plan(np.array(GOOD)[:, :15], **SHAPE)
    with pytest.raises(ValueError):
        hip.check_aug_plan(np.array(GOOD, dtype=np.float32), **SHAPE)
    with pytest.raises(ValueError):
        hip.check_aug_plan(np.zeros((0, 16), dtype=np.int32), **SHAPE)
