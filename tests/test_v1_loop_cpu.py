"""The v1 fine-tuning loop without a GPU: cosine_scheduler against the reference's output (tests/golden/v1_loop.npz, made by
tests/golden/make_golden_v1_loop.py), the overflow guard's rule (tests/v1_guard_ref.py) against real torch optimizers on the CPU whose
step() is not called on a poisoned iteration, and train_one_epoch's schedule assignment against a hand-written table."""
import os

import numpy as np
import pytest
import torch

import v1_ema_ref as E
import v1_guard_ref as GR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "v1_loop.npz")
# (base_value, final_value, epochs, niter_per_ep, warmup_epochs, start_warmup_value, warmup_steps): the issue's four cases
CASES = [(1e-3, 1e-6, 3, 5, 1, 0, -1), (1e-3, 1e-6, 3, 5, 1, 1e-6, 7), (0.05, 0.05, 2, 4, 0, 0, -1), (0.1, 1e-6, 2, 3, 0, 0, 2)]


# ================================================================================================ 1. cosine_scheduler
@pytest.mark.parametrize("i", range(4))
def test_cosine_scheduler_against_the_reference(i):
    from tvts_amd.downstream.finetune_v1 import cosine_scheduler
    z = np.load(GOLDEN)
    c = CASES[i]
    assert np.array_equal(z["cases"][i], np.array(c, dtype=np.float64))
    if i == 3:  # warmup_steps > 0 with warmup_epochs == 0: the reference's length assertion fails, and so does this one
        assert int(z["raises3"]) == 1
        with pytest.raises(AssertionError):
            cosine_scheduler(*c)
        return
    assert int(z[f"raises{i}"]) == 0
    got, want = cosine_scheduler(*c), z[f"schedule{i}"]
    assert got.dtype == np.float64 and got.shape == want.shape == (c[2] * c[3],)
    np.testing.assert_array_max_ulp(got, want, maxulp=1)  # (math.cos is not correctly rounded across libms)


# ================================================================================================ 2. the guard rule
N, LR, WD, DECAY = 1500, 0.1, 0.05, 0.9999
SEQUENCES = {"first": (4, [0]), "second_of_four": (4, [1]), "two_in_a_row": (5, [1, 2])}


def grads_of(seq, seed):
    steps, poison = SEQUENCES[seq]
    rng = np.random.RandomState(seed)
    p0 = rng.standard_normal(N).astype(np.float32)
    grads = [(rng.standard_normal(N) * 0.3).astype(np.float32) for _ in range(steps)]
    for k, idx, val in zip(poison, (0, N - 1), (np.inf, np.nan)):
        grads[k][idx] = val
    return p0, grads, poison


def torch_run(make, p0, grads, poison):
    """a real torch optimizer; on a poisoned iteration step() is simply not called -> (parameter, optimizer, per-call averages)"""
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = make([tp])
    ema, d32, o32 = p0.copy(), *E.ema_pair(DECAY)
    for k, g in enumerate(grads):
        if k in poison:
            continue
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        ema = E.ema_ref(ema, tp.detach().numpy(), DECAY)
    return tp, opt, ema


@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_guard_rule_is_an_omitted_sgd_step_bit_for_bit(seq):
    p0, grads, poison = grads_of(seq, 31)
    tp, opt, ema = torch_run(lambda ps: torch.optim.SGD(ps, lr=LR, momentum=0.9, weight_decay=WD, nesterov=True, foreach=False), p0, grads, poison)
    got = GR.guarded_run("sgd", p0, grads, lr=LR, wd=WD, momentum=0.9, nesterov=True, decay=DECAY)
    assert got["skipped"] == len(poison) and got["step"] == len(grads) - len(poison)
    assert [bool(np.isfinite(n)) for n in got["norms"]] == [k not in poison for k in range(len(grads))]
    assert np.array_equal(got["p"].view(np.uint32), tp.detach().numpy().view(np.uint32))
    assert np.array_equal(got["m"].view(np.uint32), opt.state[tp]["momentum_buffer"].numpy().view(np.uint32))
    assert np.array_equal(got["ema"].view(np.uint32), ema.view(np.uint32)) and np.isfinite(got["p"]).all()


# torch.optim.AdamW forms exp_avg with lerp and the update with addcdiv (p + value * (m / denom)); the kernel, and adamw_ref with
# it, computes b1 m + (1 - b1) g and p - (ss m) / denom.  Per update the two differ by a few roundings: of the update (at most about
# 10 lr in the first steps, relative 2^-22 for four roundings) and one of p.  A step wrongly applied or left out moves p by about lr.
def adam_tol(p, n):
    return n * (10 * 1e-3 * 2.0 ** -22 + 2.0 ** -23 * np.abs(p))


@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_guard_rule_is_an_omitted_adamw_step(seq):
    p0, grads, poison = grads_of(seq, 32)
    tp, opt, _ = torch_run(lambda ps: torch.optim.AdamW(ps, lr=1e-3, weight_decay=WD, foreach=False), p0, grads, poison)
    got = GR.guarded_run("adamw", p0, grads, lr=1e-3, wd=WD)
    n = len(grads) - len(poison)
    assert got["skipped"] == len(poison) and got["step"] == n == int(opt.state[tp]["step"])
    want = tp.detach().numpy()
    assert (np.abs(got["p"] - want) <= adam_tol(want, n)).all()
    for k, key in (("m", "exp_avg"), ("v", "exp_avg_sq")):
        w = opt.state[tp][key].numpy()
        assert np.abs(got[k] - w).max() <= 2.0 ** -20 * np.abs(w).max(), key
    # and the rule is not vacuous: the run that does step on a clean copy of the poisoned gradient lands elsewhere
    clean = [np.nan_to_num(g, nan=0.0, posinf=0.0) for g in grads]
    other = GR.guarded_run("adamw", p0, clean, lr=1e-3, wd=WD)
    assert other["step"] == len(grads) and not (np.abs(other["p"] - want) <= adam_tol(want, n)).all()


# ================================================================================================ 3. the schedule assignment
class FakeOpt:
    def __init__(self):
        self.param_groups = [dict(lr=9.0, weight_decay=0.3, lr_scale=1.0), dict(lr=9.0, weight_decay=0.0, lr_scale=0.5)]

    def zero_grad(self):
        pass


class FakeStep:
    """records the param_groups every call sees; the outputs are CPU scalars"""

    def __init__(self, update_freq):
        self.opt, self.update_freq, self.skip_nonfinite, self.calls = FakeOpt(), update_freq, False, 0
        self.skipped = torch.zeros(1, dtype=torch.int64)
        self.seen = []

    def step(self, samples, targets, mix=None, aug=None):
        self.seen.append([(g["lr"], g["weight_decay"]) for g in self.opt.param_groups])
        self.calls += 1
        updating = self.calls % self.update_freq == 0
        return dict(loss=torch.tensor(float(self.calls)), logits=None, grad_norm=torch.tensor(2.0) if updating else None, class_acc=torch.tensor(0.5))


LR_S = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
WD_S = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]


@pytest.mark.parametrize("update_freq", [1, 2])
def test_schedule_assignment_table(update_freq):
    from tvts_amd.downstream.finetune_v1 import train_one_epoch
    step = FakeStep(update_freq)
    loader = [(torch.zeros(1), torch.zeros(1), None, None)] * (3 * update_freq + 2)  # two micro-steps beyond the epoch
    stats = train_one_epoch(step, loader, 1, start_steps=2, lr_schedule_values=LR_S, wd_schedule_values=WD_S, num_training_steps_per_epoch=3,
                            update_freq=update_freq, print_freq=2)
    # it = 2 + data_iter_step // update_freq; the lr schedule assigns on EVERY micro-step (:47's precedence) with the same it;
    # group 1 (weight_decay 0) keeps 0 and takes lr * its lr_scale; micro-steps with step >= 3 never reach the step
    want = [[(LR_S[2 + k // update_freq], WD_S[2 + k // update_freq]), (0.5 * LR_S[2 + k // update_freq], 0.0)] for k in range(3 * update_freq)]
    assert step.seen == want and step.calls == 3 * update_freq
    n = 3 * update_freq
    assert stats == dict(loss=sum(range(1, n + 1)) / n, class_acc=0.5, lr=sum(w[0][0] for w in want) / n, min_lr=sum(w[1][0] for w in want) / n,
                         weight_decay=sum(w[0][1] for w in want) / n, grad_norm=2.0, skipped=0.0)


def test_weight_decay_schedule_alone_assigns_on_the_first_micro_step_only():
    """:47 without an lr schedule: `wd is not None and data_iter_step % update_freq == 0`"""
    from tvts_amd.downstream.finetune_v1 import train_one_epoch
    step = FakeStep(2)
    hits = []

    class Spy(list):
        def __getitem__(self, i):
            hits.append(i)
            return WD_S[i]
    train_one_epoch(step, [(torch.zeros(1), torch.zeros(1))] * 4, 0, wd_schedule_values=Spy(), num_training_steps_per_epoch=2, update_freq=2)
    assert hits == [0, 1] and [s[0] for s in step.seen] == [(9.0, 0.1), (9.0, 0.1), (9.0, 0.2), (9.0, 0.2)] and all(s[1] == (9.0, 0.0) for s in step.seen)


def test_loop_refusals_and_mixup_meter():
    from tvts_amd.downstream.finetune_v1 import train_one_epoch
    loader = [(torch.zeros(1), torch.zeros(1))] * 2
    with pytest.raises(ValueError, match="skip_nonfinite"):  # "skip" without the guard would train on NaN
        train_one_epoch(FakeStep(1), loader, 0, on_nonfinite="skip")
    with pytest.raises(ValueError):
        train_one_epoch(FakeStep(1), loader, 0, on_nonfinite="ignore")
    with pytest.raises(ValueError, match="update_freq"):
        train_one_epoch(FakeStep(1), loader, 0, update_freq=2)

    class NanStep(FakeStep):
        def step(self, *a, **k):
            out = super().step(*a, **k)
            if self.calls == 2:
                out["loss"] = torch.tensor(float("nan"))
            return out
    s = NanStep(1)
    with pytest.raises(FloatingPointError, match=r"iteration 6\b"):
        train_one_epoch(s, [loader[0]] * 4, 0, start_steps=5, print_freq=3)
    assert s.calls == 4  # (the readout behind micro-step 3: the host does not look on every step)
