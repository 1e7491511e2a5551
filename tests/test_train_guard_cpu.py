"""CPU side of gradient clipping / the overflow guard of the pretraining step: the two config keys, the named refusals and the
composed reference step of tests/train_guard_ref.py (no GPU needed)."""
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_guard_ref as G  # noqa: E402

from oracle import tvts_oracle as O  # noqa: E402


def test_config_keys():
    from tvts_amd.base.base_trainer import guard_config
    base = dict(epochs=1, save_period=1, verbosity=2)
    assert guard_config(base) == (None, False)                      # keys absent: the trainer of today
    assert guard_config(dict(base, clip_grad=None)) == (None, False)
    assert guard_config(dict(base, clip_grad=1)) == (1.0, False) and isinstance(guard_config(dict(base, clip_grad=1))[0], float)
    assert guard_config(dict(base, clip_grad=0.5, skip_nonfinite=True)) == (0.5, True)
    assert guard_config(dict(base, skip_nonfinite=True)) == (None, True)
    for bad in (0, -1.0, float("inf"), float("nan"), "1.0", True, [1.0]):
        with pytest.raises(ValueError, match="clip_grad"):
            guard_config(dict(base, clip_grad=bad))
    for bad in (1, "true", None, 0.0):
        with pytest.raises(ValueError, match="skip_nonfinite"):
            guard_config(dict(base, skip_nonfinite=bad))


def test_step_options_and_named_refusals():
    from tvts_amd.step import guard_options
    assert guard_options(None, False, fused=True, ranged=False) == (None, False)
    assert guard_options(None, False, fused=False, ranged=True) == (None, False)   # both off: nothing to refuse
    assert guard_options(0, False, fused=False, ranged=True) == (None, False)      # 0 is "off", as FinetuneStep reads it
    assert guard_options(2, True, fused=True, ranged=False) == (2.0, True)
    for kw, name in ((dict(clip_grad=1.0, skip_nonfinite=False), "clip_grad"), (dict(clip_grad=None, skip_nonfinite=True), "skip_nonfinite"),
                     (dict(clip_grad=1.0, skip_nonfinite=True), "clip_grad / skip_nonfinite")):
        with pytest.raises(RuntimeError, match="adamw_ranges / TVTS_ADAMW_RANGES=1") as e:
            guard_options(**kw, fused=True, ranged=True)
        assert f"StepRunner({name})" in str(e.value)
        with pytest.raises(RuntimeError, match="needs the fused optimizer") as e:
            guard_options(**kw, fused=False, ranged=False, optimizer="AdamW")
        assert f"StepRunner({name})" in str(e.value) and "got AdamW" in str(e.value)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="positive finite max_norm"):
            guard_options(bad, False, fused=True, ranged=False)


def test_ranged_update_names_the_conflict():
    """FusedHFAdamW.begin_ranges refuses in front of everything else it does: no store, no device needed to see the message"""
    from tvts_amd.optim import FusedHFAdamW
    fake = types.SimpleNamespace(norm_coef=torch.zeros(2), _cls="FusedHFAdamW")
    with pytest.raises(RuntimeError, match=r"ranged updates .* gradient clipping \(norm_coef\)"):
        FusedHFAdamW.begin_ranges(fake)
    fake.norm_coef = None
    with pytest.raises(RuntimeError, match="ranged updates .* the overflow guard"):
        FusedHFAdamW.begin_ranges(fake, guard=True)


def test_header_states_the_new_entry_points():
    from tvts_amd import _lib
    protos = _lib.parse_header()
    names = protos["tvts_adamw_hf_guarded"][2]
    assert names[:16] == protos["tvts_adamw_hf"][2][:16] and names[15:] == ["grad_scale", "norm_coef", "skipped", "stream"]
    assert protos["tvts_fp8_update_scales_guarded"][2] == ["amax", "scale", "n", "guard_norm", "stream"]
    assert protos["tvts_adamw_hf"][2][-1] == "stream" and len(protos["tvts_adamw_hf"][2]) == 17  # the old entry point as it was
    assert protos["tvts_fp8_update_scales"][2] == ["amax", "scale", "n", "stream"]


def test_clip_by_hand_on_two_tensors():
    """g = (3, 4) and (12,): norm 13.  max_norm 6.5: coefficient 6.5 / (13 + 1e-6); max_norm 26: no clipping."""
    a, b = torch.tensor([3.0, 4.0]), torch.tensor([12.0])
    total, coef, out = G.clip_by_hand([a, b], 6.5)
    assert total == 13.0 and coef == 6.5 / (13.0 + 1e-6)
    assert torch.equal(out[0], a * coef) and torch.equal(out[1], b * coef)
    total, coef, out = G.clip_by_hand([a, b], 26.0)
    assert coef == 1.0 and torch.equal(out[0], a) and torch.equal(out[1], b)
    # torch's own rule gives the same numbers
    pa, pb = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(1))
    pa.grad, pb.grad = a.clone(), b.clone()
    assert float(torch.nn.utils.clip_grad_norm_([pa, pb], 6.5)) == 13.0
    _, coef, out = G.clip_by_hand([a, b], 6.5)
    assert torch.allclose(pa.grad, out[0], rtol=1e-6, atol=0) and torch.allclose(pb.grad, out[1], rtol=1e-6, atol=0)


def test_composed_oracle_step():
    """without a max_norm the composed step IS O.train_step; with norm_fraction 0.5 the clip is active, its coefficient the
    hand-computed one, and the first AdamW step (sign-like: m / sqrt(v) is g / |g| at step 1) still moves every weight"""
    from tvts_amd import arch as A
    oarch = O.tiny_arch(**A.small_arch())
    P = O.synth_params(oarch, seed=3)
    batch = O.synth_batch(oarch, B=2, T=2, seed=4, caption_len=8)
    Pa, Pb, Pc = ({k: v.clone() for k, v in P.items()} for _ in range(3))
    sa, sb, sc = {}, {}, {}
    r1, r2, grads = O.train_step(Pa, batch, oarch, sa)
    plain = G.clipped_oracle_step(Pb, batch, oarch, sb)
    assert (plain["loss1"], plain["loss2"], plain["coef"]) == (r1, r2, 1.0)
    for k in P:
        assert torch.equal(Pa[k], Pb[k]), k
    total, coef, _ = G.clip_by_hand(list(grads.values()), 0.5 * plain["norm"])
    assert abs(total - plain["norm"]) <= 1e-5 * total
    clipped = G.clipped_oracle_step(Pc, batch, oarch, sc, norm_fraction=0.5)
    assert clipped["coef"] < 0.9 and abs(clipped["coef"] - coef) <= 1e-5 and math.isclose(clipped["max_norm"], 0.5 * plain["norm"], rel_tol=1e-6)
    k = "pred_model.head.weight"
    assert torch.allclose(sc["m"][k], sb["m"][k] * clipped["coef"], rtol=1e-5, atol=1e-12) and not torch.equal(Pc[k], P[k])


def test_prescaled_gradient_and_nan_pixel():
    g = torch.tensor([1.0, -3.0, 0.1], dtype=torch.float32)
    s, c = torch.tensor(0.3, dtype=torch.float32), torch.tensor(0.37, dtype=torch.float32)
    want = torch.stack([(x * s) * c for x in g])
    assert torch.equal(G.prescaled(g, 0.3, 0.37), want)
    b = dict(video=torch.zeros(2, 2, 3, 4, 4), text=torch.zeros(2, 3), keep_ind=torch.tensor([[0, 1], [3, 2]]))
    nb = G.nan_pixel(b, dict(patch=2, image=4), sample=1)
    assert int(torch.isnan(nb["video"]).sum()) == 1 and bool(torch.isnan(nb["video"][1, 0, 0, 2, 2])) and not bool(torch.isnan(b["video"]).any())
    assert nb["text"] is b["text"]
