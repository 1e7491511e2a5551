"""Mixup / CutMix of the v1 fine-tuning recipe, restated for the tests from the semantics of the mix table (TEST INFRASTRUCTURE
ONLY; torch on the CPU, separate fp32 multiplies and adds, no fused multiply-add):

    mix_i [B, 6] = (partner, mode, yl, yh, xl, xh)   mode 0 none / 1 mixup / 2 cutmix / 3 pair-mode cutmix (the box over frames x
                                                     rows), the box half-open in image coordinates
    mix_f [B, 2] = (lam, one_minus_lam)              fp32

and the cases of tests/golden/v1_mixup.npz, shared by its generator (tests/golden/make_golden_v1_mixup.py, which runs the reference
class on them) and the tests (which regenerate clips and labels from the stored seeds)."""
from __future__ import annotations

import hashlib
import json

import numpy as np
import torch

B, IMG, T = 4, 32, 4
DEFAULT = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5)  # run_class_finetuning.py's --mixup / --cutmix defaults

# name -> (constructor keywords, classes).  `want`: what the generator's seed search makes sure the case's draw holds.
CASES = {
    "batch_mixup": (dict(DEFAULT, mode="batch", label_smoothing=0.1), 174, "all1"),
    "batch_cutmix": (dict(DEFAULT, mode="batch", label_smoothing=0.1), 5, "all2_odd_x"),
    "pair": (dict(DEFAULT, mode="pair", label_smoothing=0.1), 5, "both"),
    "elem": (dict(DEFAULT, mode="elem", label_smoothing=0.1), 174, "both_clipped"),
    "elem_prob": (dict(DEFAULT, mode="elem", label_smoothing=0.0, prob=0.5), 5, "both_and_unmixed"),
    "batch_prob_off": (dict(DEFAULT, mode="batch", label_smoothing=0.1, prob=0.5), 174, "all0"),
    "batch_minmax": (dict(DEFAULT, mode="batch", label_smoothing=0.0, cutmix_minmax=(0.2, 0.8)), 174, "all2"),
    "elem_minmax": (dict(DEFAULT, mode="elem", label_smoothing=0.1, cutmix_minmax=(0.2, 0.8)), 5, "both"),
    "batch_uncorrected": (dict(DEFAULT, mode="batch", label_smoothing=0.1, correct_lam=False), 5, "all2_clipped"),
    "pair_uncorrected": (dict(DEFAULT, mode="pair", label_smoothing=0.0, correct_lam=False), 174, "both_clipped"),
    "pair_mixup_only": (dict(DEFAULT, mode="pair", label_smoothing=0.1, cutmix_alpha=0.0), 174, "all1"),
    "elem_cutmix_only": (dict(DEFAULT, mode="elem", label_smoothing=0.0, mixup_alpha=0.0), 5, "all2"),
}


def clipped(box, img=IMG):
    """rand_bbox centres a square on a random pixel and clips it: a clipped box touches a border and is no longer the square"""
    yl, yh, xl, xh = (int(v) for v in box)
    return (yl == 0 or yh == img or xl == 0 or xh == img) and (yh - yl) != (xh - xl)


def holds(want, mix_i):
    modes = [int(m) for m in mix_i[:, 1]]
    boxes = [mix_i[b, 2:] for b in range(len(modes)) if modes[b] >= 2]
    if want.startswith("all"):
        ok = all(m == int(want[3]) for m in modes)
    else:
        ok = 1 in modes and (2 in modes or 3 in modes)
    if "unmixed" in want:
        ok = ok and 0 in modes
    if "clipped" in want:
        ok = ok and any(clipped(bx) for bx in boxes)
    if "odd_x" in want:
        ok = ok and any(bx[2] % 8 and bx[3] % 8 and bx[3] > bx[2] for bx in boxes)
    return ok


def case_inputs(f, name, img=IMG, frames=T):
    """the seeded clip fp32 [B, 3, frames, img, img] and the labels of a fixture case"""
    try:
        import v1_downstream_synth as S
    except ImportError:  # (the generator imports this file as tests.v1_mixup_ref)
        from tests import v1_downstream_synth as S
    clip = S.synth_clip(dict(img_size=img), B, frames, int(f[name + ".clip_seed"]))
    return clip, torch.from_numpy(f[name + ".labels"].astype(np.int64))


def case_cfg(f, name):
    cfg = json.loads(str(f[name + ".cfg"]))
    if cfg.get("cutmix_minmax") is not None:
        cfg["cutmix_minmax"] = tuple(cfg["cutmix_minmax"])
    return cfg


def mix_clip(clip, mix_i, mix_f):
    """clip fp32 [B, 3, T, H, W] -> the mixed clip.  mode 0: the sample as it is; mode 1: own * lam + partner * one_minus_lam, both
    products rounded to fp32 before the sum; mode 2: the partner's pixels inside the box of every channel and frame; mode 3: the
    partner's pixels in the frames [yl, yh) and the rows [xl, xh) of every channel, whole rows."""
    out = clip.clone()
    for b in range(clip.shape[0]):
        partner, mode, yl, yh, xl, xh = (int(v) for v in mix_i[b])
        if mode == 1:
            out[b] = clip[b] * float(mix_f[b, 0]) + clip[partner] * float(mix_f[b, 1])
        elif mode == 2:
            out[b][..., yl:yh, xl:xh] = clip[partner][..., yl:yh, xl:xh]
        elif mode == 3:
            out[b][:, yl:yh, xl:xh, :] = clip[partner][:, yl:yh, xl:xh, :]
    return out


def mix_targets(labels, mix_i, mix_f, classes, smoothing):
    """soft targets fp32 [B, C]: rows of `off` with `on` at the label, own row * lam + partner's row * one_minus_lam; a mode-0 row
    takes lam = 1 and one_minus_lam = 0 and runs the same arithmetic"""
    off = smoothing / classes
    on = 1. - smoothing + off
    n = len(labels)
    y = torch.full((n, classes), off, dtype=torch.float32)
    y[torch.arange(n), labels.long()] = on
    out = torch.empty_like(y)
    for b in range(n):
        lam, oml = (float(mix_f[b, 0]), float(mix_f[b, 1])) if int(mix_i[b, 1]) else (1.0, 0.0)
        out[b] = y[b] * lam + y[int(mix_i[b, 0])] * oml
    return out


def sha256(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()
