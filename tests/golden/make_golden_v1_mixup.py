#!/usr/bin/env python3
"""Generate tests/golden/v1_mixup.npz by RUNNING THE REFERENCE's Mixup class (build container only).

v1/downstream/mixup.py is loaded read-only through the `_load` shim of make_golden_v1.py (it needs numpy and torch only) and its
``Mixup.__call__`` is run on seeded CPU clips (tests/v1_downstream_synth.synth_clip) and seeded labels, once per case of
tests/v1_mixup_ref.CASES.  What the run drew is RECORDED from the outside, by wrappers around the loaded module's
``cutmix_bbox_and_lam`` and ``mixup_target`` and the instance's ``_params_per_batch`` / ``_params_per_elem`` (no reference file is
edited or copied), and written down as the mix table of include/tvts_hip.h.  Stored per case: the seeds, the constructor
keywords, the table, the returned soft targets and the sha256 of the mixed clip's fp32 bytes -- a few KB in all.

The generator asserts what the tests rely on and tries further seeds until it holds (v1_mixup_ref.holds: which modes a case
draws, a box cut inside an 8-pixel group on both sides, a box clipped by the image border, an unmixed sample in elem mode), and that
the restatement tests/v1_mixup_ref.mix_clip / mix_targets reproduces the reference's bytes from the recorded table.

    python tests/golden/make_golden_v1_mixup.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TVTS_REFERENCE_V1", "/root/reference/v1")
sys.path.insert(0, ROOT)

from tests import v1_downstream_synth as S  # noqa: E402
from tests import v1_mixup_ref as M  # noqa: E402
from tests.golden.make_golden_v1 import _load, save  # noqa: E402


def run_case(ref, kwargs, classes, seed, clip_seed, label_seed):
    """one run of the reference class -> (mix_i, mix_f, mixed clip, targets, labels), the table read off the recorded draws"""
    B = M.B
    clip = S.synth_clip(dict(img_size=M.IMG), B, M.T, clip_seed)
    labels = torch.randint(0, classes, (B,), generator=torch.Generator().manual_seed(label_seed))
    fn = ref.Mixup(num_classes=classes, **kwargs)
    rec = dict(boxes=[], params=None, lam=None)
    orig_box, orig_target = ref.cutmix_bbox_and_lam, ref.mixup_target

    def box(*a, **k):
        out = orig_box(*a, **k)
        rec["boxes"].append(tuple(int(v) for v in out[0]))
        return out

    def target(t, nc, lam=1., smoothing=0.0, device="cuda"):
        rec["lam"] = lam
        return orig_target(t, nc, lam, smoothing, device)

    def params(orig):
        def f(*a):
            lam, cut = orig(*a)
            rec["params"] = (np.array(lam, copy=True), np.array(cut, copy=True))
            return lam, cut
        return f

    fn._params_per_batch, fn._params_per_elem = params(fn._params_per_batch), params(fn._params_per_elem)
    ref.cutmix_bbox_and_lam, ref.mixup_target = box, target
    try:
        np.random.seed(seed)
        mixed, targets = fn(clip.clone(), labels)
    finally:
        ref.cutmix_bbox_and_lam, ref.mixup_target = orig_box, orig_target

    mix_i = np.zeros((B, 6), dtype=np.int32)
    mix_i[:, 0] = B - 1 - np.arange(B)
    mix_f = np.empty((B, 2), dtype=np.float32)
    mix_f[:, 0], mix_f[:, 1] = 1.0, 0.0
    lam0, cut = rec["params"]
    boxes = iter(rec["boxes"])
    if kwargs["mode"] == "batch":
        if float(lam0) != 1.:
            lam = rec["lam"]                       # a Python / float64 scalar: 1 - lam in double, then to fp32
            mix_i[:, 1] = 2 if bool(cut) else 1
            if bool(cut):
                mix_i[:, 2:] = next(boxes)
            mix_f[:, 0], mix_f[:, 1] = np.float32(lam), np.float32(1. - lam)
    else:
        lam_t = rec["lam"].reshape(-1)            # fp32 tensor [B]: 1 - lam in fp32
        n = len(lam0)
        for i in range(n):
            if lam0[i] == 1.:
                continue
            rows = (i, B - 1 - i) if kwargs["mode"] == "pair" else (i,)
            bx = next(boxes) if cut[i] else (0, 0, 0, 0)
            for r in rows:
                # (pair mode pastes x[i][:, yl:yh, xl:xh] into 4-D clips: frames x rows, the table's mode 3)
                mix_i[r, 1], mix_i[r, 2:] = ((3 if kwargs["mode"] == "pair" else 2) if cut[i] else 1), bx
        for r in range(B):
            if mix_i[r, 1]:
                mix_f[r, 0], mix_f[r, 1] = lam_t[r].numpy(), (1. - lam_t)[r].numpy()
    assert next(boxes, None) is None
    return mix_i, mix_f, mixed, targets, labels, clip


def main():
    ref = _load("v1_downstream_mixup", os.path.join(REF, "downstream/mixup.py"))
    out = dict(names=np.array(list(M.CASES)), B=M.B, img=M.IMG, T=M.T)
    seen_odd = seen_clip = seen_unmixed = False
    for k, (name, (kwargs, classes, want)) in enumerate(M.CASES.items()):
        for seed in range(1000 * k, 1000 * k + 500):
            mix_i, mix_f, mixed, targets, labels, clip = run_case(ref, kwargs, classes, seed, 7000 + k, 7100 + k)
            if M.holds(want, mix_i):
                break
        else:
            raise SystemExit(f"{name}: no seed whose draw holds '{want}'")
        # the restatement, from the recorded table, is the reference's run bit for bit
        assert M.sha256(M.mix_clip(clip, mix_i, mix_f)) == M.sha256(mixed), name
        mine = M.mix_targets(labels, mix_i, mix_f, classes, kwargs["label_smoothing"])
        assert mine.numpy().tobytes() == targets.numpy().tobytes(), name
        assert targets.dtype == torch.float32 and mixed.dtype == torch.float32
        boxes = [mix_i[b, 2:] for b in range(M.B) if mix_i[b, 1] >= 2]
        seen_odd |= any(bx[2] % 8 and bx[3] % 8 for bx in boxes)
        seen_clip |= any(M.clipped(bx) for bx in boxes)
        seen_unmixed |= kwargs["mode"] == "elem" and 0 in mix_i[:, 1] and mix_i[:, 1].any()
        out.update({name + ".seed": seed, name + ".clip_seed": 7000 + k, name + ".labels": labels.numpy().astype(np.int32),
                    name + ".classes": classes, name + ".cfg": json.dumps(kwargs), name + ".mix_i": mix_i, name + ".mix_f": mix_f,
                    name + ".smoothing": float(kwargs["label_smoothing"]), name + ".targets": targets,
                    name + ".sha256": M.sha256(mixed)})
        print(f"{name}: seed {seed}\n{mix_i}\n{mix_f}")
    assert seen_odd and seen_clip and seen_unmixed
    save("v1_mixup", **out)


if __name__ == "__main__":
    main()
