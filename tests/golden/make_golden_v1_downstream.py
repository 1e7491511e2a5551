#!/usr/bin/env python3
"""Generate tests/golden/v1_downstream.npz by RUNNING THE REFERENCE's downstream classes (build container only).

/root/reference/v1/downstream/video_encoder_zero.py and video_encoder.py are imported read-only, with the same import shim for
timm as make_golden_v1.py (it is not installed here).  No reference file is edited or copied: weights and clips are regenerated
from seeds (tests/v1_downstream_synth.py), and only seeds, key lists and OUTPUTS (features, logits, ranks, recalls) are stored.

    python tests/golden/make_golden_v1_downstream.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TVTS_REFERENCE_V1", "/root/reference/v1")
sys.path.insert(0, ROOT)

from tests import v1_downstream_synth as S  # noqa: E402
from tests.golden.make_golden_v1 import _load, _stub, save  # noqa: E402

SEED_TINY, SEED_REAL, CLIP_TINY, CLIP_REAL, SEED_V2V = 51, 52, 53, 54, 55
CLASSES_TINY, CLASSES_REAL = 7, 5


def import_downstream():
    _stub("timm"); _stub("timm.models")
    _stub("timm.models.layers", StdConv2dSame=object, DropPath=torch.nn.Identity,
          to_2tuple=lambda x: x if isinstance(x, tuple) else (x, x), trunc_normal_=lambda t, std=1.0: t)
    zero = _load("v1_downstream_video_encoder_zero", os.path.join(REF, "downstream/video_encoder_zero.py"))
    full = _load("v1_downstream_video_encoder", os.path.join(REF, "downstream/video_encoder.py"))
    return zero, full


def run(zero, full, kw, seed, clip_seed, B, T, classes):
    sd = S.synth_state(kw, seed, classes)
    x = S.synth_clip(kw, B, T, clip_seed)
    with torch.no_grad():
        mz = zero.VisionTransformer(**kw).eval()
        keys_zero = list(mz.state_dict().keys())
        miss = mz.load_state_dict(sd, strict=False)  # as the script loads (run_class_zero.py:340): head.* has no home here
        assert not miss.missing_keys and sorted(miss.unexpected_keys) == ["head.bias", "head.weight"], miss
        feats = mz(x)
        mf = full.VisionTransformer(num_classes=classes, **kw).eval()
        keys_full = list(mf.state_dict().keys())
        mf.load_state_dict(sd, strict=True)
        assert list(sd.keys()) == keys_full and keys_full[:-2] == keys_zero
        logits = mf(x)
        assert torch.equal(mf.forward_features(x), feats)
    return dict(keys=np.array(keys_full), shapes=np.array([str(tuple(v.shape)) for v in mf.state_dict().values()]),
                feats=feats, logits=logits)


def main():
    torch.manual_seed(0)
    zero, full = import_downstream()
    tiny = run(zero, full, S.TINY, SEED_TINY, CLIP_TINY, B=3, T=8, classes=CLASSES_TINY)
    real = run(zero, full, S.REAL, SEED_REAL, CLIP_REAL, B=2, T=16, classes=CLASSES_REAL)
    feats, labels = S.v2v_data(SEED_V2V)
    ranks = S.script_ranks(S.sim_matrix_np(feats), labels.numpy())
    recalls = [100.0 * len(np.where(ranks < k)[0]) / len(ranks) for k in (1, 5, 10)]  # run_class_zero.py:407-409
    save("v1_downstream",
         keys=tiny["keys"], shapes_tiny=tiny["shapes"], shapes_real=real["shapes"], keys_real=real["keys"],
         seed_tiny=SEED_TINY, clip_seed_tiny=CLIP_TINY, B_tiny=3, T_tiny=8, classes_tiny=CLASSES_TINY,
         feats_tiny=tiny["feats"], logits_tiny=tiny["logits"],
         seed_real=SEED_REAL, clip_seed_real=CLIP_REAL, B_real=2, T_real=16, classes_real=CLASSES_REAL,
         feats_real=real["feats"], logits_real=real["logits"],
         v2v_seed=SEED_V2V, v2v_labels=labels.numpy(), v2v_ranks=ranks, v2v_recall=np.array(recalls))


if __name__ == "__main__":
    main()
