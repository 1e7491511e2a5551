#!/usr/bin/env python3
"""Generate tests/golden/v1_input.npz by RUNNING THE REFERENCE's v1 pretraining transform under PIL (build container only).

v1/video_transforms/videoaug.py, video_transform.py and functional.py are loaded read-only through the `_load` / `_stub` shims of
make_golden_v1.py; ``cv2``, ``skimage`` and ``torchvision`` (import-time dependencies of those files only, none installed here) are
stubbed, ``torchvision.transforms.Compose`` by the three-line composer below.  No reference file is edited or copied; only data lands
in the fixture.  ``VideoTransform('train' / 'test', crop_size=32)`` -- so Resize(int(32 * 1.2) = 38) -- runs over five clips of T = 4
random-byte frames under a seeded ``random``; per clip the fixture stores
    src.<i>    the source frames, uint8 [T, Hs, Ws, 3]
    crop.<i>   the (top, left) the reference drew (mode 'train'; recorded from OUTSIDE by wrapping functional.crop_clip) or computed
               (mode 'test'), in resized coordinates
    u8.<i>     the uint8 resized and cropped frames [T, 32, 32, 3], made with the reference's own Resize and crop_clip calls
    f32.<i>    the final clip fp32 [T, 3, 32, 32] as base_dataset.py:119 permutes it
and `mode`, `seed`, `crop_size`, `resize`.

    python tests/golden/make_golden_v1_input.py
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TVTS_REFERENCE_V1", "/root/reference/v1")
sys.path.insert(0, ROOT)

from tests.golden.make_golden_v1 import _load, _stub, save  # noqa: E402

CROP, T, SEED = 32, 4, 20240521
# (Hs, Ws, mode): landscape at scale 1.18 | portrait | upscale | short side already 38 (the reference returns the clip untouched) |
# scale 4.2, long supports, odd width
CLIPS = ((45, 80, "train"), (80, 45, "train"), (20, 30, "test"), (38, 51, "train"), (160, 203, "train"))


class Compose:
    def __init__(self, ts): self.ts = ts
    def __call__(self, x):
        for t in self.ts: x = t(x)
        return x


def load_reference():
    _stub("cv2"); _stub("skimage"); _stub("skimage.transform")
    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms", Compose=Compose)
    pkg = _stub("video_transforms")
    pkg.__path__ = [os.path.join(REF, "video_transforms")]
    fn = _load("video_transforms.functional", os.path.join(REF, "video_transforms", "functional.py"))
    vt = _load("video_transforms.video_transform", os.path.join(REF, "video_transforms", "video_transform.py"))
    pkg.functional, pkg.video_transform = fn, vt
    va = _load("video_transforms.videoaug", os.path.join(REF, "video_transforms", "videoaug.py"))
    return fn, vt, va


def main():
    fn, vt, va = load_reference()
    tf = {m: va.VideoTransform(m, crop_size=CROP) for m in ("train", "test")}
    resize = vt.Resize(int(CROP * 1.2))
    out = {"n": len(CLIPS), "crop_size": CROP, "resize": int(CROP * 1.2), "seed": SEED, "T": T,
           "mode": np.array([m for _, _, m in CLIPS])}
    rng = np.random.RandomState(SEED)
    random.seed(SEED)
    orig_crop = fn.crop_clip
    for i, (hs, ws, mode) in enumerate(CLIPS):
        src = rng.randint(0, 256, size=(T, hs, ws, 3), dtype=np.uint8)
        seen = []

        def rec(clip, min_h, min_w, h, w):
            seen.append((int(min_h), int(min_w), int(h), int(w)))
            return orig_crop(clip, min_h, min_w, h, w)
        fn.crop_clip = rec
        try:
            clip = torch.from_numpy(src).permute(3, 0, 1, 2)  # [C, T, H, W]: what base_dataset.py:119 hands the transform
            final = tf[mode](clip).permute(1, 0, 2, 3).contiguous()
        finally:
            fn.crop_clip = orig_crop
        assert len(seen) == 1 and seen[0][2:] == (CROP, CROP), seen
        top, left = seen[0][:2]
        # the uint8 stage, by the reference's own calls on the same PIL images
        pil = vt.TensorToNumpy()(clip)
        u8 = np.stack([np.asarray(im) for im in fn.crop_clip(resize(pil), top, left, CROP, CROP)])
        assert u8.shape == (T, CROP, CROP, 3) and u8.dtype == np.uint8 and final.shape == (T, 3, CROP, CROP) and final.dtype == torch.float32
        mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
        again = (torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255) - mean[None, :, None, None]) / std[None, :, None, None]
        assert torch.equal(again, final), "the fp32 clip is not ClipToTensor + Normalize of the recorded uint8 frames"
        out.update({f"src.{i}": src, f"crop.{i}": np.array([top, left], dtype=np.int32), f"u8.{i}": u8, f"f32.{i}": final.numpy()})
        print(f"clip {i}: {hs} x {ws} {mode}: crop (top, left) = ({top}, {left})")
    save("v1_input", **out)


if __name__ == "__main__":
    main()
