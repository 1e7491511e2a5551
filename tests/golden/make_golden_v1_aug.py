#!/usr/bin/env python3
"""Generate tests/golden/v1_aug.npz by RUNNING THE REFERENCE's per-sample augmentation (build container only).

v1/downstream/video_transforms.py, random_erasing.py and ssv2.py are loaded read-only through the `_load` / `_stub` shims of
make_golden_v1.py -- ``torchvision``, ``rand_augment``, ``functional``, ``decord`` and ``volume_transforms`` are stubbed (none of
them is reached by the functions run here; torchvision is not installed in the build container), random_erasing.py is loaded as it
is.  Per sample of every case of tests/v1_aug_ref.CASES, in the collate order of ``--num_sample``, the generator runs what
ssv2.py:191-225 runs on a decoded clip: ``tensor_normalize`` on seeded uint8 frames, ``spatial_sampling`` (which calls
``random_resized_crop`` and, for a data set that flips, ``horizontal_flip(0.5, ...)``) and ``RandomErasing(reprob, mode=remode,
max_count=recount, num_splits=recount, device="cpu")``, under seeded ``random`` / ``np.random`` / ``torch``.

What the run drew is RECORDED from the outside (no reference file is edited or copied): wrappers around the loaded module's
``_get_param_spatial_crop`` (the crop; a counter on ``np.random.uniform`` tells the ten failed tries of the central fallback),
``horizontal_flip`` (the flip, read off the returned frames) and ``_get_pixels`` (the erase mode and the box size); the erase box is
located from the difference to the clone taken in front of the erase.  Stored per case: the seeds, the constructor keywords, the
table (noise keys as tvts_amd's Augment numbers them), the fallback flags and the fp32 result clips.

The generator tries further seeds until the draw of a case holds what the tests rely on (v1_aug_ref.holds), and asserts that
the whole fixture holds an upscaling, a downscaling and a fallback crop, a crop whose far edges are interior to the frame, an erase box cut
inside an 8-pixel group on both sides and an unerased sample, and that tests/v1_aug_ref.aug_clip reproduces the reference's clips
outside the erase boxes to 2e-6.

    python tests/golden/make_golden_v1_aug.py
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TVTS_REFERENCE_V1", "/root/reference/v1")
sys.path.insert(0, ROOT)

from tests import v1_aug_ref as A  # noqa: E402
from tests.golden.make_golden_v1 import _load, _stub, save  # noqa: E402

EMODE = {(False, False): 1, (False, True): 2, (True, False): 3}  # (per_pixel, rand_color) of _get_pixels -> the table's emode


def load_reference():
    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms")
    tv.transforms.functional = _stub("torchvision.transforms.functional")
    _stub("rand_augment", rand_augment_transform=None)
    _stub("functional")
    _stub("decord", VideoReader=None, cpu=None)
    _stub("volume_transforms")
    d = os.path.join(REF, "downstream")
    re_ = _load("random_erasing", os.path.join(d, "random_erasing.py"))
    vt = _load("video_transforms", os.path.join(d, "video_transforms.py"))
    ss = _load("ssv2", os.path.join(d, "ssv2.py"))
    return vt, re_, ss


def run_case(ref, kwargs, Bs, H0, W0, seed, frame_seed):
    """one run of the reference's chain over Bs clips x num_sample views -> (aug_i, fallback flags, fp32 clips [B, 3, T, img, img])"""
    vt, re_, ss = ref
    from tvts_amd.downstream.finetune_v1 import splitmix64
    frames = A.case_frames(frame_seed, Bs, H0, W0)
    ns, img = kwargs["num_sample"], A.IMG
    scale, ratio = list(kwargs.get("scale", (0.08, 1.0))), list(kwargs.get("ratio", (0.75, 1.3333)))
    rec = {}
    orig_crop, orig_flip, orig_pixels, orig_uniform = vt._get_param_spatial_crop, vt.horizontal_flip, re_._get_pixels, np.random.uniform
    count = dict(uniform=0)

    def uniform(*a, **k):
        count["uniform"] += 1
        return orig_uniform(*a, **k)

    def crop(sc, ra, height, width, *a, **k):
        n0 = count["uniform"]
        i, j, h, w = orig_crop(sc, ra, height, width, *a, **k)
        rec["crop"], rec["tries"] = (int(i), int(j), int(h), int(w)), count["uniform"] - n0
        return i, j, h, w

    def flip(prob, images, boxes=None):
        out, bx = orig_flip(prob, images, boxes)
        rec["flip"] = int(not torch.equal(out, images))
        return out, bx

    def pixels(per_pixel, rand_color, patch_size, **k):
        rec["emode"], rec["patch"] = EMODE[(bool(per_pixel), bool(rand_color))], tuple(int(v) for v in patch_size)
        return orig_pixels(per_pixel, rand_color, patch_size, **k)

    vt._get_param_spatial_crop, vt.horizontal_flip, re_._get_pixels, np.random.uniform = crop, flip, pixels, uniform
    aug_i = np.zeros((Bs * ns, 16), dtype=np.int32)
    fallback = np.zeros(Bs * ns, dtype=bool)
    clips = []
    try:
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        key0 = splitmix64(seed)
        for b in range(Bs * ns):
            rec.clear()
            s = b // ns
            buf = ss.tensor_normalize(torch.from_numpy(frames[s]), [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])  # T H W C
            buf = buf.permute(3, 0, 1, 2)
            buf = ss.spatial_sampling(buf, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=img,
                                      random_horizontal_flip=kwargs["hflip"] > 0, inverse_uniform_sampling=False,
                                      aspect_ratio=ratio, scale=scale, motion_shift=False)
            before = buf.clone()
            if kwargs["reprob"] > 0:  # ssv2.py:38-40: rand_erase = reprob > 0
                erase = re_.RandomErasing(kwargs["reprob"], mode=kwargs["remode"], max_count=1, num_splits=1, device="cpu")
                buf = erase(buf.permute(1, 0, 2, 3)).permute(1, 0, 2, 3)
            row = aug_i[b]
            row[0], row[1:5], row[5] = s, rec["crop"], rec.get("flip", 0)
            i, j, h, w = rec["crop"]
            fallback[b] = rec["tries"] == 10 and (i, j) == ((H0 - h) // 2, (W0 - w) // 2)
            if "emode" in rec:
                _, eh, ew = rec["patch"]
                changed = (buf != before).any(dim=0).any(dim=0)  # [img, img]
                ys, xs = np.nonzero(changed.numpy())
                # (pixel / rand noise differs from the picture everywhere; a const box can hold a pixel that was 0 already, not a whole edge)
                assert ys.max() - ys.min() + 1 == eh and xs.max() - xs.min() + 1 == ew, (rec, ys.min(), ys.max(), xs.min(), xs.max())
                row[6], row[7:11] = rec["emode"], (ys.min(), xs.min(), eh, ew)
            else:
                assert torch.equal(buf, before)
            key = (key0 + b) & ((1 << 64) - 1)
            row[11:13] = np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint32).view(np.int32)
            assert buf.dtype == torch.float32 and tuple(buf.shape) == (3, A.T, img, img)
            clips.append(buf.contiguous())
    finally:
        vt._get_param_spatial_crop, vt.horizontal_flip, re_._get_pixels, np.random.uniform = orig_crop, orig_flip, orig_pixels, orig_uniform
    return aug_i, fallback, torch.stack(clips).numpy(), frames


def main():
    ref = load_reference()
    out = dict(names=np.array(list(A.CASES)), img=A.IMG, T=A.T)
    seen = dict.fromkeys(("up", "down", "fallback", "interior", "oddbox", "unerased"), False)
    worst = 0.0
    for k, (name, (kwargs, Bs, H0, W0, want)) in enumerate(A.CASES.items()):
        for seed in range(1000 * k, 1000 * k + 500):
            aug_i, fallback, clips, frames = run_case(ref, kwargs, Bs, H0, W0, seed, 8000 + k)
            if A.holds(want, aug_i, fallback, H0, W0):
                break
        else:
            raise SystemExit(f"{name}: no seed whose draw holds '{want}'")
        for w in seen:
            seen[w] |= A.holds(w, aug_i, fallback, H0, W0)
        for src, t, l, h, w in aug_i[:, :5]:   # an interior far edge shows a clamp to the frame only if the pixels just outside differ
            if t + h < H0 and l + w < W0:
                assert (frames[src, :, t + h, l:l + w] != frames[src, :, t + h - 1, l:l + w]).any(), name
                assert (frames[src, :, t:t + h, l + w] != frames[src, :, t:t + h, l + w - 1]).any(), name
        mine = A.aug_clip(frames, aug_i, erase=False)
        for b, row in enumerate(aug_i):
            m = A.box_mask(row, A.IMG)
            worst = max(worst, float(np.abs(mine[b] - clips[b])[:, :, ~m].max()))
            if int(row[6]) == 1:
                assert not clips[b][:, :, m].any(), name
        out.update({name + ".seed": seed, name + ".frame_seed": 8000 + k, name + ".cfg": json.dumps(kwargs),
                    name + ".shape": np.array([Bs, H0, W0]), name + ".aug_i": aug_i, name + ".fallback": fallback, name + ".clips": clips})
        print(f"{name}: seed {seed}\n{aug_i[:, :11]}\nfallback {fallback}")
    print(f"restatement against the reference outside the erase boxes: max |d| = {worst:.3e}")
    assert all(seen.values()), seen
    assert worst <= 2e-6, worst
    save("v1_aug", **out)


if __name__ == "__main__":
    main()
