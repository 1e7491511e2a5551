"""The dataset side of the v2 pretraining step's ragged uint8 input ("v2 ragged").

The reference's dataset builds ``VideoTransform(mode=split)`` (v2/video_transforms/videoaug.py:8-27) and ships fp32 clips, zero-padded
to ``num_frames`` behind the transform (v2/base/base_dataset.py:116-130).  Its chain is ``TensorToNumpy -> Resize(int(crop * 1.2)) ->
RandomCrop | CenterCrop -> ClipToTensor -> Normalize`` -- v1's chain, with PIL's nearest-neighbour Resize.  The host-side part that is
left is the same as v1's, the draw of the crop: ``RandomCrop`` draws ``x1`` then ``y1`` with ``random.randint``
(v2/video_transforms/video_transform.py:228-229), ``CenterCrop`` is ``int(round((side - crop) / 2.))`` (:454-455).  So
``U8VideoTransform`` of ``v1_input`` stands in the transform's place unchanged; the frames stay uint8 at the decoder's size and
length, and Resize, crop, ``ClipToTensor``, ``Normalize`` and the zero frames of a short clip run inside
``tvts_patch_gather_u8_ragged``.

``failed_clip`` is what the reference's ``except`` branch feeds its transform under ``"loading": "lax"``; ``collate_u8_v2`` builds the
batch dict ``Engine.prepare_batch`` takes (``video`` a list of ragged clips or one tensor, ``crop`` in resized coordinates,
``resize``, ``num_frames``).

Not covered: ColorJitter, bilinear Resize, decoding.
"""
from __future__ import annotations

from typing import Mapping, Sequence

import torch

from .v1_input import U8VideoTransform, collate_u8, pack_clips  # noqa: F401


def failed_clip(input_res: int) -> torch.Tensor:
    """the clip of a failed decode (base_dataset.py:122-123: ONE black input_res x input_res RGB picture) as the transform's
    TensorToNumpy sees it -> uint8 zeros [1, input_res, input_res, 3].  It is resized and cropped like any other clip (a black crop,
    (0 - mean) / std behind Normalize) and the frames behind it are the zero frames of a short clip."""
    res = int(input_res)
    if res < 1:
        raise ValueError(f"failed_clip: input_res {input_res}")
    return torch.zeros(1, res, res, 3, dtype=torch.uint8)


def collate_u8_v2(samples: Sequence[dict], video_params: Mapping) -> dict:
    """collate_u8 plus num_frames = video_params["num_frames"], the length base_dataset.py:128-130 pads every clip to.  video is
    ONE tensor [B, T, Hs, Ws, 3] only when every clip has the same shape AND the full length; otherwise the list of clips, so that
    a batch of equally short clips is still padded."""
    T = int(video_params["num_frames"])
    for b, s in enumerate(samples):
        if int(s["video"].shape[0]) > T:
            raise ValueError(f"collate_u8_v2: sample {b} has {int(s['video'].shape[0])} frames, video_params['num_frames'] is {T}")
    out = collate_u8(samples)
    if torch.is_tensor(out["video"]) and int(out["video"].shape[1]) < T:
        out["video"] = list(out["video"].unbind(0))
    out["num_frames"] = T
    return out
