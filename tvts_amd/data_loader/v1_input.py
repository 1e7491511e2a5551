"""The dataset side of the v1 pretraining step's uint8 input.

The reference's dataset builds ``VideoTransform(mode=split)`` (v1/video_transforms/videoaug.py:8-22) and ships fp32 clips.  Its chain is
``TensorToNumpy -> Resize(int(crop * 1.2)) -> RandomCrop | CenterCrop -> ClipToTensor -> Normalize``.  ``U8VideoTransform`` stands in
its place and does the ONE host-side part that is left, the draw of the crop: the frames stay uint8 at the decoder's size, Resize and
the crop run in ``tvts_resize_crop_u8``, ``ClipToTensor`` and ``Normalize`` inside ``tvts_patch_gather_tube_u8``.  ``collate_u8``
builds the batch dict ``EngineV1.prepare_batch`` takes (``video`` a list of ragged clips or one tensor, ``crop`` in resized
coordinates, ``resize``).

Not covered: ``TextImageDataset`` batches (torchvision ``RandomResizedCrop`` on a PIL image), the unused ``train_old`` /
``init_transform_dict`` chain, ColorJitter, clips shorter than the batch's T, decoding.
"""
from __future__ import annotations

import random
from typing import Sequence

import numpy as np
import torch

from .transforms import centre_crop_offset, resize_sizes


class U8VideoTransform:
    """``VideoTransform(mode, crop_size)`` without its pixel work.  Called with the clip the reference's transform gets -- a tensor
    [C, T, H, W] of byte values (base_dataset.py:119) -- it returns dict(video uint8 [T, H, W, 3], crop (top, left) in RESIZED
    coordinates, resize).  mode 'train': ``x1 = random.randint(0, new_w - crop)`` then ``y1 = random.randint(0, new_h - crop)`` from
    ``random``, the reference's two draws in its order (v1/video_transforms/video_transform.py:228-229), so the same ``random`` state
    gives the reference's crop; any other mode: CenterCrop's ``int(round((new_w - crop) / 2.))`` (:454-455)."""

    def __init__(self, mode: str = "train", crop_size: int = 224):
        self.mode, self.crop_size, self.resize = mode, int(crop_size), int(crop_size * 1.2)

    def __call__(self, clip: torch.Tensor) -> dict:
        if clip.dim() != 4 or clip.shape[0] != 3:
            raise ValueError(f"U8VideoTransform: expected a clip [3, T, H, W], got {tuple(clip.shape)}")
        # TensorToNumpy (video_transform.py:661-664): np.uint8 of the [T, H, W, C] values
        frames = torch.from_numpy(np.ascontiguousarray(np.uint8(clip.permute(1, 2, 3, 0).cpu().detach().numpy())))
        c = self.crop_size
        new_h, new_w = resize_sizes(int(frames.shape[1]), int(frames.shape[2]), self.resize)
        if c > new_w or c > new_h:  # (RandomCrop / CenterCrop raise the same way, :220-226)
            raise ValueError(f"U8VideoTransform: frames of {frames.shape[1]} x {frames.shape[2]} resize to {new_h} x {new_w}, below "
                             f"the crop of {c} x {c}")
        if self.mode == "train":
            x1 = random.randint(0, new_w - c)
            y1 = random.randint(0, new_h - c)
        else:
            x1, y1 = centre_crop_offset(new_w - c), centre_crop_offset(new_h - c)
        return dict(video=frames, crop=(y1, x1), resize=self.resize)


def collate_u8(samples: Sequence[dict]) -> dict:
    """samples of U8VideoTransform (plus any other per-sample fields) -> the batch dict of the resize-on-device wire format:
    video = the list of B clips [T, Hs_b, Ws_b, 3] (ONE tensor [B, T, Hs, Ws, 3] when every clip has the same shape), crop int32
    [B, 2] (top, left) in resized coordinates, resize.  Other fields: tensors of one shape are stacked, anything else is listed."""
    if not samples:
        raise ValueError("collate_u8: no samples")
    sizes = {int(s["resize"]) for s in samples}
    if len(sizes) != 1:
        raise ValueError(f"collate_u8: samples of different Resize sizes {sorted(sizes)}")
    clips = [s["video"] for s in samples]
    same = all(c.shape == clips[0].shape for c in clips)
    out = dict(video=torch.stack(clips) if same else clips, crop=torch.tensor([list(s["crop"]) for s in samples], dtype=torch.int32),
               resize=sizes.pop())
    for k in samples[0]:
        if k in out:
            continue
        vals = [s[k] for s in samples]
        stackable = all(torch.is_tensor(v) and v.shape == vals[0].shape for v in vals)
        out[k] = torch.stack(vals) if stackable else vals
    return out


def pack_clips(clips: Sequence[torch.Tensor], offsets: Sequence[int], out: torch.Tensor) -> torch.Tensor:
    """the ragged clips as bytes into `out` (uint8 1-D, e.g. page-locked), clip b at offsets[b]: the packed source buffer of
    tvts_resize_crop_u8"""
    for c, off in zip(clips, offsets):
        out[int(off):int(off) + c.numel()].copy_(c.reshape(-1))
    return out
