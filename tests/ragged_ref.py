"""Host restatement of the reference's v2 input chain on ragged uint8 clips (checker of tests/test_input_u8_ragged_*.py): per clip
PIL's nearest-neighbour Resize through its index tables (v2/video_transforms/functional.py:47-78), the crop, ClipToTensor + Normalize
(O.frames_to_video, pinned to the reference by tests/test_oracle_golden.py) and the zero frames base_dataset.py:128-130 puts behind
a short clip.  Held against the reference's own outputs (tests/golden/transform_resize.npz) by the CPU test."""
import numpy as np
import torch

from oracle import tvts_oracle as O
from tvts_amd.data_loader import transforms as TR


def resized_hw(hs, ws, size):
    return (hs, ws) if size is None else TR.resize_sizes(hs, ws, size)


def restate(clips, crops, size, img, T):
    """clips: B uint8 [T_b, Hs_b, Ws_b, 3]; crops: B x (top, left) in resized coordinates or None (centre) -> fp32 [B, T, 3, img, img]"""
    out = torch.zeros(len(clips), T, 3, img, img, dtype=torch.float32)
    for b, c in enumerate(clips):
        hs, ws = int(c.shape[1]), int(c.shape[2])
        nh, nw = resized_hw(hs, ws, size)
        yt, xt = np.array(TR.pil_nearest_table(hs, nh)), np.array(TR.pil_nearest_table(ws, nw))
        resized = c[:, yt][:, :, xt]
        crop = None if crops is None else torch.tensor([[int(crops[b][0]), int(crops[b][1])]])
        out[b, :c.shape[0]] = O.frames_to_video(resized.unsqueeze(0), img, crop)[0]
    return out


def im2col_rows(video, keep, patch):
    """fp32 [B, T, 3, img, img], keep [B, n] -> the gather's rows [(b, f, i), (ch, py, px)] rounded to bf16, as fp32"""
    B, T, _, img, _ = video.shape
    g, n, Kc = img // patch, keep.shape[1], 3 * patch * patch
    pix = video.reshape(B, T, 3, g, patch, g, patch).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, T, g * g, Kc)
    rows = torch.gather(pix, 2, keep.long()[:, None, :, None].expand(B, T, n, Kc)).reshape(-1, Kc)
    return rows.bfloat16().float()


def pack(clips, gaps):
    """byte offsets of the clips with gaps[b] pad bytes in front of clip b -> (offsets, total bytes)"""
    offs, at = [], 0
    for c, gap in zip(clips, gaps):
        at += gap
        offs.append(at)
        at += c.numel()
    return offs, at
