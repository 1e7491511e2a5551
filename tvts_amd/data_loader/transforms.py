"""Host-side halves of the input pipeline that the device kernels complete.

* the Resize of the reference's transform chain -- ``video_transform.Resize(int(crop_size * 1.2))`` with its default
  interpolation 'nearest' on the PIL images ``TensorToNumpy`` hands over (v2/video_transforms/videoaug.py:12,21,
  video_transform.py:171-188,656-664, functional.py:47-64,71-78) -- as INDEX TABLES: Pillow's nearest-neighbour resize reads
  source column ``int(xo)`` for ``xo = 0.5 * s, += s`` (s = src / dst, accumulated in double; Pillow's ImagingScaleAffine).
  The tables are built here exactly that way (a few hundred integers per clip shape, cached) and the gather kernel
  (tvts_patch_gather_u8_resized) reads the decoder's uint8 frames through them: resize, crop, /255, normalise and the tube-mask
  gather are one pass over the kept patches only.
* the Resize of the v1 chain, which is Pillow's 8-bit BILINEAR resample (``pil_bilinear_coeffs``): the fixed-point taps per axis,
  restated from Pillow's Resample.c; tvts_resize_crop_u8 applies them on the device.
* ``CaptionCache``: the tokenised-caption cache keyed by caption text in front of ``clip.tokenize``
  (v2/CLIP/clip/clip.py:197-237): BPE-encoding a caption costs ~100 us of Python per call and the YT-Temporal transcripts
  repeat from epoch to epoch; rows are stored as int32 [context] and stacked clip-major as the trainer needs them.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Dict, List, Sequence, Tuple

import torch


def resize_sizes(im_h: int, im_w: int, size: int) -> Tuple[int, int]:
    """(new_h, new_w) of functional.get_resize_sizes (:71-78); a picture whose smaller side already equals `size` is left alone
    (resize_clip :49-53)."""
    if (im_w <= im_h and im_w == size) or (im_h <= im_w and im_h == size):
        return im_h, im_w
    if im_w < im_h:
        return int(size * im_h / im_w), size
    return size, int(size * im_w / im_h)


def pil_nearest_table(n_in: int, n_out: int) -> List[int]:
    """source index of every output index of PIL.Image.resize(..., NEAREST) along one axis"""
    s = n_in / n_out
    xo = s * 0.5
    tab = []
    for _ in range(n_out):
        tab.append(min(int(xo), n_in - 1))
        xo += s
    return tab


_TABLES: Dict[tuple, tuple] = {}


def resize_tables(hs: int, ws: int, size: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """device int32 (ytab [H0], xtab [W0]) for decoder pictures of hs x ws resized with video_transform.Resize(size)"""
    key = (hs, ws, size, str(device))
    t = _TABLES.get(key)
    if t is None:
        h0, w0 = resize_sizes(hs, ws, size)
        t = _TABLES[key] = (torch.tensor(pil_nearest_table(hs, h0), dtype=torch.int32, device=device),
                            torch.tensor(pil_nearest_table(ws, w0), dtype=torch.int32, device=device))
    return t


PIL_PRECISION_BITS = 22  # Pillow's Resample.c: 8-bit samples, int32 accumulators, taps in 2^-22

_BILINEAR: Dict[tuple, tuple] = {}


def pil_bilinear_coeffs(n_in: int, n_out: int) -> Tuple[Tuple[int, Tuple[int, ...]], ...]:
    """Pillow's 8-bit BILINEAR resample along one axis of n_in -> n_out samples: per output index (first source index, int taps),
    cached per (n_in, n_out).  The v1 chain's Resize (v1/video_transforms/videoaug.py:10,18 -> video_transform.py:181-188 with the
    default 'nearest' -> functional.py:56-59, whose PIL branch maps everything but 'bilinear' to PIL.Image.BILINEAR) is this
    resample.  Restated from Resample.c `precompute_coeffs` with the bilinear filter (support 1.0) and `normalize_coeffs_8bpc`, in
    Python floats (C doubles), operation for operation:
        scale = n_in / n_out, filterscale = support = max(scale, 1)
        center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), n_in) - xmin
        w[x] = max(0, 1 - |(x + xmin - center + 0.5) / filterscale|), summed in tap order, each divided by the sum
        k[x] = int(0.5 + w[x] * 2^22)                                    (every bilinear weight is >= 0)
    One pass over a line is acc = 2^21 + sum px[xmin + i] * k[i], byte = clip8(acc >> 22); the horizontal pass runs first and the
    vertical pass reads its uint8 result.  An axis with n_in == n_out gets the identity (one tap of 2^22, beside zeros)."""
    key = (int(n_in), int(n_out))
    t = _BILINEAR.get(key)
    if t is not None:
        return t
    n_in, n_out = key
    if n_in < 1 or n_out < 1:
        raise ValueError(f"pil_bilinear_coeffs: sizes {n_in} -> {n_out}")
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    rows = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / filterscale)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append((xmin, tuple(int(0.5 + v * (1 << PIL_PRECISION_BITS)) for v in w)))
    t = _BILINEAR[key] = tuple(rows)
    return t


def centre_crop_offset(d: int) -> int:
    """(top or left) of the centre crop over a margin of d = side - crop pixels: CenterCrop's int(round(d / 2.))
    (v1/video_transforms/video_transform.py:454-455), round half to even -- the rule tvts_patch_gather_tube_u8 uses for crop = NULL"""
    return int(round(d / 2.))


class CaptionCache:
    """tokenizer(texts, truncate=...) -> int32 [len(texts), context] with the rows of already-seen captions served from a bounded
    LRU map.  `tokenizer` is the reference's ``clip.tokenize`` (or anything with its signature); rows are bit-identical to
    calling it directly because each caption is tokenised on its own there too (clip.py:222-235)."""

    def __init__(self, tokenizer: Callable, max_entries: int = 1 << 20):
        self.tokenizer, self.max_entries = tokenizer, max_entries
        self.rows: "OrderedDict[tuple, torch.Tensor]" = OrderedDict()
        self.hits = self.misses = 0

    def __call__(self, texts: Sequence[str], truncate: bool = False, **kw) -> torch.Tensor:
        if isinstance(texts, str):
            texts = [texts]
        miss = [t for t in dict.fromkeys(texts) if (t, truncate) not in self.rows]
        if miss:
            toks = self.tokenizer(miss, truncate=truncate, **kw) if (truncate or kw) else self.tokenizer(miss)
            for t, row in zip(miss, toks):
                self.rows[(t, truncate)] = row.clone()
            while len(self.rows) > self.max_entries:
                self.rows.popitem(last=False)
        self.misses += len(miss)
        self.hits += len(texts) - len(miss)
        out = []
        for t in texts:
            r = self.rows.get((t, truncate))
            if r is None:  # evicted by this very call (cache smaller than the batch)
                r = (self.tokenizer([t], truncate=truncate, **kw) if (truncate or kw) else self.tokenizer([t]))[0]
            else:
                self.rows.move_to_end((t, truncate))
            out.append(r)
        return torch.stack(out)
