"""The per-sample augmentation of the v1 fine-tuning recipe behind RandAugment (random-resized crop, flip, random erasing), restated
for the tests from the semantics of the augmentation table (TEST INFRASTRUCTURE ONLY; numpy on the CPU):

    aug_i [B, 16] = (src, top, left, h, w, flip, emode, etop, eleft, eh, ew, key_lo, key_hi, 0, 0, 0)      include/tvts_hip.h

``aug_clip`` forms the taps in fp32 exactly as torch's interpolate does (scale, source index and weight are fp32 numbers) and
everything behind them -- normalisation, blend -- in float64; ``noise`` is the counter-based normal in uint64 / float64; and
the cases of tests/golden/v1_aug.npz, shared by its generator (tests/golden/make_golden_v1_aug.py, which runs the reference's
functions on them) and the tests (which regenerate the frames from the stored seeds)."""
from __future__ import annotations

import json

import numpy as np

IMG, T = 16, 2
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RAND_STREAM = 0xD1B54A32D192ED03
GOLDEN_GAMMA = 0x9E3779B97F4A7C15

# name -> (Augment keywords, Bs, H0, W0, want).  `want`: what the generator's seed search makes sure the case's draw holds
# (space-separated words of `holds`).  The reference's recipe values are ssv2.py:196-222: scale 0.08-1, ratio 0.75-1.3333.
CASES = {
    "recipe_ns2": (dict(hflip=0.0, reprob=0.25, remode="pixel", num_sample=2), 2, 37, 53, "erased unerased down interior"),
    "pixel_odd": (dict(hflip=0.5, reprob=0.9, remode="pixel", num_sample=1), 4, 37, 53, "oddbox flipped unflipped"),
    "const_flip": (dict(hflip=0.5, reprob=0.7, remode="const", num_sample=1), 4, 37, 53, "erased flipped unflipped up"),
    "rand_ns2": (dict(hflip=0.5, reprob=0.6, remode="rand", num_sample=2), 2, 23, 31, "erased down"),
    "fallback": (dict(hflip=0.0, reprob=0.0, remode="pixel", num_sample=1, scale=(0.5, 1.0)), 4, 12, 40, "fallback"),
    "small_src": (dict(hflip=0.5, reprob=0.5, remode="pixel", num_sample=2), 2, 9, 11, "up erased"),
}


def holds(want, aug_i, fallback, H0, W0, img=IMG):
    a = np.asarray(aug_i)
    tests = {
        "erased": (a[:, 6] > 0).any(), "unerased": (a[:, 6] == 0).any(),
        "flipped": (a[:, 5] == 1).any(), "unflipped": (a[:, 5] == 0).any(),
        "up": ((a[:, 3] < img) & (a[:, 4] < img)).any(), "down": ((a[:, 3] > img) & (a[:, 4] > img)).any(),
        "interior": ((a[:, 1] + a[:, 3] < H0) & (a[:, 2] + a[:, 4] < W0)).any(),   # the far edges lie inside the frame
        "oddbox": ((a[:, 6] > 0) & (a[:, 8] % 8 != 0) & ((a[:, 8] + a[:, 10]) % 8 != 0) & (a[:, 8] // 8 != (a[:, 8] + a[:, 10]) // 8)).any(),
        "fallback": bool(np.asarray(fallback).any()),
    }
    return all(tests[w] for w in want.split())


def case_frames(seed, Bs, H0, W0, frames=T):
    """seeded uint8 frames [Bs, frames, H0, W0, 3]: uniform noise, so that neighbouring pixels (and the ones just outside a crop) differ"""
    return np.random.RandomState(seed).randint(0, 256, (Bs, frames, H0, W0, 3)).astype(np.uint8)


def case_cfg(f, name):
    cfg = json.loads(str(f[name + ".cfg"]))
    for k in ("scale", "ratio"):
        if k in cfg:
            cfg[k] = tuple(cfg[k])
    return cfg


def key_of(row):
    return (int(row[11]) & 0xFFFFFFFF) | ((int(row[12]) & 0xFFFFFFFF) << 32)


# ---------------------------------------------------------------------------------------------- the noise rule
def noise(key, idx):
    """z(key, idx): r = splitmix64 finaliser of key + idx * 0x9E3779B97F4A7C15 (mod 2^64); u1 = ((r >> 32) + 1) 2^-32 in (0, 1],
    u2 = (r & 0xffffffff) 2^-32; z = sqrt(-2 ln u1) cos(2 pi u2), in float64"""
    with np.errstate(over="ignore"):
        z = np.uint64(key & 0xFFFFFFFFFFFFFFFF) + np.asarray(idx, dtype=np.uint64) * np.uint64(GOLDEN_GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u1 = ((z >> np.uint64(32)).astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = (z & np.uint64(0xFFFFFFFF)).astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


# ---------------------------------------------------------------------------------------------- crop, resize, flip
def taps(size, img, flip=False):
    """torch's bilinear source index for every output coordinate (align_corners=False), formed in fp32 as torch forms it
    -> (i0, i1 int64 [img], lambda1 float64 [img] holding fp32 values)"""
    o = np.arange(img)
    if flip:
        o = img - 1 - o
    scale = np.float32(size) / np.float32(img)
    s = np.maximum(scale * (o.astype(np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    assert s.dtype == np.float32
    i0 = np.minimum(s.astype(np.int64), size - 1)
    i1 = np.minimum(i0 + 1, size - 1)
    lam = (s - i0.astype(np.float32)).astype(np.float64)
    return i0, i1, lam


def normalise(u8, mean=MEAN, std=STD):
    """uint8 [..., 3] -> float64, with the fp32 mean / std the kernel is handed"""
    m, s = np.asarray(mean, dtype=np.float32).astype(np.float64), np.asarray(std, dtype=np.float32).astype(np.float64)
    return (u8.astype(np.float64) / 255.0 - m) / s


def resized(frames, row, img, mean=MEAN, std=STD):
    """one sample in front of the erase: frames uint8 [Bs, T, H0, W0, 3], row of aug_i -> float64 [3, T, img, img]"""
    src, top, left, h, w, flip = (int(v) for v in row[:6])
    crop = normalise(frames[src, :, top:top + h, left:left + w], mean, std)      # [T, h, w, 3]
    y0, y1, ly = taps(h, img)
    x0, x1, lx = taps(w, img, bool(flip))
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    a, b = crop[:, y0][:, :, x0], crop[:, y0][:, :, x1]
    c, d = crop[:, y1][:, :, x0], crop[:, y1][:, :, x1]
    out = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)     # [T, img, img, 3]
    return np.ascontiguousarray(out.transpose(3, 0, 1, 2))


def box_mask(row, img):
    """bool [img, img]: the erase box of a table row (empty for emode 0)"""
    m = np.zeros((img, img), dtype=bool)
    if int(row[6]):
        etop, eleft, eh, ew = (int(v) for v in row[7:11])
        m[etop:etop + eh, eleft:eleft + ew] = True
    return m


def erase_fill(row, frames_n, img):
    """the values inside the erase box, as a whole picture float64 [3, T, img, img] (to be taken under box_mask)"""
    emode, key = int(row[6]), key_of(row)
    f, c, y, x = np.meshgrid(np.arange(frames_n), np.arange(3), np.arange(img), np.arange(img), indexing="ij")
    if emode == 1:
        fill = np.zeros(f.shape)
    elif emode == 2:
        fill = noise(key + RAND_STREAM, f * 3 + c)
    else:
        fill = noise(key, ((f * 3 + c) * img + y) * img + x)
    return np.ascontiguousarray(fill.transpose(1, 0, 2, 3))


def aug_clip(frames, aug_i, img=IMG, mean=MEAN, std=STD, erase=True):
    """frames uint8 [Bs, T, H0, W0, 3], aug_i [B, 16] -> float64 [B, 3, T, img, img]: every sample cropped, resized, flipped and
    (erase=True) erased with the noise rule above"""
    frames, aug_i = np.asarray(frames), np.asarray(aug_i)
    out = np.empty((len(aug_i), 3, frames.shape[1], img, img))
    for b, row in enumerate(aug_i):
        out[b] = resized(frames, row, img, mean, std)
        if erase and int(row[6]):
            m = box_mask(row, img)
            out[b][:, :, m] = erase_fill(row, frames.shape[1], img)[:, :, m]
    return out
