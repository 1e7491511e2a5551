"""Seeded inputs and numpy restatements shared by tests/golden/make_golden_v1_eval.py (which runs the reference's test-view
slicing and its compute_video / merge on them) and the v1 evaluation tests (which regenerate them): the fixture stores seeds,
lists and results only.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import hashlib

import numpy as np

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHORT, TSRC, SEG, CROP = 32, 8, 2, 3
SIZES = ((32, 48), (48, 32))       # (H0, W0) of the two recorded source clips: a wide one and a tall one
FRAME_SEEDS = (9101, 9102)
VIEWS = [(ck, cp) for ck in range(SEG) for cp in range(CROP)]  # ssv2.py:77-83: chunk-major, then crop
N_VIDEOS, N_CLASSES = 7, 11
DUP_VIDEO, SHORT_VIDEO = 2, 5      # the video with a repeated (chunk, split) line / the one with a missing view


def source_clip(seed: int, H0: int, W0: int, frames: int = TSRC) -> np.ndarray:
    """uint8 [frames, H0, W0, 3]: what the patched loadvideo_decord returns"""
    return np.random.RandomState(seed).randint(0, 256, (frames, H0, W0, 3)).astype(np.uint8)


def normalise(clip_u8: np.ndarray) -> np.ndarray:
    """ClipToTensor + Normalize (volume_transforms.py:42-67, functional.py:81-97) on uint8 [T, H, W, 3] -> fp32 [3, T, H, W]:
    fp32(u) / 255 in fp32, minus the fp32 mean, divided by the fp32 std, every operation rounded to fp32"""
    x = clip_u8.astype(np.float32).transpose(3, 0, 1, 2) / np.float32(255)
    m = np.asarray(MEAN, dtype=np.float32)[:, None, None, None]
    s = np.asarray(STD, dtype=np.float32)[:, None, None, None]
    return ((x - m) / s).astype(np.float32)


def slice_view(clip_u8: np.ndarray, row, T: int, img: int) -> np.ndarray:
    """the uint8 view a table row (src, t0, tstep, top, left, ...) names, cut from ITS source clip [Tsrc, H0, W0, 3]"""
    _, t0, tstep, top, left = (int(v) for v in row[:5])
    return np.ascontiguousarray(clip_u8[t0::tstep][:T, top:top + img, left:left + img])


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sample(clip_f32: np.ndarray) -> np.ndarray:
    """the stored slice of a returned clip [3, T, H, W]"""
    return clip_f32[:, :, ::5, ::7].copy()


# ---------------------------------------------------------------------------------------------- view logits for the merge
def eval_lines(seed: int):
    """-> (labels int [N_VIDEOS], lines): lines is a list of (video, chunk, split, logits fp32 [N_CLASSES]) in file order.  Every
    video has its SEG x CROP views except SHORT_VIDEO, whose last view is missing; DUP_VIDEO has a second line for its view (1, 0)
    with other logits, behind the first (merge keeps the first)."""
    rs = np.random.RandomState(seed)
    labels = rs.randint(0, N_CLASSES, N_VIDEOS)
    logits = rs.standard_normal((N_VIDEOS, SEG * CROP, N_CLASSES)).astype(np.float32)
    logits[np.arange(N_VIDEOS), :, labels] += np.float32(0.45)
    dup = rs.standard_normal(N_CLASSES).astype(np.float32) * np.float32(4.0)
    lines = []
    for v in range(N_VIDEOS):
        for k, (ck, cp) in enumerate(VIEWS):
            if v == SHORT_VIDEO and k == len(VIEWS) - 1:
                continue
            lines.append((v, ck, cp, logits[v, k]))
        if v == DUP_VIDEO:
            lines.append((v, 1, 0, dup))
    return labels, lines


def kept_views(lines):
    """merge's rule (engine_for_finetuning.py:247-255): per video the logits of the FIRST line of every (chunk, split), in file order"""
    feats, pos = {}, {}
    for v, ck, cp, x in lines:
        if (ck, cp) in pos.setdefault(v, set()):
            continue
        pos[v].add((ck, cp))
        feats.setdefault(v, []).append((ck * CROP + cp, x))
    return feats


def video_id(v: int) -> str:
    return "vid%03d" % v


def write_file(path, labels, lines):
    """the reference's file format (engine_for_finetuning.py:202-222): a first line merge skips, then `id [logits] label chunk split`"""
    with open(path, "w") as f:
        f.write("0.0, 0.0\n")
        for v, ck, cp, x in lines:
            f.write("{} {} {} {} {}\n".format(video_id(v), str(x.tolist()), str(int(labels[v])), str(int(ck)), str(int(cp))))


def class_ranks_np(x: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """the definition of tvts_class_ranks: #{c : x_c > x_label} + #{c < label : x_c == x_label}"""
    x, labels = np.asarray(x), np.asarray(labels)
    xl = x[np.arange(x.shape[0]), labels][:, None]
    below = np.arange(x.shape[1])[None, :] < labels[:, None]
    with np.errstate(invalid="ignore"):
        return ((x > xl) | ((x == xl) & below)).sum(axis=1).astype(np.int32)


def view_sum_np(view_logits: np.ndarray, seen: np.ndarray):
    """the definition of tvts_view_sum: fp32 adds from +0 in the order v = 0 .. V - 1 over the seen views -> (sum, count)"""
    N, V, C = view_logits.shape
    out = np.zeros((N, C), dtype=np.float32)
    for v in range(V):
        m = seen[:, v] != 0
        out[m] = (out[m] + view_logits[m, v]).astype(np.float32)
    return out, (seen != 0).sum(axis=1).astype(np.int32)
