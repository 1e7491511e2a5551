"""Seeded inputs shared by tests/golden/make_golden_v1_downstream.py (which runs the reference classes on them) and the v1
inference tests (which regenerate them): the fixture stores seeds and outputs only.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np
import torch

from oracle import tvts_v1_oracle as V

TINY = dict(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_frames=8, tubelet_size=2)
REAL = dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, num_frames=16, tubelet_size=2)
PREFIX = "video_model."


def oracle_arch(kw) -> dict:
    """the v1 oracle's arch dict of a downstream constructor's keywords; the text tower and the sort head are cut to nothing --
    synth_params seeds every tensor by its NAME, so the video tower's values do not depend on them"""
    return dict(V.ARCH, image=kw["img_size"], patch=kw["patch_size"], width=kw["embed_dim"], layers=kw["depth"],
                heads=kw["num_heads"], num_frames=kw["num_frames"], tubelet=kw["tubelet_size"], text_layers=0, vocab=2, max_pos=2,
                text_width=64, text_ffn=64, sort_depth=0, sort_width=64)


def synth_state(kw, seed: int, num_classes: int = 0) -> "dict[str, torch.Tensor]":
    """a state dict of the downstream class (its own key names, its own order): the video tower of V.synth_params(seed), plus
    head.* seeded by name the same way"""
    P = V.synth_params(oracle_arch(kw), seed=seed)
    sd = {k[len(PREFIX):]: v for k, v in P.items() if k.startswith(PREFIX)}
    if num_classes > 0:
        W = kw["embed_dim"]
        g = torch.Generator().manual_seed(V._key_seed(seed, "head.weight"))
        sd["head.weight"] = torch.randn(num_classes, W, generator=g) * W ** -0.5 * 0.7
        g = torch.Generator().manual_seed(V._key_seed(seed, "head.bias"))
        sd["head.bias"] = 0.02 * torch.randn(num_classes, generator=g)
    return sd


def synth_clip(kw, B: int, T: int, seed: int) -> torch.Tensor:
    """fp32 [B, 3, T, H, W], the layout the downstream classes take"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, T, kw["img_size"], kw["img_size"], generator=g, dtype=torch.float32)


def v2v_data(seed: int, N: int = 40, D: int = 128, classes: int = 6):
    """features fp32 [N, D] with a class-dependent mean (so that retrieval is neither trivial nor hopeless) and labels int64 [N];
    the LAST class has exactly one member (its query's best same-label score is its own -1000)"""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, max(classes - 1, 1), (N,), generator=g)
    if N > 1 and classes > 1:
        labels[int(torch.randint(0, N, (1,), generator=g))] = classes - 1
    centres = torch.randn(classes, D, generator=g)
    feats = 0.15 * centres[labels] + torch.randn(N, D, generator=g)
    return feats, labels


def sim_matrix_np(feats: torch.Tensor, eps: float = 1e-8) -> np.ndarray:
    """the script's sim_matrix(feats, feats) with its self-mask applied (v1/downstream/run_class_zero.py:348-356,385-387)"""
    n = feats.norm(dim=1)[:, None]
    fn = feats / torch.max(n, eps * torch.ones_like(n))
    s = torch.mm(fn, fn.t()).numpy().copy()
    np.fill_diagonal(s, -1000)
    return s


def script_ranks(scores: np.ndarray, labels) -> np.ndarray:
    """restatement of the script's loop (:389-404) on self-masked scores: position of the first same-label video among the first
    10 of argsort(-scores), 1e20 if there is none (fewer than 10 videos: among all of them)"""
    lab = np.asarray(labels)
    N = scores.shape[0]
    ix = np.argsort(-scores, axis=1)
    ranks = np.full(N, 1e20)
    for q in range(N):
        for r in range(min(10, N)):
            if lab[ix[q, r]] == lab[q]:
                ranks[q] = r
                break
    return ranks


def defined_ranks(scores: np.ndarray, labels) -> np.ndarray:
    """the rank definition of tvts_v2v_ranks on self-masked scores: #{j : label differs and score > best same-label score}"""
    lab = np.asarray(labels)
    same = lab[None, :] == lab[:, None]
    best = np.where(same, scores, -np.inf).max(axis=1)
    return ((~same) & (scores > best[:, None])).sum(axis=1).astype(np.float64)
