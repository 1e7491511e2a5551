"""The device-side arithmetic of the zero-shot scripts (v2/downstream/zero_recognition_TVTSv2_ViT_B_16.py:67-108):
prompt-ensemble class embeddings and `100 * normalise(video) @ W` logits on HIP kernels, top-k accuracy."""
from __future__ import annotations

import torch

from .. import hip as K


def _l2norm(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous().float()
    xn, inv = torch.empty_like(x), torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    K.l2norm_rows(x, xn, inv, 0.0)  # the scripts divide by the plain norm (no eps clamp)
    return xn


@torch.no_grad()
def class_embedding(model, prompt_ids: torch.Tensor, n_patches: int) -> torch.Tensor:
    """One class: the tokenised prompts [P, ctx] go through the text tower (beside dummy frames, as the script does),
    are normalised, averaged and normalised again (:70-80)."""
    dev = model.store.device
    P = prompt_ids.shape[0]
    data = {"text": prompt_ids, "video": torch.zeros(P, 3, model.arch["image"], model.arch["image"], device=dev),
            "keep_ind": torch.arange(n_patches).unsqueeze(0)}
    emb, _ = model(data, return_embeds=True)
    mean = _l2norm(emb).mean(dim=0, keepdim=True)
    return _l2norm(mean)[0]


@torch.no_grad()
def class_embeddings(model, prompt_ids_per_class, packed=False) -> torch.Tensor:
    """[C, E]: class_embedding of every class (a list of [P_c, ctx] prompt-id tensors), text only -- the prompts of all
    classes through model.encode_text, without dummy frames.  Classes whose captions end at the same token position share a
    pass: the caption length L of a pass is the longest caption in it, and a class keeps the L of its own pass in
    class_embedding, so both evaluate the same arithmetic.
    packed=True: the prompts of ALL classes go through one packed variable-length pass instead (encode_text(packed=True))."""
    if packed:
        emb = model.encode_text(torch.cat([p.to("cpu", torch.int64) for p in prompt_ids_per_class]), packed=True)
        out, o = [], 0
        for p in prompt_ids_per_class:
            mean = _l2norm(emb[o:o + p.shape[0]]).mean(dim=0, keepdim=True)
            out.append(_l2norm(mean)[0])
            o += p.shape[0]
        return torch.stack(out)
    ends = [int(p.argmax(-1).max()) for p in prompt_ids_per_class]
    out = [None] * len(prompt_ids_per_class)
    for end in sorted(set(ends)):
        idx = [c for c, e in enumerate(ends) if e == end]
        ids = torch.cat([prompt_ids_per_class[c][:, :end + 1].to("cpu", torch.int64) for c in idx])
        emb = model.encode_text(ids)
        o = 0
        for c in idx:
            P = prompt_ids_per_class[c].shape[0]
            mean = _l2norm(emb[o:o + P]).mean(dim=0, keepdim=True)
            out[c] = _l2norm(mean)[0]
            o += P
    return torch.stack(out)


@torch.no_grad()
def class_logits(video_emb: torch.Tensor, zeroshot_weights: torch.Tensor) -> torch.Tensor:
    """100 * normalise(video_emb) @ zeroshot_weights (:99-100); zeroshot_weights is [E, n_classes]."""
    v = _l2norm(video_emb)
    w = zeroshot_weights.contiguous().float()
    E, C = w.shape
    out = torch.empty(v.shape[0], C, dtype=torch.float32, device=v.device)
    K.gemm_small(v, w, out, M=v.shape[0], N=C, K=E, sa=(E, 1), sb=(C, 1), alpha=100.0)
    return out


@torch.no_grad()
def mc_logits(text_features: torch.Tensor, video_features: torch.Tensor) -> torch.Tensor:
    """The multiple-choice scoring of zero_ssv2_mc_TVTSv2_ViT_B_16.py:80-88: text_features [C, B, E] (option-major, as the _mc
    models return them), video_features [B, E] -> logits [B, C] = 100 * cos(video b, option c of clip b), one HIP launch."""
    t = text_features.contiguous().float()
    v = video_features.contiguous().float()
    if t.dim() != 3 or v.dim() != 2 or t.shape[1:] != v.shape:
        raise ValueError(f"mc_logits: text {tuple(t.shape)} must be [C, B, E] for video {tuple(v.shape)} [B, E]")
    out = torch.empty(v.shape[0], t.shape[0], dtype=torch.float32, device=v.device)
    K.mc_logits(t, v, out)
    return out


def accuracy(logits: torch.Tensor, target: torch.Tensor, topk=(1,)):
    """Per k: the number of samples whose target class is among the k highest logits (what the scripts accumulate)."""
    own = logits.gather(1, target.view(-1, 1).long())
    higher = (logits > own).sum(dim=1)  # classes scoring above the target
    return [float((higher < k).sum()) for k in topk]


# ---- v1's published zero-shot protocol: video-to-video retrieval by label (v1/downstream/run_class_zero.py:344-413)
@torch.no_grad()
def v2v_ranks(feats: torch.Tensor, labels: torch.Tensor, chunk: int = 2048) -> torch.Tensor:
    """ranks [N] (fp32, exact integers) of the script's protocol: features [N, D] are normalised as its sim_matrix does (norms
    clamped at 1e-8, :348-356), every video queries all the others (its own score read as -1000, :385-387), and
    ranks[q] = the number of other-label videos scoring above the best same-label one -- `ranks < k` is the script's hit among the
    first k of argsort(-scores) for k <= 10 (:389-404).  The similarities are formed `chunk` query rows at a time
    (tvts_gemm_small_f32 into a [chunk, N] workspace, then tvts_v2v_ranks): the [N, N] matrix never exists."""
    x = feats.contiguous().float()
    if x.dim() != 2 or x.shape[0] == 0 or labels.numel() != x.shape[0] or chunk < 1:
        raise ValueError(f"v2v_ranks: features {tuple(x.shape)} need one label each, got {tuple(labels.shape)}")
    N, D = x.shape
    lab = labels.reshape(-1).to(x.device, torch.int32).contiguous()
    xn, inv = torch.empty_like(x), torch.empty(N, dtype=torch.float32, device=x.device)
    K.l2norm_rows(x, xn, inv, 1e-8)
    chunk = min(int(chunk), N)
    sims = torch.empty(chunk, N, dtype=torch.float32, device=x.device)
    ranks = torch.empty(N, dtype=torch.float32, device=x.device)
    for q0 in range(0, N, chunk):
        nq = min(chunk, N - q0)
        K.gemm_small(xn[q0:], xn, sims, M=nq, N=N, K=D, sa=(D, 1), sb=(1, D))
        K.v2v_ranks(sims[:nq], q0, lab, ranks[q0:q0 + nq])
    return ranks


def recall_at(ranks, ks=(1, 5, 10)):
    """R@k in percent, as the script prints them (:407-409): 100 * #{ranks < k} / N"""
    r = torch.as_tensor(ranks).reshape(-1)
    return [100.0 * float((r < k).sum()) / r.numel() for k in ks]
