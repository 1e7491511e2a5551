"""Reference side of the micro-batched pretraining step (tests/test_micro_batch_*.py), composed from the oracle's own pieces
(model_forward, sim_matrix, norm_softmax_loss, sorting_ce, param_groups); the oracle itself is not changed.

``unsplit_grads``      the oracle's step on the whole batch: losses and the gradient of every trainable tensor.
``schedule_grads``     the embedding-cache schedule restated: every chunk forward once for its embeddings (no graph), the InfoNCE
                       and dE over the cached rows of the WHOLE batch, every chunk forward again and backward with its rows of dE and
                       its share 1 / n of the sorting loss, all into the same .grad.
``chunk_local_grads``  plain accumulation, the negative control: one loss per chunk (its own negatives only), weight 1 / n.
``contiguous_split``   the WRONG text split (a contiguous slice of the transcript-major rows), the negative control of split_batch.
"""
import torch

from oracle import tvts_oracle as O

# (B, chunks, batch seed): the cases of the issue's table; synth_batch(T=2, caption_len=8) on small_arch, synth_params(seed=31)
CASES = ((4, 2, 40), (4, 2, 41), (6, 3, 42), (4, 4, 43))


def leaves_of(P, arch):
    _, frozen = O.param_groups(list(P.keys()), arch)
    return {k: t.detach().clone().requires_grad_(k not in frozen) for k, t in P.items()}


def grads_of(leaves):
    return {k: t.grad.detach().clone() for k, t in leaves.items() if t.grad is not None}


def unsplit_grads(P, batch, arch):
    """-> (loss1, loss2, {name: gradient}) of O.step_losses on the whole batch, frozen tensors left out"""
    leaves = leaves_of(P, arch)
    l1, l2, *_ = O.step_losses(leaves, batch, arch)
    (l1 + l2).backward()
    return float(l1.detach()), float(l2.detach()), grads_of(leaves)


def schedule_grads(P, chunks, arch):
    """chunks: the n batch dicts of split_batch, in clip order -> (loss1, loss2, grads) of the embedding-cache schedule"""
    n = len(chunks)
    leaves = leaves_of(P, arch)
    with torch.no_grad():  # pass 1: embeddings only
        embs = [O.model_forward(leaves, c, arch)[:2] for c in chunks]
    te = torch.cat([e[0] for e in embs]).requires_grad_(True)
    ve = torch.cat([e[1] for e in embs]).requires_grad_(True)
    loss1 = O.norm_softmax_loss(O.sim_matrix(ve, te))
    d_te, d_ve = torch.autograd.grad(loss1, (te, ve))
    loss2, lo = 0.0, 0
    for c in chunks:  # pass 2: each chunk again, its rows of dE and 1 / n of its sorting loss
        t, v, pred = O.model_forward(leaves, c, arch)
        b = t.shape[0]
        assert torch.equal(t.detach(), te[lo:lo + b].detach()) and torch.equal(v.detach(), ve[lo:lo + b].detach())
        total = (t * d_te[lo:lo + b]).sum() + (v * d_ve[lo:lo + b]).sum()
        if pred is not None:
            l2 = O.sorting_ce(pred, c["label"]) / n
            total = total + l2
            loss2 += float(l2.detach())
        total.backward()
        lo += b
    return float(loss1.detach()), loss2, grads_of(leaves)


def chunk_local_grads(P, chunks, arch):
    """one loss per chunk, gradients summed at weight 1 / n -> (mean loss1, mean loss2, grads)"""
    n = len(chunks)
    leaves = leaves_of(P, arch)
    s1 = s2 = 0.0
    for c in chunks:
        l1, l2, *_ = O.step_losses(leaves, c, arch)
        ((l1 + l2) / n).backward()
        s1, s2 = s1 + float(l1.detach()) / n, s2 + float(l2.detach()) / n
    return s1, s2, grads_of(leaves)


def contiguous_split(data, n):
    """split_batch with the text rows sliced contiguously: pairs the wrong captions whenever NT > 1"""
    B = data["video"].shape[0]
    b, NT = B // n, data["text"].shape[0] // B
    out = []
    for k in range(n):
        d = {key: (val[k * b:(k + 1) * b] if torch.is_tensor(val) and val.shape[0] == B else val) for key, val in data.items()}
        d["text"] = data["text"][k * b * NT:(k + 1) * b * NT]
        out.append(d)
    return out


def flat(grads, keys=None):
    return torch.cat([grads[k].double().flatten() for k in (keys or sorted(grads))])


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))
