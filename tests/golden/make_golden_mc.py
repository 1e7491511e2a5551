#!/usr/bin/env python3
"""Generate tests/golden/mc_b16.npz by RUNNING THE REFERENCE's SSv2 multiple-choice model (container only).

The real v2/downstream/model_TVTSv2_ViT_B_16_mc.py is loaded the way make_golden.gen_downstream loads its sibling (import shims,
synthetic parameters from the oracle), fed B = 3 clips with C = 8 ragged candidate captions each, and scored with the arithmetic of
zero_ssv2_mc_TVTSv2_ViT_B_16.py:80-88.  Only arrays are stored: the caption ids, the labels, the reference's embeddings, logits and
top-1 / top-5 counts, and the seeds from which the test side regenerates the parameters and the video.

    python tests/golden/make_golden_mc.py
"""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, O, _load, _stub, downstream_arch, import_reference, save  # noqa: E402

B, T, C = 3, 4, 8
# caption lengths (SOT and EOT included): both sides of the 16 / 32 / 48 / 64-row tiles of the packed attention, the context's 77,
# the shortest caption there is, and a few in between; shuffled over the [C * B] rows below
LENGTHS = [2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 76, 77, 5, 9, 12, 20, 24, 28, 40, 56, 70]
PARAM_SEED, VIDEO_SEED = 0, 31
MARGIN = 1.0  # twice the GPU test's gate on |logits - golden|


def mc_captions(arch, seed):
    """[C * B, context] int32 ids built like O.synth_batch builds captions (SOT = vocab - 2 first, EOT = vocab - 1 last, zeros
    behind), with the ragged LENGTHS in an order drawn from `seed`."""
    g = torch.Generator().manual_seed(seed)
    lens = [LENGTHS[i] for i in torch.randperm(len(LENGTHS), generator=g).tolist()]
    text = torch.zeros(C * B, arch["context"], dtype=torch.int32)
    for r, n in enumerate(lens):
        text[r, 0] = arch["vocab"] - 2
        if n > 2:
            text[r, 1:n - 1] = torch.randint(1, arch["vocab"] - 408, (n - 2,), generator=g, dtype=torch.int32)
        text[r, n - 1] = arch["vocab"] - 1
    return text


def script_scores(te, ve, label):
    """What the script computes per batch (zero_ssv2_mc_TVTSv2_ViT_B_16.py:80-91), restated: both sides divided by their plain
    norms, 100 x the batched product of clip b with its own C options, and the number of clips whose label is among the k
    highest logits for k = 1, 5 (torch.topk, as the script's accuracy())."""
    v = (ve / ve.norm(dim=-1, keepdim=True)).unsqueeze(1)            # [B, 1, E]
    t = te.transpose(0, 1)
    t = t / t.norm(dim=-1, keepdim=True)                             # [B, C, E]
    logits = 100.0 * torch.bmm(v, t.transpose(1, 2)).squeeze(1)      # [B, C]
    top = logits.topk(5, dim=1).indices
    hit = top == label.view(-1, 1)
    return logits, [float(hit[:, :k].sum()) for k in (1, 5)]


def decisive_gap(logits, label):
    """smallest distance between a clip's label logit and any other logit of that clip: with it above MARGIN, a perturbation of
    every logit by less than MARGIN / 2 changes neither the top-1 nor the top-5 membership of any clip"""
    own = logits.gather(1, label.view(-1, 1))
    d = (logits - own).abs()
    d.scatter_(1, label.view(-1, 1), float("inf"))
    return d.min(dim=1)[0]


def gen_mc():
    assert len(LENGTHS) == C * B
    import_reference()
    if "downstream" not in sys.modules:
        _stub("downstream")
    dm = _load("downstream.model_TVTSv2_ViT_B_16_mc", os.path.join(REF, "downstream/model_TVTSv2_ViT_B_16_mc.py"))
    arch = downstream_arch("B_16")
    m = dm.TVTSv2_B_16(load_checkpoint="")
    P = O.synth_params(arch, seed=PARAM_SEED)
    assert list(m.state_dict().keys()) == list(P.keys()), "the _mc state dict is not the downstream one"
    m.load_state_dict(P, strict=True)
    m.eval()
    video = O.synth_batch(O.ARCHS["B_16"], B=B, T=T, seed=VIDEO_SEED, n_trans=1)["video"]
    keep = torch.arange(196).unsqueeze(0).expand(B, -1)
    for text_seed in range(32, 64):  # the first caption / label draw whose decisions all clear the margin
        text = mc_captions(arch, text_seed)
        with torch.no_grad():
            te, ve = m({"text": text, "video": video, "keep_ind": keep}, return_embeds=True)
        assert te.shape == (C, B, arch["embed"]) and ve.shape == (B, arch["embed"])
        for label_seed in range(16):
            label = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(label_seed))
            logits, (acc1, acc5) = script_scores(te.clone(), ve.clone(), label)
            gap = decisive_gap(logits.clone(), label)
            if bool((gap > MARGIN).all()) and 0 < acc5 and acc1 < B:
                break
        else:
            continue
        break
    else:
        raise AssertionError("no seed leaves every clip's decisions clear of the margin")
    assert bool((decisive_gap(logits.clone(), label) > MARGIN).all())
    print("lengths", (text.argmax(-1) + 1).tolist(), "label", label.tolist(), "gap", gap.tolist(), "acc", acc1, acc5)
    save("mc_b16", text=text, label=label.to(torch.int64), te=te, ve=ve, logits=logits, acc1=acc1, acc5=acc5, seed=PARAM_SEED,
         batch_seed=VIDEO_SEED, text_seed=text_seed, label_seed=label_seed, B=B, T=T, C=C)


if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_mc()
