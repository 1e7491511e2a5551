#!/usr/bin/env python3
"""The v1 step with its DistilBERT tower over packed captions (arch["text_unpadded"], DESIGN.md 8b "v1") against the padded one
(GPU dev tool, modelled on tools/bench_text_packed.py).

v1 (tubelet ViT-B/16 + DistilBERT), 4 frames, 4 captions per clip, at 256 clips and at the reference's 24 clips per GPU
(v1/configs/dist-yt-pt.json).  Both models hold the same weights and run the SAME ragged batch, resident on the device, alternated in
one process; the padded model runs the code of a tree without this option (the option changes no padded path), so its time is the
yardstick.  One JSON line each:
  - token rows kept (M) over token rows padded (N * longest caption);
  - the whole step (forward, losses, backward, AdamW), padded against unpadded;
  - the text tower alone (forward + backward, dropout 0.1 as the reference trains), padded against unpadded;
  - the host side: pack_captions(lens=...) against the padded path's token_sort.
The caption lengths are a STAND-IN: [CLS] and [SEP] included, uniform in [4, 50] (the trainer's tokenizer call truncates at 50), fixed
seed.  Nobody has measured the length distribution of the YT-Temporal transcripts for this repository; every line carries that note.
--lo moves the lower end (the crossover probe [lo, 50]; --lo 50: every caption has 50 tokens and packing saves no row)."""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tools.bench_text_packed import median_alternated  # noqa: E402


def ragged_batch(a, clips, frames, lo, hi, seed):
    from tvts_amd.data_loader import synth_batch_v1
    batch = synth_batch_v1(a, clips, frames, seed=seed, caption_len=hi, n_trans=a["n_trans"])
    ids = batch["text"]["input_ids"]
    N = ids.shape[0]
    lens = torch.randint(lo, hi + 1, (N,), generator=torch.Generator().manual_seed(seed + 1))
    mask = (torch.arange(hi)[None, :] < lens[:, None]).to(torch.int64)
    ids *= mask
    ids[torch.arange(N), lens - 1] = 102  # [SEP]
    batch["text"]["attention_mask"] = mask
    return batch, lens


def make(a, flags):
    from tvts_amd.model.model_dist_TVTS import TVTS
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner
    m = TVTS(types.SimpleNamespace(local_rank=0, rank=0, world_size=1), arch=dict(a, **flags), init_seed=0)
    # one parameter group, lr 1e-4, weight_decay 0 (v1/configs/dist-yt-pt.json)
    opt = FusedHFAdamW([dict(params=list(m.parameters()), lr=1e-4, weight_decay=0.0)], m.store, model=m)
    m._fresh_shadows(); m._sync_requires_grad()
    return m, StepRunner(m, opt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[256, 24])
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--lo", type=int, default=4)
    ap.add_argument("--hi", type=int, default=50)
    ap.add_argument("--reps", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_packed_v1.py measures on the GPU: no device found")
    from tvts_amd import arch as A
    from tvts_amd import hip as K
    note = (f"caption lengths: STAND-IN, [CLS] / [SEP] included, uniform in [{args.lo}, {args.hi}], fixed seed -- no real transcript "
            f"length distribution has been measured")
    base = dict(A.ARCH_V1)
    for clips in args.clips:
        batch, lens = ragged_batch(base, clips, args.frames, args.lo, args.hi, seed=0)
        N, L = lens.numel(), int(lens.max())
        (mp, rp), (mk, rk) = make(base, {}), make(base, dict(text_unpadded=True))
        pbp, pbk = mp.engine.prepare_batch(batch), mk.engine.prepare_batch(batch)
        lab = batch["label"].reshape(-1).to(torch.int32).cuda()
        M = pbk["M"]
        head = {"clips": clips, "frames": args.frames, "captions": N, "note": note}
        print(json.dumps({"what": "token rows of the v1 text tower", **head, "rows kept (M)": M, "rows padded (N * L)": N * L,
                          "longest caption": L, "rows kept / rows padded": M / (N * L)}), flush=True)
        med = median_alternated({"padded": lambda: rp.run(pbp, lab), "unpadded": lambda: rk.run(pbk, lab)}, args.reps)
        print(json.dumps({"what": "whole v1 step (forward, losses, backward, AdamW), resident batch", **head,
                          "padded ms (median)": 1e3 * med["padded"], "unpadded ms (median)": 1e3 * med["unpadded"],
                          "unpadded / padded": med["unpadded"] / med["padded"], "reps": args.reps}), flush=True)

        def tower(m, pb):
            e, E = m.engine, m.arch["embed"]
            dt = torch.randn(N, E, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda") * 1e-3
            pk = pb.get("txt_pk")

            def run():
                e.text_forward_v1(pb["ids"], pb["kv_len"], pb["txt_cls_rows"], N, pb["L"], pk=pk)
                e.text_backward_v1(dt, pb["ids"], pb["kv_len"], pb["txt_cls_rows"], N, pb["L"], tok_sort=pb["tok_sort"], pk=pk)
            return run
        med = median_alternated({"padded": tower(mp, pbp), "unpadded": tower(mk, pbk)}, args.reps)
        print(json.dumps({"what": "v1 text tower alone (forward + backward, dropout 0.1, gradients accumulated)", **head,
                          "padded ms (median)": 1e3 * med["padded"], "unpadded ms (median)": 1e3 * med["unpadded"],
                          "unpadded / padded": med["unpadded"] / med["padded"], "reps": args.reps}), flush=True)
        del mp, rp, mk, rk, pbp, pbk
        torch.cuda.empty_cache()

        ids_cpu, mask = batch["text"]["input_ids"], batch["text"]["attention_mask"]
        t0 = time.perf_counter()
        for _ in range(10):
            K.pack_captions(ids_cpu, base["max_pos"], lens=mask.sum(-1))
        t1 = time.perf_counter()
        for _ in range(10):
            K.token_sort(ids_cpu[:, :L])
        t2 = time.perf_counter()
        print(json.dumps({"what": "host side of prepare_batch's text part (mean of 10)", **head,
                          "pack_captions ms (both sort plans included)": 1e2 * (t1 - t0), "padded path: token_sort ms": 1e2 * (t2 - t1)}),
              flush=True)


if __name__ == "__main__":
    main()
