#!/usr/bin/env python3
"""The packed text tower of the training step (arch["text_packed"]) against the padded one (GPU dev tool).

ViT-B/16, 8 frames, 4 captions per clip, at 192 pairs and at the reference's 12 pairs.  Both models hold the same weights and run
the SAME ragged batch, resident on the device, alternated in one process; the padded model runs the code of a tree without this
option (the option changes no padded path), so its time is the yardstick.  One JSON line each:
  - the whole step (forward, losses, backward, AdamW), padded against packed;
  - the text tower alone (forward + backward, in line on the main stream), padded against packed;
  - token rows kept (M) over token rows padded (N * longest caption);
  - the attention site alone: tvts_attn_bwd_packed against the FULL causal backward on the same captions (and the forwards);
  - the host side: pack_captions against the padded path's token_sort.
The caption lengths are a STAND-IN: EOT included, uniform in [8, 77], fixed seed.  Nobody has measured the length distribution of
the YT-Temporal transcripts or the WebVid captions for this repository; every line carries that note.  --lo / --hi move the range
(--lo 77: every caption fills the context and packing saves no row)."""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def median_alternated(fns, reps, warmup=3):
    """{name: median seconds per call}, the calls alternated in one process, each timed with its own synchronisation"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def ragged_batch(a, pairs, frames, lo, hi, seed):
    from tvts_amd.data_loader import synth_batch
    batch = synth_batch(a, pairs, frames, seed=seed, caption_len=a["context"], n_trans=a["n_trans"])
    N = batch["text"].shape[0]
    lens = torch.randint(lo, hi + 1, (N,), generator=torch.Generator().manual_seed(seed + 1))
    col = torch.arange(a["context"])[None, :]
    batch["text"][col >= lens[:, None]] = 0
    batch["text"][torch.arange(N), lens - 1] = a["vocab"] - 1
    return batch, lens


def make(a, flags):
    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner
    a = dict(a, **flags)
    m = TVTSv2Base(types.SimpleNamespace(local_rank=0, rank=0, world_size=1), arch=a, init_seed=0)
    groups = [[], [], [], []]
    for name, p in m.named_parameters():
        gi = A.param_group_of(name, a)
        if gi < 0:
            p.requires_grad = False
        else:
            groups[gi].append(p)
    hp = A.GROUP_HPARAMS
    opt = FusedHFAdamW([dict(params=groups[i], lr=hp[i][0], weight_decay=hp[i][1]) for i in range(4) if groups[i]], m.store, model=m)
    m._fresh_shadows(); m._sync_requires_grad()
    return m, StepRunner(m, opt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[192, 12])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--lo", type=int, default=8)
    ap.add_argument("--hi", type=int, default=77)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--text-side", choices=("on", "off"), default="on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_packed.py measures on the GPU: no device found")
    from tvts_amd import arch as A
    from tvts_amd import hip as K
    note = (f"caption lengths: STAND-IN, EOT included, uniform in [{args.lo}, {args.hi}], fixed seed -- no real transcript length "
            f"distribution has been measured")
    base = dict(A.ARCHS["B_16"], text_side=args.text_side == "on")
    for pairs in args.pairs:
        batch, lens = ragged_batch(base, pairs, args.frames, args.lo, args.hi, seed=0)
        N, L = lens.numel(), int(lens.max())
        (mp, rp), (mk, rk) = make(base, {}), make(base, dict(text_packed=True))
        pbp, pbk = mp.engine.prepare_batch(batch), mk.engine.prepare_batch(batch)
        lab = batch["label"].reshape(-1).to(torch.int32).cuda()
        M = pbk["M"]
        head = {"pairs": pairs, "frames": args.frames, "captions": N, "note": note}
        print(json.dumps({"what": "token rows of the text tower", **head, "rows kept (M)": M, "rows padded (N * L)": N * L,
                          "longest caption": L, "rows kept / rows padded": M / (N * L)}), flush=True)
        med = median_alternated({"padded": lambda: rp.run(pbp, lab), "packed": lambda: rk.run(pbk, lab)}, args.reps)
        print(json.dumps({"what": "whole step (forward, losses, backward, AdamW), resident batch, text_side " + args.text_side, **head,
                          "padded ms (median)": 1e3 * med["padded"], "packed ms (median)": 1e3 * med["packed"],
                          "packed / padded": med["packed"] / med["padded"], "reps": args.reps}), flush=True)

        def tower(m, pb):
            e, E = m.engine, m.arch["embed"]
            dt = torch.randn(N, E, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda") * 1e-3
            pk = pb if pb.get("seq_start") is not None else None

            def run():
                e.text_forward(pb["ids"], pb["eot_rows"], N, pb["L"], eot_index=pb.get("eot_index"), packed=pk)
                e.text_backward(dt, pb["ids"], pb["eot_rows"], N, pb["L"], tok_sort=pb["tok_sort"], packed=pk)
            return run
        side = (mp.engine.text_side, mk.engine.text_side)
        mp.engine.text_side = mk.engine.text_side = False  # the tower alone: in line, on the timed stream
        med = median_alternated({"padded": tower(mp, pbp), "packed": tower(mk, pbk)}, args.reps)
        mp.engine.text_side, mk.engine.text_side = side
        print(json.dumps({"what": "text tower alone (forward + backward, gradients accumulated)", **head,
                          "padded ms (median)": 1e3 * med["padded"], "packed ms (median)": 1e3 * med["packed"],
                          "packed / padded": med["packed"] / med["padded"], "reps": args.reps}), flush=True)
        del mp, rp, mk, rk, pbp
        torch.cuda.empty_cache()

        # the attention site alone, on the same captions (random operands; the forwards fill O and lse2)
        heads = base["text_heads"]
        W = heads * 64
        ss, ml = pbk["seq_start"], pbk["max_len"]
        g = torch.Generator(device="cuda").manual_seed(2)
        bf = torch.bfloat16
        qp, dop = torch.randn(M, 3 * W, generator=g, device="cuda").to(bf), torch.randn(M, W, generator=g, device="cuda").to(bf)
        qr, dor = torch.randn(N * L, 3 * W, generator=g, device="cuda").to(bf), torch.randn(N * L, W, generator=g, device="cuda").to(bf)
        op, orr = torch.empty(M, W, dtype=bf, device="cuda"), torch.empty(N * L, W, dtype=bf, device="cuda")
        lp, lr = torch.empty(M, heads, device="cuda"), torch.empty(N * L, heads, device="cuda")
        dp, dr = torch.empty_like(lp), torch.empty_like(lr)
        gp, gr = torch.empty(M, 3 * W, dtype=bf, device="cuda"), torch.empty(N * L, 3 * W, dtype=bf, device="cuda")
        med = median_alternated({
            "fwd full": lambda: K.attn_fwd("full", qr, orr, lr, B=N, heads=heads, S=L, causal=True),
            "fwd packed": lambda: K.attn_fwd_packed(qp, ss, op, N=N, heads=heads, max_len=ml, lse2=lp),
            "bwd full": lambda: K.attn_bwd("full", qr, dor, orr, lr, dr, gr, B=N, heads=heads, S=L, causal=True),
            "bwd packed": lambda: K.attn_bwd_packed(qp, ss, dop, op, lp, dp, gp, N=N, heads=heads, max_len=ml)}, max(args.reps, 20))
        print(json.dumps({"what": f"text attention site, {heads} heads, lse2 stored (launch + sync, median)", **head,
                          "FULL causal S=%d" % L: {"fwd us": 1e6 * med["fwd full"], "bwd us": 1e6 * med["bwd full"]},
                          "packed": {"fwd us": 1e6 * med["fwd packed"], "bwd us": 1e6 * med["bwd packed"]},
                          "packed / FULL, backward": med["bwd packed"] / med["bwd full"]}), flush=True)
        del qp, dop, qr, dor, op, orr, lp, lr, dp, dr, gp, gr, pbk
        torch.cuda.empty_cache()

        ids_cpu = batch["text"].to(torch.int64)
        t0 = time.perf_counter()
        for _ in range(10):
            K.pack_captions(ids_cpu, base["context"])
        t1 = time.perf_counter()
        for _ in range(10):
            K.token_sort(ids_cpu[:, :L])
        t2 = time.perf_counter()
        print(json.dumps({"what": "host side of prepare_batch's text part (mean of 10)", **head,
                          "pack_captions ms (both sort plans included)": 1e2 * (t1 - t0), "padded path: token_sort ms": 1e2 * (t2 - t1)}),
              flush=True)


if __name__ == "__main__":
    main()
