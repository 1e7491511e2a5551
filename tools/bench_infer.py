#!/usr/bin/env python3
"""The forward-only video encoder against the training-path forward (GPU dev tool): clips/s and peak allocated GB of
`compute_video` under no_grad (Engine.video_forward) and of `encode_video` (Engine.encode_video) at the downstream geometry
(12 unmasked frames), B/16 at 32 / 128 clips and H/14 at 8 / 32 clips; and the full-frame SPACE attention site alone, the
streaming kernel + CLS-query pair (what calls with lse2 run) against the forward-only fused kernel.  One JSON line each.
  --attn-only: the attention lines only (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

CONFIGS = [("B_16", 196, 32), ("B_16", 196, 128), ("H_14", 256, 8), ("H_14", 256, 32)]


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def attention(K):
    """one SPACE site of each geometry at 128 / 32 clips (B/16 heads 12 dh 64, H/14 heads 16 dh 80), T = 12"""
    for name, B, n, heads, dh in (("B_16", 128, 196, 12, 64), ("H_14", 32, 256, 16, 80)):
        T, W = 12, heads * dh
        S = 1 + T * n
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B * S, 3 * W, generator=g, device="cuda").bfloat16()
        out = torch.empty(B * S, W, dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(B * heads * T * (dh + 2), device="cuda")
        res = {}
        for form, fused in (("streaming + CLS pass", False), ("fused full-frame", True)):
            res[form] = timed(lambda: K.attn_fwd_divided("space", qkv, out, None, ws, B=B, heads=heads, S=S, T=T, n=n,
                                                         head_dim=dh, fused=fused), 20)
        print(json.dumps({"what": f"SPACE attention forward-only, {name} T=12 n={n}", "clips": B,
                          **{k + " us": 1e6 * v for k, v in res.items()}}), flush=True)
        del qkv, out, ws
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    from tvts_amd import hip as K
    attention(K)
    if args.attn_only:
        return
    import importlib
    models = {}
    for name, n, B in CONFIGS:
        m = models.get(name)
        if m is None:
            for k in list(models):
                del models[k]
            torch.cuda.empty_cache()
            mod = importlib.import_module(f"tvts_amd.downstream.model_TVTSv2_ViT_{name}")
            m = models[name] = getattr(mod, f"TVTSv2_{name}")(load_checkpoint=None, pretrained=False)
        g = torch.Generator().manual_seed(1)
        v = torch.randn(B, 12, 3, 224, 224, generator=g).cuda()
        keep = torch.arange(n).unsqueeze(0)
        line = {"what": f"video embeddings, {name} T=12 n={n}", "clips": B}
        for form, fn in (("training forward", lambda: m.compute_video(v, keep.expand(B, -1))),
                         ("encode_video", lambda: m.encode_video(v, keep))):
            eng = m.engine
            eng.buf.clear(); eng._back.clear(); eng._seen.clear(); eng._inf.clear()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            try:
                with torch.no_grad():
                    dt = timed(fn, args.iters)
                line[form + " clips/s"] = B / dt
                line[form + " peak GB"] = torch.cuda.max_memory_allocated() / 1e9
            except torch.cuda.OutOfMemoryError:
                line[form + " clips/s"] = None
                line[form + " peak GB"] = "out of memory"
        print(json.dumps(line), flush=True)
        del v


if __name__ == "__main__":
    main()
