#!/usr/bin/env python3
"""What gradient clipping and the overflow guard cost the pretraining step: StepRunner(clip_grad=1.0, skip_nonfinite=True) beside
the plain StepRunner, same model, same resident batches, eager launches (the trainer's path), in ONE run.

Three workloads: `b16x192` and `b16x12` (ViT-B/16, 8 frames, 192 and 12 pairs per step: bench.py's batch and the reference's) and
`h14x48` (ViT-H/14, 16 frames, e4m3 operands and weight gradients, 48 pairs).  Per workload the legs alternate -- plain, guarded, plain, guarded, ...
for --rounds rounds (3) -- so that a drift of the box shows in both.  Every leg is a fresh child process (this file with --leg)
under its own time limit; the parent starts nothing further once a leg has failed or run out of time.  Per leg: --warmup untimed
steps, then --steps timed ones between two host-side synchronisations.  Prints every leg's ms per step, the median per kind and the
difference.

The expected cost is one more read of the gradient buffer (tvts_grad_sumsq: 4 B per trained element), three small launches (the
norm's two stages and the guard's counter kernel; on h14x48 the guarded scale update replaces the plain one).

usage: python tools/bench_train_guard.py [--workloads b16x192,b16x12,h14x48] [--rounds 3] [--steps 20] [--warmup 5] [--leg-timeout 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "b16x192": dict(arch="B_16", frames=8, batch=192, fp8_wgrad=False),
    "b16x12": dict(arch="B_16", frames=8, batch=12, fp8_wgrad=False),
    "h14x48": dict(arch="H_14", frames=16, batch=48, fp8_wgrad=True),
}


def leg(workload, kind, steps, warmup):
    """one leg in this (fresh) process -> one JSON line"""
    import torch

    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner
    w = WORKLOADS[workload]
    a = dict(A.ARCHS[w["arch"]])
    if w["frames"] > a["num_frames"]:
        a["num_frames"] = w["frames"]
    if w["fp8_wgrad"]:
        a.update(fp8=True, fp8_dgrad=True, fp8_wgrad=True)
    torch.cuda.set_device(0)
    model = TVTSv2Base(types.SimpleNamespace(local_rank=0, rank=0, world_size=1), arch=a, init_seed=0)
    groups = [[], [], [], []]
    for name, p in model.named_parameters():
        gi = A.param_group_of(name, a)
        if gi < 0:
            p.requires_grad = False
        else:
            groups[gi].append(p)
    opt = FusedHFAdamW([dict(params=groups[i], lr=A.GROUP_HPARAMS[i][0], weight_decay=A.GROUP_HPARAMS[i][1]) for i in range(4) if groups[i]],
                       model.store, model=model)
    kw = dict(clip_grad=1.0, skip_nonfinite=True) if kind == "guarded" else {}
    runner = StepRunner(model, opt, **kw)
    pool = [synth_batch(a, w["batch"], w["frames"], seed=i, caption_len=32, n_trans=4) for i in range(2)]
    model._fresh_shadows(); model._sync_requires_grad()
    dev = model.store.device
    pbs = [model.engine.prepare_batch(b) for b in pool]
    labels = [b["label"].reshape(-1).to(torch.int32).to(dev) for b in pool]
    for i in range(max(warmup, 1)):
        out = runner.run(pbs[i % 2], labels[i % 2])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = runner.run(pbs[i % 2], labels[i % 2])
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    trained = int((opt.chunk_group < 255).sum()) * 1024
    res = dict(workload=workload, kind=kind, ms_per_step=ms, steps=steps, warmup=warmup, trained_elements=trained,
               loss=float(out["loss1"]) + float(out["loss2"]), finite=bool(torch.isfinite(model.store.flat).all()))
    if kind == "guarded":
        res.update(grad_norm=float(out["grad_norm"]), skipped=int(runner.skipped.item()), step_dev=int(opt.step_dev.item()))
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workloads", default="b16x192,b16x12,h14x48")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=300.0, help="seconds per child process")
    ap.add_argument("--leg", nargs=2, metavar=("WORKLOAD", "KIND"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg[0], args.leg[1], args.steps, args.warmup)
    summary = {}
    for wl in [w for w in args.workloads.split(",") if w]:
        if wl not in WORKLOADS:
            ap.error(f"unknown workload {wl!r} (have {sorted(WORKLOADS)})")
        got = {"plain": [], "guarded": []}
        for rnd in range(args.rounds):
            for kind in ("plain", "guarded"):
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", wl, kind, "--steps", str(args.steps), "--warmup", str(args.warmup)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout, cwd=ROOT)
                except subprocess.TimeoutExpired:
                    raise SystemExit(f"[bench_train_guard] {wl} {kind} round {rnd + 1}: no result within {args.leg_timeout:.0f} s; stopping")
                line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")), None)
                if r.returncode != 0 or line is None:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"[bench_train_guard] {wl} {kind} round {rnd + 1} failed (exit status {r.returncode}); stopping")
                res = json.loads(line[4:])
                if not res["finite"] or (kind == "guarded" and res["skipped"] != 0):
                    raise SystemExit(f"[bench_train_guard] {wl} {kind} round {rnd + 1}: not a clean run {res}; stopping")
                got[kind].append(res)
                print(f"{wl:8s} round {rnd + 1} {kind:8s} {res['ms_per_step']:9.3f} ms/step" +
                      (f"   grad_norm {res['grad_norm']:.4g}" if kind == "guarded" else ""), flush=True)
        p, g = (statistics.median(r["ms_per_step"] for r in got[k]) for k in ("plain", "guarded"))
        spread = max(r["ms_per_step"] for r in got["plain"]) - min(r["ms_per_step"] for r in got["plain"])
        n = got["plain"][0]["trained_elements"]
        summary[wl] = dict(plain_ms=p, guarded_ms=g, diff_ms=g - p, diff_pct=100.0 * (g - p) / p, plain_spread_ms=spread,
                           trained_elements=n, extra_read_gb=4.0 * n / 1e9, rounds=args.rounds, steps=args.steps)
        print(f"{wl:8s} median plain {p:.3f} ms, guarded {g:.3f} ms: {g - p:+.3f} ms ({100.0 * (g - p) / p:+.2f} %), plain legs spread "
              f"{spread:.3f} ms; {n / 1e6:.1f} M trained elements, {4.0 * n / 1e9:.2f} GB more gradient read per step", flush=True)
    print("RESULT " + json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
