#!/usr/bin/env python3
"""Activation recomputation of the video tower (arch["recompute"], DESIGN.md "Activation recomputation"): what the modes cost in
time and what they save in memory (GPU dev tool).

Configurations: ViT-B/16 with 8 frames at 192 pairs, ViT-H/14 with 16 frames at 48 and at 96 pairs; 4 captions of 32 tokens per
clip, one resident synthetic batch, eager steps (forward, losses, backward, fused AdamW).  Per configuration and mode ("none",
"mlp", "block") ONE JSON line: ms per step (median and mean of the timed steps), pairs/s, Engine.workspace_bytes(),
torch.cuda.max_memory_allocated(), the card's memory and recompute_count.

Every mode runs in a FRESH CHILD PROCESS (its peak is its own; an allocator that has held another mode's buffers tells nothing)
under a time limit of its own; the parent never opens the device and stops at the first child that fails.

    python tools/bench_recompute.py                          # the three configurations, three modes each
    python tools/bench_recompute.py --only H_14:16:96        # one configuration
    python tools/bench_recompute.py --batch 160 --mode block # H/14, 16 frames, ONE mode at a larger batch

--batch N is checked BEFORE anything of that size runs: the peak of the same mode at 96 pairs (measured first, or read from
--lines FILE, the output of an earlier run) is scaled linearly to N pairs -- an over-estimate, the parameters and optimizer state
do not grow with the batch -- and N is refused unless that leaves at least 10 % of the card free.  --batch auto takes the largest
multiple of 8 that passes.  A second bound holds beside the memory rule: the largest tensor of the step (the MLP's [M, 4W] bf16
pair) stays below 2^31 bytes -- no step with a larger tensor has ever run through these kernels, and a benchmark is not the place
to find out.  The tool never looks for the limit by running into an out-of-memory error."""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (("B_16", 8, 192), ("H_14", 16, 48), ("H_14", 16, 96))
MODES = ("none", "mlp", "block")
FREE_FRACTION = 0.10


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_recompute.py measures on the GPU: no device found")
    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner
    a = dict(A.ARCHS[args.arch], recompute=args.mode)
    a["num_frames"] = max(a["num_frames"], args.frames)
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
    run = StepRunner(m, opt)
    m._fresh_shadows(); m._sync_requires_grad()
    batch = synth_batch(a, args.pairs, args.frames, seed=0, caption_len=32)
    pb = m.engine.prepare_batch(batch)
    lab = batch["label"].reshape(-1).to(torch.int32).cuda()
    for _ in range(args.warmup):
        out = run.run(pb, lab)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        out = run.run(pb, lab)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    l1, l2 = float(out["loss1"]), float(out["loss2"])
    if not (l1 == l1 and l2 == l2):
        raise SystemExit(f"losses are not finite: {l1} {l2}")
    med, mean = sorted(times)[len(times) // 2], sum(times) / len(times)
    print(json.dumps({"what": "training step under activation recomputation", "arch": args.arch, "frames": args.frames,
                      "pairs": args.pairs, "mode": args.mode, "ms_per_step": 1e3 * med, "ms_per_step_mean": 1e3 * mean,
                      "pairs_per_s": args.pairs / med, "workspace_bytes": m.engine.workspace_bytes(),
                      "max_memory_allocated": torch.cuda.max_memory_allocated(),
                      "device_bytes": torch.cuda.get_device_properties(0).total_memory,
                      "recompute_count": m.engine.recompute_count, "steps": args.steps, "warmup": args.warmup,
                      "loss1": l1, "loss2": l2, "launches": "eager"}), flush=True)


def run_child(arch, frames, pairs, mode, args):
    """one mode of one configuration in a fresh process under its own time limit -> its JSON line (dict), None if it failed"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--arch", arch, "--frames", str(frames), "--pairs", str(pairs),
           "--mode", mode, "--steps", str(args.steps), "--warmup", str(args.warmup)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        print(f"bench_recompute: {arch} {frames} frames {pairs} pairs {mode!r} ran into its time limit of {args.limit} s", file=sys.stderr)
        return None
    line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
    if r.returncode != 0 or line is None:
        print(f"bench_recompute: {arch} {frames} frames {pairs} pairs {mode!r} failed (exit status {r.returncode})\n{r.stderr[-2000:]}",
              file=sys.stderr)
        return None
    print(line, flush=True)
    return json.loads(line)


def rows_bound(arch_name="H_14", frames=16):
    """the most pairs at which the [M, 4W] bf16 tensors of a block stay below 2^31 bytes (M = pairs * (1 + frames * kept patches))"""
    from tvts_amd import arch as A
    a = A.ARCHS[arch_name]
    return (2 ** 31 - 1) // ((1 + frames * A.n_keep(a)) * 4 * a["width"] * 2)


def largest_batch(peak96, device_bytes, want=None, cap=None):
    """The batch rule: bytes(N) = peak at 96 pairs * N / 96 must leave FREE_FRACTION of the card free, and N <= cap (rows_bound).
    want None -> the largest multiple of 8 that passes; a number -> that number if it passes, else ValueError."""
    room = (1.0 - FREE_FRACTION) * device_bytes
    best = int(room * 96 / peak96) // 8 * 8
    if cap is not None:
        best = min(best, cap // 8 * 8)
        if want is not None and want > cap:
            raise ValueError(f"--batch {want}: a block's [M, 4W] tensors would pass 2^31 bytes (at most {cap} pairs stay below)")
    if want is None:
        return best
    if peak96 * want / 96.0 > room:
        raise ValueError(f"--batch {want}: {peak96 * want / 96.0 / 2 ** 30:.1f} GiB by the 96-pair peak scaled linearly, more than "
                         f"{100 * (1 - FREE_FRACTION):.0f} % of the card's {device_bytes / 2 ** 30:.1f} GiB (largest batch that passes: {best})")
    return int(want)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=420, help="seconds one child may take")
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=MODES)
    ap.add_argument("--only", nargs="+", metavar="ARCH:FRAMES:PAIRS", help="these configurations instead of the three")
    ap.add_argument("--batch", help="H/14, 16 frames: one mode (--mode) at this many pairs, or 'auto'")
    ap.add_argument("--mode", default="block", choices=MODES)
    ap.add_argument("--lines", help="with --batch: a file of earlier output lines to take the 96-pair peak from")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--arch", help=argparse.SUPPRESS)
    ap.add_argument("--frames", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--pairs", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.batch is not None:
        base = None
        if args.lines:
            for ln in open(args.lines):
                if ln.startswith("{"):
                    d = json.loads(ln)
                    if (d.get("arch"), d.get("frames"), d.get("pairs"), d.get("mode")) == ("H_14", 16, 96, args.mode):
                        base = d
        if base is None:
            base = run_child("H_14", 16, 96, args.mode, args)
            if base is None:
                raise SystemExit(1)
        try:
            n = largest_batch(base["max_memory_allocated"], base["device_bytes"], None if args.batch == "auto" else int(args.batch),
                              cap=rows_bound())
        except ValueError as e:
            raise SystemExit(str(e))
        if run_child("H_14", 16, n, args.mode, args) is None:
            raise SystemExit(1)
        return
    configs = CONFIGS if not args.only else tuple((c.split(":")[0], int(c.split(":")[1]), int(c.split(":")[2])) for c in args.only)
    for arch, frames, pairs in configs:
        for mode in args.modes:
            if run_child(arch, frames, pairs, mode, args) is None:
                raise SystemExit(1)  # the first failure ends the run: nothing more is started on the card


if __name__ == "__main__":
    main()
