#!/usr/bin/env python3
"""The pretraining step's gradient clipping and overflow guard across two data-parallel ranks on ONE GPU (gloo backend moving CUDA
tensors), in the style of tools/dist_smoke.py.

Three steps of StepRunner(clip_grad=..., skip_nonfinite=True) over FusedHFAdamW; on step 2 the clip of rank 1's shard -- and only
that one -- carries one NaN pixel.  The norm is taken behind the all-reduce, so both ranks must see the same (non-finite) number
without any further collective, skip together and stay replicas: per rank this prints and checks skipped == 1, parameter checksums
equal across the ranks after every step, grad_norm the same bits on both ranks, and a finite state at the end.  In front of that,
a rank that guards beside a rank that does not must raise on BOTH (StepRunner's construction check).
usage: python tools/dist_train_guard_smoke.py"""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def nan_pixel(batch, arch):
    """a copy of the batch with ONE NaN pixel in sample 0, inside a patch the tube mask keeps"""
    out = dict(batch)
    v = batch["video"].clone()
    p = arch["patch"]
    g = arch["image"] // p
    k = int(batch["keep_ind"][0][0])
    v[0, 0, 0, (k // g) * p, (k % g) * p] = float("nan")
    out["video"] = v
    return out


def worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from oracle import tvts_oracle as O
    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    m = TVTSv2Base(types.SimpleNamespace(local_rank=0, rank=rank, world_size=world), arch=a)
    m.load_state_dict(O.synth_params(oarch, seed=3), strict=True)
    groups = [[], [], [], []]
    for name, p in m.named_parameters():
        gi = A.param_group_of(name, a)
        if gi < 0:
            p.requires_grad = False
        else:
            groups[gi].append(p)
    opt = FusedHFAdamW([dict(params=groups[i], lr=A.GROUP_HPARAMS[i][0], weight_decay=A.GROUP_HPARAMS[i][1]) for i in range(4)],
                       m.store, model=m)
    def say(*x):  # one write per line: the two ranks share the parent's stdout, and pieces of two lines would interleave
        sys.stdout.write(" ".join([f"[rank {rank}]"] + [str(v) for v in x]) + "\n")
        sys.stdout.flush()
    ok = True

    def across(t):
        """the tensor of every rank -> True when all ranks hold the same bits"""
        t = t.detach().reshape(-1).contiguous()
        t = t.view(torch.int32 if t.element_size() == 4 else torch.int64).to(torch.int64)
        rows = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(rows, t)
        return all(torch.equal(rows[0], r) for r in rows[1:])

    # a rank with the guard beside a rank without it: the construction check raises on both
    try:
        StepRunner(m, opt, skip_nonfinite=(rank == 0))
        ok = False
        say("the mismatched construction did NOT raise")
    except RuntimeError as e:
        say("GUARD_MISMATCH_RAISED", str(e)[:120])
    assert opt.norm_coef is None  # (a refused construction leaves the optimizer as it was)

    runner = StepRunner(m, opt, clip_grad=0.05, skip_nonfinite=True)
    norms = []
    for step in range(3):
        batch = O.synth_batch(oarch, B=3, T=2, seed=50 + 10 * step + rank, caption_len=9)
        if step == 1 and rank == 1:
            batch = nan_pixel(batch, oarch)
        out = runner.step(batch)
        torch.cuda.synchronize()
        chk = m.store.flat.view(torch.int32).to(torch.int64).sum().reshape(1)
        same_p, same_n = across(chk), across(out["grad_norm"])
        norms.append(float(out["grad_norm"]))
        say(f"step {step + 1}: grad_norm {norms[-1]!r}, parameter checksum {int(chk)}, equal across ranks {same_p}, grad_norm equal {same_n}")
        ok = ok and same_p and same_n
    skipped, st = int(runner.skipped.item()), m.store
    finite = all(bool(torch.isfinite(t.float()).all()) for t in (st.flat, st.m, st.v, st.shadow))
    expect = [True, False, True]
    ok = ok and skipped == 1 and finite and [n == n and abs(n) != float("inf") for n in norms] == expect
    ok = ok and opt.state_dict()["state"][0]["step"] == 2
    if ok:
        say("guard: skipped 1, replicas equal after every step, same grad_norm on both ranks, finite state at the end")
    else:
        say("FAILED", dict(skipped=skipped, finite=finite, norms=norms))
    q.put(bool(ok))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, 2, 29517, q)) for r in range(2)]
    for p in procs:
        p.start()
    oks = [q.get(timeout=200) for _ in procs]
    for p in procs:
        p.join()
    assert all(oks) and all(p.exitcode == 0 for p in procs)
    print("DIST_TRAIN_GUARD_OK")
