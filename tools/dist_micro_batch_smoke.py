#!/usr/bin/env python3
"""The micro-batched pretraining step (StepRunner(micro_batches=2)) across two data-parallel ranks on ONE GPU (gloo
backend moving CUDA tensors), in the style of tools/dist_train_guard_smoke.py.

B = 4 clips per rank, two chunks of 2.  Per rank this prints and checks: a rank built with another chunk count raises on BOTH
(StepRunner's construction check); two steps whose parameter checksums are equal across the ranks; bytes_sent of the gradient
exchange equal to the n = 1 step's on the same batch (ONE exchange, behind the last chunk's backward, not one per chunk); loss1 the
same bits on both ranks.  The parent then runs the plain single-process step on the 8-pair batch (rank 0's clips, then rank 1's)
and holds the ranks' first loss1 to it within the loss tolerance of the model tests (1e-2): the negatives are all 8 pairs.
usage: python tools/dist_micro_batch_smoke.py"""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

B, N_MICRO, STEPS = 4, 2, 2


def rank_batch(O, oarch, step, rank):
    return O.synth_batch(oarch, B=B, T=2, seed=60 + 10 * step + rank, caption_len=9)


def build(rank, world, micro_batches=None, construct=True):
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
    runner = None
    if construct:
        runner = StepRunner(m, opt) if micro_batches is None else StepRunner(m, opt, micro_batches=micro_batches)
    return O, oarch, m, opt, runner


def worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from tvts_amd.step import StepRunner

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

    O, oarch, m, opt, _ = build(rank, world, construct=False)
    # a rank that splits in two beside a rank that does not: the construction check raises on both
    try:
        StepRunner(m, opt, micro_batches=1 + rank)
        ok = False
        say("the mismatched construction did NOT raise")
    except RuntimeError as e:
        say("MICRO_MISMATCH_RAISED", str(e)[:120])

    runner = StepRunner(m, opt, micro_batches=N_MICRO)
    _, _, m1, opt1, plain = build(rank, world)  # the n = 1 step beside it, on the same batches: its bytes_sent is the bar
    first = None
    for step in range(STEPS):
        batch = rank_batch(O, oarch, step, rank)
        out = runner.step(batch)
        torch.cuda.synchronize()
        sent = runner.sync.bytes_sent
        out1 = plain.step(batch)
        torch.cuda.synchronize()
        chk = m.store.flat.view(torch.int32).to(torch.int64).sum().reshape(1)
        same_p, same_l = across(chk), across(out["loss1"])
        d1 = abs(float(out["loss1"]) - float(out1["loss1"]))
        say(f"step {step + 1}: loss1 {float(out['loss1'])!r} (n = 1 step {float(out1['loss1'])!r}), parameter checksum {int(chk)}, equal across "
            f"ranks {same_p}, loss1 equal {same_l}, bytes_sent {sent} (n = 1: {plain.sync.bytes_sent})")
        ok = ok and same_p and same_l and sent == plain.sync.bytes_sent and sent > 0 and d1 < 1e-2
        if first is None:
            first = float(out["loss1"])
    finite = bool(torch.isfinite(m.store.flat).all())
    ok = ok and finite and opt.state_dict()["state"][0]["step"] == STEPS
    if ok:
        say("micro: replicas equal after every step, one exchange per step, same loss1 on both ranks")
    else:
        say("FAILED", dict(finite=finite))
    q.put((bool(ok), first))
    dist.barrier()
    dist.destroy_process_group()


def merged(batches):
    """the ranks' batches as ONE batch: clips rank by rank, text transcript-major over all of them"""
    Bs = [b["video"].shape[0] for b in batches]
    NT = batches[0]["text"].shape[0] // Bs[0]
    text = torch.cat([torch.cat([b["text"].reshape(NT, n, -1)[t] for b, n in zip(batches, Bs)]) for t in range(NT)])
    out = {k: torch.cat([b[k] for b in batches]) for k in batches[0] if k != "text"}
    out["text"] = text
    return out


if __name__ == "__main__":
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, 2, 29523, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=200) for _ in procs]
    for p in procs:
        p.join()
    assert all(r[0] for r in res) and all(p.exitcode == 0 for p in procs)
    # the single-process step on the 8-pair batch (the ranks are gone: this process is the only one on the GPU now)
    O, oarch, m, opt, runner = build(0, 1)
    out = runner.step(merged([rank_batch(O, oarch, 0, r) for r in range(2)]))
    torch.cuda.synchronize()
    whole = float(out["loss1"])
    print(f"single-process step on the {2 * B}-pair batch: loss1 {whole!r}; the ranks' {res[0][1]!r}")
    assert abs(whole - res[0][1]) < 1e-2 and res[0][1] == res[1][1], (whole, res)
    print("DIST_MICRO_BATCH_OK")
