#!/usr/bin/env python3
"""Two data-parallel ranks of the v1 fine-tuning step and of the evaluation merges on ONE GPU (gloo moving device tensors, the
pattern of tools/dist_smoke.py): FinetuneStep's gradient exchange, validation_one_epoch's meter merge and ViewMerger.gather.
usage: python tools/dist_finetune_smoke.py [--ema] [--guard] [--opt {adamw,sgd}] [check ...]      (no argument: every check, in one pair of processes)
checks: identical distinct replicas travel bf16 start mismatch seeds validation merge
--opt sgd: the same checks with FusedTorchSGD (lr 0.1, momentum 0.9, Nesterov: torch.optim.SGD as the linear-probe script builds it)
in place of FusedTorchAdamW -- all but `bf16`, whose bound is derived for AdamW's first step -- and the check `optimizers` behind
them: a rank built with AdamW beside a rank built with SGD, both raise.
--ema: the check `ema` behind the named ones (alone when none is named; not part of "every check") -- a ModelEma made BEFORE the
step object on ranks that start from different weights, both ranks' ModelEma.checksum() after _join and after two updating steps.
--guard: the check `guard` behind the named ones (alone when none is named; not part of "every check") -- FinetuneStep(
skip_nonfinite=True) on both ranks, a NaN pixel in rank 1's shard only on call 2 of 3: both ranks skip that update, count it, and
hold equal, finite replicas after every call; a guarded rank beside an unguarded one raises on both.
The model is tests/v1_downstream_synth.TINY; the gates are the test suite's own (tests/kernel_bounds.py, check_grads of
tests/test_v1_gpu.py), imported from tests/.  Prints DIST_FINETUNE_OK when every rank passed every check."""
import math
import multiprocessing as mp
import os
import socket
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = ("identical", "distinct", "replicas", "travel", "bf16", "start", "mismatch", "seeds", "validation", "merge")
OPTIONAL = ("ema", "optimizers", "guard")  # checks a flag asks for
ADAMW_ONLY = ("bf16",)  # (its bound is AdamW's first step)
SGD_LR, SGD_MOMENTUM = 0.1, 0.9
DEV, CLASSES, T, LR, WD, LAYER_DECAY, CH = "cuda:0", 5, 4, 1e-3, 0.05, 0.75, 1024
SEED_BASE = 0x9A3C5F1B7E24D694


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class Ctx:
    """what every check of one rank shares: the modules, the rank, a model that was built BEFORE the process group existed"""

    def __init__(self, rank, world, early, opt="adamw"):
        import numpy as np
        import torch
        import torch.distributed as dist

        import kernel_bounds as KB
        import v1_downstream_synth as S
        from tvts_amd import hip as K
        from tvts_amd.downstream import evaluate_v1 as E
        from tvts_amd.downstream import finetune_v1 as F
        self.np, self.torch, self.dist, self.KB, self.S, self.K, self.E, self.F = np, torch, dist, KB, S, K, E, F
        self.rank, self.world, self.early, self.opt = rank, world, early, opt
        self.sd = S.synth_state(S.TINY, 61, CLASSES)

    # ---- builders
    def model(self, rate=0.0, load=True, init_seed=0):
        from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
        m = VisionTransformer(num_classes=CLASSES, drop_path_rate=rate, init_seed=init_seed, **self.S.TINY)
        if load:
            m.load_state_dict(self.sd, strict=True)
        return m

    def stepper(self, m, trainable="all", opt=None, **kw):
        F = self.F
        groups = F.param_groups(m, WD, LAYER_DECAY, trainable=trainable)
        if (opt or self.opt) == "sgd":
            lr, opt = SGD_LR, F.FusedTorchSGD(groups, m.store, lr=SGD_LR, momentum=SGD_MOMENTUM, nesterov=True, model=m)
        else:
            lr, opt = LR, F.FusedTorchAdamW(groups, m.store, lr=LR, model=m)
        for g in opt.param_groups:
            g["lr"] = lr * g["lr_scale"]
        return F.FinetuneStep(m, opt, trainable=trainable, **kw), opt

    def clips(self, B, seed):
        return self.S.synth_clip(self.S.TINY, B, T, seed)

    def labels(self, B, seed):
        torch = self.torch
        return torch.randint(0, CLASSES, (B,), generator=torch.Generator().manual_seed(seed))

    def table(self, B, seed):
        """a fixed stochastic-depth table [2 * depth, B]: kept samples scaled by 1.25, one dropped entry"""
        torch = self.torch
        t = torch.where(torch.rand(2 * self.S.TINY["depth"], B, generator=torch.Generator().manual_seed(seed)) < 0.5, 1.25, 1.0)
        t[1, 0] = 0.0
        return t.to(torch.float32).to(DEV).contiguous()

    # ---- exchanges of the checks themselves
    def all_equal(self, t, what):
        """the device tensor t holds the same bits on every rank"""
        torch, dist = self.torch, self.dist
        t = t.contiguous()
        every = [torch.empty_like(t) for _ in range(self.world)]
        dist.all_gather(every, t)
        for r, o in enumerate(every[1:], 1):
            self.KB.assert_equal_bits(o, every[0], f"{what}: rank {r} against rank 0")
        return every

    def bits(self, got, want, what):
        self.KB.assert_equal_bits(got, want, f"[rank {self.rank}] {what}")

    def say(self, *a):
        sys.stdout.write(f"[rank {self.rank}] " + " ".join(str(v) for v in a) + "\n")  # (one write: the ranks share the terminal)
        sys.stdout.flush()


def state_of(m):
    st = m.store
    # (SGD keeps no second state buffer: store.v does not exist then)
    return {k: t.clone() for k, t in (("flat", st.flat), ("m", st.m), ("v", st.v), ("shadow", st.shadow)) if t is not None}


def bitsum(c, t):
    return t.view(c.torch.int32).sum(dtype=c.torch.int64)


# ================================================================================================ 1. identical shards
def check_identical(c):
    """both ranks hold the same clips, targets and mask table: the averaged gradient is (g + g) / 2 = g exactly, so two updating
    steps leave the bits of the single-process step -- parameters, moments, shadows, grad_norm and loss"""
    torch = c.torch
    clips, labels = [c.clips(2, 100 + k) for k in range(4)], [c.labels(2, 200 + k) for k in range(4)]
    for name, kw in (("clip off", {}), ("clip on", dict(clip_grad=0.05)), ("update_freq 2", dict(update_freq=2, clip_grad=0.05))):
        runs = []
        for dp in (None, False):
            m = c.model(rate=0.1)
            step, _ = c.stepper(m, smoothing=0.1, data_parallel=dp, **kw)
            assert (step.sync is not None) == (dp is None)
            outs = []
            for k in range(2 * kw.get("update_freq", 1)):
                m.engine.drop_path_override = c.table(2, 300 + k)
                o = step.step(clips[k], labels[k])
                outs.append((o["loss"].clone(), o["grad_norm"], step.norm_coef[1].clone()))
            torch.cuda.synchronize()
            runs.append((state_of(m), outs))
        (sa, oa), (sb, ob) = runs
        for k in sa:
            c.bits(sa[k], sb[k], f"identical shards, {name}: {k}")
        for k, (a, b) in enumerate(zip(oa, ob)):
            c.bits(a[0].reshape(1), b[0].reshape(1), f"identical shards, {name}: loss of call {k}")
            assert (a[1] is None) == (b[1] is None)
            if a[1] is not None:
                c.bits(a[1].reshape(1), b[1].reshape(1), f"identical shards, {name}: grad_norm of call {k}")
                if "clip_grad" in kw:
                    assert float(a[2]) < 1.0, ("the clip is not active", float(a[1]), float(a[2]))
        assert not torch.equal(sa["flat"], c.model().store.flat)
        c.say(f"identical shards, {name}: bit-equal to the single-process step (grad_norm {float(oa[-1][1]):.5f})")


# ================================================================================================ 2. distinct shards
def fwd_bwd(c, m, clip, labels, sync=None):
    """one forward / loss / backward through the engine, the gradients left in the store -> (logits, loss)"""
    torch, K, eng = c.torch, c.K, m.engine
    m.set_trainable("all")
    m._fresh_shadows()
    K.zero_(m.store.grad)
    B = clip.shape[0]
    logits = eng.finetune_forward(clip.to(DEV), B, T // 2)
    cell = torch.zeros(1, dtype=torch.float32, device=DEV)
    dl, ws = torch.empty_like(logits), torch.empty(2 * B, dtype=torch.float32, device=DEV)
    K.soft_ce(logits, cell, ws, labels=labels.to(DEV, torch.int32), smoothing=0.1, scale=1.0, dlogits=dl)
    eng.grad_ready = None if sync is None else sync.reduce_range
    try:
        eng.finetune_backward(dl, "all")
    finally:
        eng.grad_ready = None
    scale = 1.0 if sync is None else sync.finish()
    torch.cuda.synchronize()
    return logits.clone(), float(cell), scale


def check_distinct(c):
    """2 + 2 clips on two ranks against the single-process backward over the 4: the exchanged gradient times 1 / W under
    check_grads (tests/test_v1_gpu.py, as test_update_freq_two_half_batches uses it); at step level grad_norm within 1 % of the
    float64 norm of the full-batch gradient, and the mean of the ranks' losses against the full-batch loss"""
    from test_v1_gpu import check_grads
    from tvts_amd import dist as D
    torch, dist = c.torch, c.dist
    clip, labels = c.clips(4, 71), c.labels(4, 72)
    m = c.model()
    full_logits, full_loss, _ = fwd_bwd(c, m, clip, labels)
    full = {m.store_name(n): g.detach().cpu().clone() for n, g in m.grad_views().items()}
    mine = slice(2 * c.rank, 2 * c.rank + 2)
    sync = D.GradSync(m.store.grad, payload="fp32")
    logits, loss, scale = fwd_bwd(c, m, clip[mine], labels[mine], sync=sync)
    assert scale == 1.0 / c.world and sync.bytes_sent > 0
    m.store.grad.mul_(scale)
    check_grads(m.store, full)
    c.all_equal(m.store.grad, "the exchanged gradient")
    # the step: a fresh replica per rank
    m2 = c.model()
    step, _ = c.stepper(m2, smoothing=0.1)
    out = step.step(clip[mine], labels[mine])
    gn_full = math.sqrt(sum(float(g.double().norm()) ** 2 for g in full.values()))
    gn = float(out["grad_norm"])
    c.say(f"distinct shards: grad_norm {gn:.6f}, float64 norm of the full-batch gradient {gn_full:.6f}")
    assert abs(gn - gn_full) < 0.01 * gn_full, (gn, gn_full)
    both = [torch.zeros(1, device=DEV) for _ in range(c.world)]
    dist.all_gather(both, out["loss"].reshape(1).clone())
    mean = sum(float(b) for b in both) / c.world
    # the bound tests/test_v1_finetune_gpu.py holds losses to: cross entropy is 2-Lipschitz in the sup norm of the logits, here the
    # half batch's logits against the same rows of the full batch's; plus the fp32 rounding of the two loss sums (4 rows + the
    # scale + the mean of the two: 8 roundings of numbers no larger than the loss)
    dm = torch.zeros(1, device=DEV) + float((out["logits"] - full_logits[mine]).abs().max())
    dist.all_reduce(dm, op=dist.ReduceOp.MAX)
    bound = 2 * float(dm) + 8 * 2.0 ** -24 * abs(full_loss)
    c.say(f"distinct shards: mean of the ranks' losses {mean:.7f}, full batch {full_loss:.7f}, bound {bound:.3e}")
    assert abs(mean - full_loss) <= bound and abs(mean - full_loss) < 1e-2, (mean, full_loss, bound)


# ================================================================================================ 3. replicas stay identical
def check_replicas(c):
    """3 steps with distinct shards, each rank's own stochastic-depth masks (rate 0.1) and its own Mixup plan: parameters and
    moments keep the same bits on both ranks, while the mask tables differ"""
    torch, np = c.torch, c.np
    m = c.model(rate=0.1)
    m.engine.set_drop_seed_base(SEED_BASE)
    step, _ = c.stepper(m, clip_grad=1.0)
    mix = c.F.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1, num_classes=CLASSES)
    np.random.seed(7 + c.rank)  # (the script: seed + rank)
    differ = False
    for k in range(3):
        step.step(c.clips(2, 400 + 10 * k + c.rank), c.labels(2, 500 + 10 * k + c.rank), mix=mix.draw(2, c.S.TINY["img_size"]))
        tabs = [torch.empty_like(m.engine.buf["ft.dp_table"]) for _ in range(c.world)]
        c.dist.all_gather(tabs, m.engine.buf["ft.dp_table"].contiguous())
        differ = differ or not torch.equal(tabs[0], tabs[1])
    assert differ, "both ranks drew the same stochastic-depth masks in every step"
    sums = torch.stack([step.replicas_checksum()] + [bitsum(c, t) for t in (m.store.m, m.store.v) if t is not None])
    assert sums.dtype == torch.int64 and sums.is_cuda
    assert sums.numel() == (2 if c.opt == "sgd" else 3)
    c.all_equal(sums, "replicas_checksum and the checksums of the optimizer's state buffers after 3 steps")
    c.all_equal(m.store.flat, "the parameters after 3 steps")
    assert int(step.replicas_checksum()) != int(bitsum(c, c.model().store.flat))
    c.say("replicas: parameters and moments equal on both ranks after 3 steps, masks differ")


# ================================================================================================ 4. what travels
def check_travel(c):
    torch, dist = c.torch, c.dist
    depth = c.S.TINY["depth"]
    for payload, trainable in (("fp32", "all"), ("bf16", "all"), ("fp32", "head")):
        m = c.model()
        step, opt = c.stepper(m, trainable=trainable, update_freq=2, payload=payload)
        ranges, calls = [], [0]
        inner, real = step.sync.reduce_range, dist.all_reduce

        def record(lo, hi):
            ranges.append((lo, hi))
            return inner(lo, hi)

        def counted(*a, **k):
            calls[0] += 1
            return real(*a, **k)
        step.sync.reduce_range, dist.all_reduce = record, counted
        before = state_of(m)
        try:
            o1 = step.step(c.clips(2, 600 + c.rank), c.labels(2, 610 + c.rank))
            assert o1["grad_norm"] is None and step.bytes_sent == 0 and not ranges and calls[0] == 0, (step.bytes_sent, ranges, calls)
            assert m.engine.grad_ready is None
            step.step(c.clips(2, 620 + c.rank), c.labels(2, 630 + c.rank))
        finally:
            dist.all_reduce = real
        torch.cuda.synchronize()
        assert m.engine.grad_ready is None and calls[0] >= len(ranges) > 0
        # disjoint, chunk-aligned, and together exactly the chunks the optimizer updates
        cover = torch.zeros(opt.chunk_group.numel(), dtype=torch.int32)
        for lo, hi in ranges:
            assert lo % CH == 0 and hi % CH == 0 and hi > lo, (lo, hi)
            cover[lo // CH:hi // CH] += 1
        want = (opt.chunk_group.cpu() != 255).to(torch.int32)
        assert torch.equal(cover, want), ("the ranges are not a disjoint cover of the trainable chunks", ranges)
        count = int(want.sum()) * CH
        assert step.bytes_sent == (4 if payload == "fp32" else 2) * count, (payload, step.bytes_sent, count)
        # backward order: head, blocks depth - 1 .. 0, then the embedding parameters (and the final norm, which the engine reports last)
        st = m.store

        def stage(lo, hi):
            s = set()
            for n in st.shapes:
                if lo <= st.off[n] < hi:
                    s.add(0 if n.startswith("head.") else 1 + (depth - 1 - int(n.split("blocks.")[1].split(".")[0])) if ".blocks." in n
                          else depth + 1)
            assert len(s) == 1, (lo, hi, s)
            return s.pop()
        stages = [stage(lo, hi) for lo, hi in ranges]
        assert stages == sorted(stages) and stages[0] == 0, stages
        if trainable == "head":
            lo = st.off["head.weight"]
            assert set(stages) == {0} and min(r[0] for r in ranges) == lo, (ranges, lo)
            after = state_of(m)
            for k in before:
                c.bits(after[k][:lo], before[k][:lo], f"linear probe across ranks: {k} of the tower")
                assert not torch.equal(after[k][lo:], before[k][lo:]), k
        else:
            assert set(stages) == set(range(depth + 2)), stages
        c.all_equal(m.store.flat, f"parameters after the {payload} / {trainable} exchange")
        c.say(f"travel {payload} {trainable}: {len(ranges)} ranges, {count} elements, {step.bytes_sent} bytes, stages {stages}")


# ================================================================================================ 5. bf16 payload
def check_bf16(c):
    """identical shards, no clipping, first step: the averaged gradient is the bf16 rounding of g, |dg| <= 2^-8 |g| (round to nearest
    of an 8-bit significand; bf(g) + bf(g) and the halving are exact).  The first AdamW update is lr f(g), f(g) = g / (|g| + eps):
    m / bc1 = g and sqrt(v / bc2) = |g| at step 1.  f'(g) = eps / (|g| + eps)^2 <= 1 / (|g| + eps), so
    |df| <= 2^-8 |xi| eps / (|xi| + eps)^2 <= 2^-8 / 4 for xi between g and bf(g) (x eps / (x + eps)^2 peaks at 1/4): below the
    2^-9 the bound is stated with.  A gradient under bf16's normal range (|g| < 2^-126) moves by at most 2^-134, f by that over
    eps.  Both runs then round in fp32: the decay product, m, v, the square root, the quotient and the final subtraction, each
    within one unit roundoff of a number no larger than |p| + lr -- 8 roundings per run, 16 between the two."""
    torch, KB = c.torch, c.KB
    clip, labels = c.clips(2, 700), c.labels(2, 701)
    res = {}
    for payload in ("fp32", "bf16"):
        m = c.model()
        step, opt = c.stepper(m, payload=payload)
        step.step(clip, labels)
        torch.cuda.synchronize()
        res[payload] = m.store.flat.clone()
    lr = torch.tensor([float(g["lr"]) for g in opt.param_groups] + [0.0] * (256 - len(opt.param_groups)), dtype=torch.float64)
    lr_elem = lr[opt.chunk_group.cpu().long()].repeat_interleave(CH).to(DEV)  # 0 on frozen / padding chunks (group 255)
    eps = 1e-8
    ref = res["fp32"].double()
    bound = lr_elem * (2.0 ** -9 + 2.0 ** -134 / eps) + 16 * KB.U32 * (ref.abs() + lr_elem)
    w = KB.assert_within(res["bf16"], ref, bound, f"[rank {c.rank}] parameters after one step, bf16 against fp32 payload")
    for r in range(c.world):  # (one rank's line at a time: the ranks share the terminal)
        if r == c.rank:
            KB.bound_line(f"finetune bf16 payload rank={c.rank}", w)
            sys.stdout.flush()
        c.dist.barrier()
    assert not torch.equal(res["bf16"], res["fp32"])
    c.all_equal(res["bf16"], "parameters after the bf16 exchange")


# ================================================================================================ 6. start-up
def check_start(c):
    """ranks built from different init seeds hold rank 0's parameters (and the shadows derived from them) after construction"""
    torch = c.torch
    m = c.model(load=False, init_seed=11 + c.rank)
    own = m.store.flat.clone()
    first = [torch.empty_like(own) for _ in range(c.world)]
    c.dist.all_gather(first, own)
    assert not torch.equal(first[0], first[1]), "the test's replicas start equal"
    step, _ = c.stepper(m)
    torch.cuda.synchronize()
    c.bits(m.store.flat, first[0], "parameters after construction against rank 0's")
    c.all_equal(m.store.shadow, "bf16 shadows after construction")
    c.all_equal(m.store.shadow_t, "transposed shadows after construction")
    m0 = c.model(load=False, init_seed=11)  # rank 0's model, built locally: its shadows are what every rank must hold
    m0._fresh_shadows()
    c.bits(m.store.shadow, m0.store.shadow, "bf16 shadows against a local build of rank 0's model")
    c.all_equal(step.replicas_checksum().reshape(1), "replicas_checksum after construction")
    c.say("start: every rank holds rank 0's parameters")


def check_mismatch(c):
    """trainable="head" beside "all": both ranks raise, neither is left in a collective (the checks that follow still run)"""
    m = c.model()
    try:
        c.stepper(m, trainable="all" if c.rank == 0 else "head")
    except RuntimeError as e:
        c.say("MISMATCH_RAISED:", str(e))
        assert "differs between the ranks" in str(e)
    else:
        raise AssertionError("ranks with different `trainable` were accepted")
    t = c.torch.ones(1, device=DEV)
    c.dist.all_reduce(t)  # the group is still usable
    assert float(t) == c.world


def check_seeds(c):
    """the per-rank offset reaches the fine-tune path whether the process group exists when the model is built or is created
    afterwards, and a resumed pair (set_drop_seed_base of rank 0's value) continues each rank's own mask sequence"""
    torch = c.torch
    early, late = c.early, c.model(rate=0.1)
    assert early.engine._drop_rank == 0 and late.engine._drop_rank == c.rank
    tabs = {}
    for name, m in (("early", early), ("late", late)):
        step, _ = c.stepper(m)
        assert m.engine._drop_rank == c.rank  # (no seed is set here: both models run on from the seed they were built with)
        seq, bases = [], []
        for k in range(3):
            bases.append(m.engine.drop_seed_base())
            step.step(c.clips(2, 800 + k), c.labels(2, 810 + k))
            seq.append(m.engine.buf["ft.dp_table"].clone())
        both = [torch.zeros(1, dtype=torch.int64, device=DEV) for _ in range(c.world)]
        c.dist.all_gather(both, torch.tensor([bases[2] - (1 << 63)], dtype=torch.int64, device=DEV))
        assert int(both[0]) == int(both[1]), "drop_seed_base differs between the ranks"
        m.engine.set_drop_seed_base(int(both[0]) + (1 << 63))  # rank 0 wrote the checkpoint in front of step 3, every rank reads it
        step.step(c.clips(2, 802), c.labels(2, 812))
        c.bits(m.engine.buf["ft.dp_table"], seq[2], f"{name}: the resumed step's mask table against the uninterrupted run's")
        tabs[name] = torch.stack(seq)
    c.bits(tabs["early"], tabs["late"], "mask tables of a model built before the process group against one built after")
    every = [torch.empty_like(tabs["late"]) for _ in range(c.world)]
    c.dist.all_gather(every, tabs["late"])
    assert not torch.equal(every[0], every[1]), "both ranks drew the same masks"
    c.say("seeds: per-rank mask sequences, early and late construction agree, resume continues them")


# ================================================================================================ 7. validation
def check_validation(c):
    """four fixed batches (2, 2, 2 and 1 clips) as two per rank against one process over the four, within 1e-12 relative"""
    torch, E = c.torch, c.E
    m = c.model()
    sizes = (2, 2, 2, 1)
    vids = [c.clips(n, 900 + k) for k, n in enumerate(sizes)]
    # labels from the model's own predictions: the short batch is all right, the full ones all wrong, so the sample-weighted
    # top-1 (100 / 7) and the batch-weighted one (25) cannot be mistaken for one another
    labs = [(m(v).argmax(dim=1).cpu() + (0 if n == 1 else 1)) % CLASSES for v, n in zip(vids, sizes)]
    batches = list(zip(vids, labs))
    single = E.validation_one_epoch(batches, m, sync=False)
    merged = E.validation_one_epoch(batches[c.rank::2], m)
    own = E.validation_one_epoch(batches[c.rank::2], m, sync=False)
    c.say("validation: merged", merged, "single process", single, "this rank alone", own)
    for k in ("acc1", "acc5", "loss"):
        assert abs(merged[k] - single[k]) <= 1e-12 * abs(single[k]), (k, merged[k], single[k])
    assert abs(single["acc1"] - 100.0 / 7) < 1e-9 and abs(merged["acc1"] - 25.0) > 1.0 and single["acc5"] == 100.0
    assert own["acc1"] != merged["acc1"]
    vals = torch.tensor([merged[k] for k in ("acc1", "acc5", "loss")], dtype=torch.float64, device=DEV)
    c.all_equal(vals, "the merged meters")


# ================================================================================================ 8. test merge
def check_merge(c):
    """b0 .. b3 of one process as b0, b2 on rank 0 and b1, b3 on rank 1, which also carries duplicates of two b0 lines with
    other logits: gather() holds the single-process merger's bits, the duplicates lose to rank 0's lines"""
    torch, E, K = c.torch, c.E, c.K
    m = c.model()
    V, crops, nvid = 6, 3, 4
    lines = [(f"video{v}", s // crops, s % crops, 1000 + 10 * v + s) for v in range(nvid) for s in range(V)]
    order = torch.randperm(len(lines), generator=torch.Generator().manual_seed(5)).tolist()
    lines = [lines[i] for i in order]
    label = {f"video{v}": int(c.labels(nvid, 55)[v]) for v in range(nvid)}

    def batch(ls):
        return (torch.cat([c.clips(1, seed) for *_, seed in ls]), torch.tensor([label[l[0]] for l in ls]), [l[0] for l in ls],
                [l[1] for l in ls], [l[2] for l in ls])
    b = [batch(lines[6 * k:6 * k + 6]) for k in range(4)]
    dup = batch([(vid, ch, sp, seed + 5000) for vid, ch, sp, seed in lines[:2]])  # b0's first two keys, other clips

    def run(batches, n):
        mg = E.ViewMerger(n, V, CLASSES, DEV, num_crop=crops)
        E.final_test(batches, m, None, None, merger=mg)
        return mg
    single = run(b, nvid)
    local = run([b[0], b[2]] if c.rank == 0 else [dup, b[1], b[3]], nvid)
    g = local.gather()
    assert set(g.index) == set(single.index) and g.N == nvid

    def summed(mg):
        total, count = torch.empty(mg.N, CLASSES, device=DEV), torch.empty(mg.N, dtype=torch.int32, device=DEV)
        K.view_sum(mg.view_logits, mg.seen, total, count)
        return total, count
    (tg, cg), (ts, cs) = summed(g), summed(single)
    for vid, i in single.index.items():
        j = g.index[vid]
        c.bits(g.view_logits[j], single.view_logits[i], f"merge: view logits of {vid}")
        c.bits(tg[j], ts[i], f"merge: summed logits of {vid}")
        assert int(cg[j]) == int(cs[i]) == V and int(g.labels[j]) == int(single.labels[i]) == label[vid]
    assert g.result() == single.result(), (g.result(), single.result())
    if c.rank == 1:  # the duplicate was this rank's first line of its key, and holds other logits than rank 0's line
        vid, ch, sp, _ = lines[0]
        mine, kept = local.view_logits[local.index[vid], ch * crops + sp], g.view_logits[g.index[vid], ch * crops + sp]
        assert not torch.equal(mine, kept)
    c.all_equal(g.view_logits, "the gathered merger's view logits")
    c.say("merge: gather() equals the single-process merger", g.result())


# ================================================================================================ 9. averaged weights (--ema)
def check_ema(c):
    """rank r is built from init seed 11 + r and makes its ModelEma BEFORE the step object: behind _join every rank's average is a
    bit copy of rank 0's masters, and it stays equal across the ranks over two updating steps on distinct shards (no exchange of
    its own); ranks that disagree on the decay all raise"""
    torch, F = c.torch, c.F
    m = c.model(load=False, init_seed=11 + c.rank)
    ema = F.ModelEma(m, decay=0.99)
    first = [torch.zeros(1, dtype=torch.int64, device=DEV) for _ in range(c.world)]
    c.dist.all_gather(first, ema.checksum().reshape(1))
    assert int(first[0]) != int(first[1]), "the test's replicas start equal"
    step, opt = c.stepper(m, clip_grad=1.0, model_ema=ema)
    assert opt.ema is not None and opt.ema[0] is ema.flat
    torch.cuda.synchronize()
    cs, master = int(ema.checksum()), int(step.replicas_checksum())
    c.say(f"EMA after _join: checksum {cs} master {master} built-from {int(first[c.rank])}")
    c.all_equal(ema.checksum().reshape(1), "ModelEma.checksum() after _join")
    c.bits(ema.flat, m.store.flat, "the average after _join against the broadcast masters")
    assert cs == master == int(first[0]), (cs, master, int(first[0]))
    for k in range(2):
        out = step.step(c.clips(2, 950 + 10 * k + c.rank), c.labels(2, 960 + 10 * k + c.rank))
        assert out["grad_norm"] is not None
    torch.cuda.synchronize()
    c.say(f"EMA after 2 updating steps: checksum {int(ema.checksum())} master {int(step.replicas_checksum())}")
    c.all_equal(ema.checksum().reshape(1), "ModelEma.checksum() after two updating steps")
    c.all_equal(ema.flat, "the average after two updating steps")
    c.all_equal(m.store.flat, "the masters after two updating steps")
    assert int(ema.checksum()) != cs and not torch.equal(ema.flat, m.store.flat)
    m2 = c.model()
    try:
        c.stepper(m2, model_ema=F.ModelEma(m2, decay=0.99 if c.rank == 0 else 0.999))
    except RuntimeError as e:
        assert "differs between the ranks" in str(e) and "ModelEma" in str(e)
        c.say("EMA_MISMATCH_RAISED")
    else:
        raise AssertionError("ranks with different ModelEma decays were accepted")


# ================================================================================================ 10. optimizers (--opt sgd)
def check_optimizers(c):
    """rank 0 built with FusedTorchAdamW, rank 1 with FusedTorchSGD over the same groups: both raise from the agreement, neither
    is left in a collective; two ranks with SGD that differ in `nesterov` raise too"""
    F = c.F
    for what in ("kind", "nesterov"):
        m = c.model()
        try:
            if what == "kind":
                c.stepper(m, opt="adamw" if c.rank == 0 else "sgd")
            else:
                opt = F.FusedTorchSGD(F.param_groups(m, WD, LAYER_DECAY), m.store, lr=SGD_LR, momentum=SGD_MOMENTUM, nesterov=c.rank == 0, model=m)
                F.FinetuneStep(m, opt)
        except RuntimeError as e:
            assert "differs between the ranks" in str(e) and "the optimizer's kind" in str(e), str(e)
            c.say(f"OPTIMIZER_MISMATCH_RAISED ({what})")
        else:
            raise AssertionError(f"ranks with different optimizers ({what}) were accepted")
    t = c.torch.ones(1, device=DEV)
    c.dist.all_reduce(t)  # the group is still usable
    assert float(t) == c.world


# ================================================================================================ 11. the overflow guard (--guard)
def check_guard(c):
    """the decision is taken behind the all-reduce, so a NaN in ONE rank's shard skips the update on EVERY rank, with no
    collective of its own; ranks that disagree about skip_nonfinite raise from the agreement"""
    torch = c.torch
    m = c.model()
    step, opt = c.stepper(m, clip_grad=1.0, skip_nonfinite=True)
    start = int(step.replicas_checksum())
    sums = []
    for k in range(3):
        clip = c.clips(2, 700 + 10 * k + c.rank)
        if k == 1 and c.rank == 1:
            clip[0, 1, 2, 3, 4] = float("nan")
        before = int(step.replicas_checksum())
        out = step.step(clip, c.labels(2, 800 + 10 * k + c.rank))
        c.all_equal(step.replicas_checksum().reshape(1), f"replicas_checksum after call {k + 1}")
        c.all_equal(out["grad_norm"].reshape(1), f"grad_norm of call {k + 1}")
        now = int(step.replicas_checksum())
        assert math.isfinite(float(out["grad_norm"])) == (k != 1) and (now == before) == (k == 1), (k, float(out["grad_norm"]), now, before)
        sums.append(now)
    c.all_equal(step.skipped, "the skip counter")
    state = torch.stack([bitsum(c, t) for t in (m.store.flat, m.store.m, m.store.v) if t is not None])
    c.all_equal(state, "parameters and optimizer state after 3 calls")
    assert bool(torch.isfinite(m.store.flat).all()) and bool(torch.isfinite(m.store.m).all()) and sums[-1] != start
    assert int(step.skipped.item()) == 1 and int(opt.step_dev.item()) == 2
    c.say(f"guard: skipped {int(step.skipped.item())}, replicas equal after every call, finite state at the end")
    try:
        c.stepper(c.model(), skip_nonfinite=c.rank == 0)
    except RuntimeError as e:
        assert "differs between the ranks" in str(e) and "skip_nonfinite" in str(e), str(e)
        c.say("GUARD_MISMATCH_RAISED")
    else:
        raise AssertionError("a guarded rank beside an unguarded one was accepted")
    t = torch.ones(1, device=DEV)
    c.dist.all_reduce(t)  # the group is still usable
    assert float(t) == c.world


# ================================================================================================ driver
def worker(rank, world, port, checks, q, opt="adamw"):
    try:
        sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        early = None
        if "seeds" in checks:  # a model built BEFORE the process group exists (check_seeds)
            import v1_downstream_synth as S
            from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
            early = VisionTransformer(num_classes=CLASSES, drop_path_rate=0.1, **S.TINY)
            early.load_state_dict(S.synth_state(S.TINY, 61, CLASSES), strict=True)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        c = Ctx(rank, world, early, opt)
        for name in checks:
            globals()["check_" + name](c)
            torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, True, ""))
    except BaseException:
        q.put((rank, False, traceback.format_exc()))
        raise


def main(argv):
    with_ema, argv = "--ema" in argv, [a for a in argv if a != "--ema"]
    with_guard, argv = "--guard" in argv, [a for a in argv if a != "--guard"]
    opt = "adamw"
    if "--opt" in argv:
        i = argv.index("--opt")
        if i + 1 >= len(argv) or argv[i + 1] not in ("adamw", "sgd"):
            raise SystemExit("--opt adamw | sgd")
        opt, argv = argv[i + 1], argv[:i] + argv[i + 2:]
    every = list(CHECKS) if opt == "adamw" else [n for n in CHECKS if n not in ADAMW_ONLY] + ["optimizers"]
    checks = argv + ["ema"] if with_ema else argv or every
    if with_guard:
        checks = (argv + ["ema"] if with_ema else argv) + ["guard"]
    bad = [n for n in checks if n not in CHECKS + OPTIONAL]
    if bad:
        raise SystemExit(f"unknown check {bad}: one of {CHECKS}")
    if opt == "sgd" and any(n in ADAMW_ONLY for n in checks):
        raise SystemExit(f"--opt sgd: {ADAMW_ONLY} hold AdamW to a bound of its own and do not run under SGD")
    world, port = 2, free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, checks, q, opt)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    done, failed = 0, None
    while done < world and failed is None:
        try:
            rank, ok, msg = q.get(timeout=0.2)
            done += 1
            if not ok:
                failed = f"rank {rank} failed:\n{msg}"
        except queue.Empty:
            dead = [p for p in procs if p.exitcode not in (None, 0)]
            if dead:
                failed = f"a rank ended with exit code {dead[0].exitcode} and no report"
    if failed is not None:  # the other rank may be waiting in a collective for the one that failed: end it, do not wait for it
        for p in procs:
            if p.is_alive():
                p.terminate()
    for p in procs:
        p.join()
    if failed is not None:
        print(failed, flush=True)
        raise SystemExit(1)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    print("DIST_FINETUNE_OK " + " ".join(checks))


if __name__ == "__main__":
    main(sys.argv[1:])
