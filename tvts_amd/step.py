"""One TVTSv2 pretrain step (v2/trainer/trainer.py:463-512) on the HIP engine, without autograd.

zero_grad -> model forward -> all-gather of embeddings -> sim_matrix + InfoNCE (+ 2*CE sorting loss) ->
hand-written backward (gradients all-reduced range by range while it runs) -> fused HF-AdamW.
Optional, both decided on the device: the global gradient norm with its clip coefficient in front of the update (clip_grad) and the
overflow guard that skips a step whose norm is not finite (skip_nonfinite).
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import dist as D
from . import hip as K
from .engine import LossHead


def guard_options(clip_grad, skip_nonfinite, *, fused: bool, ranged: bool, optimizer: str = "the optimizer"):
    """The two options of StepRunner as it keeps them -> (clip_grad or None, skip_nonfinite), or the named refusal: a max_norm that
    is not a positive finite number; either option with an optimizer that is not the fused one; either option together with the
    ranged update."""
    clip = float(clip_grad) if clip_grad else None
    skip = bool(skip_nonfinite)
    if clip is not None and not (0.0 < clip < float("inf")):
        raise ValueError(f"StepRunner: clip_grad {clip_grad!r} must be a positive finite max_norm (None switches clipping off)")
    what = " / ".join(n for n, on in (("clip_grad", clip is not None), ("skip_nonfinite", skip)) if on)
    if what and not fused:
        raise RuntimeError(f"StepRunner({what}) needs the fused optimizer (FusedHFAdamW): the norm, the coefficient and the "
                           f"guard's decision stay on the device; got {optimizer}")
    if what and ranged:
        raise RuntimeError(f"StepRunner({what}) cannot be combined with adamw_ranges / TVTS_ADAMW_RANGES=1: a ranged update "
                           "starts before the last gradient exists, the global gradient norm only behind the whole backward")
    return clip, skip


def micro_batch_option(micro_batches, *, fused: bool = True, ranged: bool = False, family=None, optimizer: str = "the optimizer") -> int:
    """StepRunner's micro_batches as it keeps it (an int >= 1), or the named refusal: anything that is not such an int; and, for
    n > 1, an optimizer that is not the fused one, the ranged update, the v1 engine."""
    n = micro_batches
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"StepRunner: micro_batches {micro_batches!r} must be an int >= 1 (1: the unsplit step)")
    if n == 1:
        return n
    if family == "v1":
        raise NotImplementedError(f"StepRunner(micro_batches={n}) is not built for the v1 engine: its text dropout seed advances with "
                                  "every forward, so a second forward does not reproduce the first, and it has no forward-only encoders")
    if not fused:
        raise RuntimeError(f"StepRunner(micro_batches={n}) needs the fused optimizer (FusedHFAdamW): one update behind the last "
                           f"chunk's backward, the gradient scale folded into its launch; got {optimizer}")
    if ranged:
        raise RuntimeError(f"StepRunner(micro_batches={n}) cannot be combined with adamw_ranges / TVTS_ADAMW_RANGES=1: a ranged update "
                           "starts before the last chunk's gradient exists")
    return n


# the per-clip fields of the reference batch dict, sliced by clip; "text" is transcript-major and handled apart
_PER_CLIP = ("video", "keep_ind", "crop", "label")


def split_batch(data: dict, n: int):
    """The reference batch dict of B clips -> n dicts of b = B / n clips, chunk k holding the clips [k * b, (k + 1) * b).
    text is TRANSCRIPT-major (row t * B + b, what prepare_batch and the model's reshape(NT, B, -1) read): chunk rows are
    text.reshape(NT, B, L)[:, lo:hi], never a contiguous slice of rows.  video (fp32 or the uint8 wire format), keep_ind [B, n],
    crop [B, 2] and label are sliced by clip; keep_ind [1, n] and resize are kept; a device-drawn mask keeps mask_seed and moves
    sample_offset by lo (tvts_tube_mask numbers the samples globally); everything else (meta, ...) is carried through untouched.
    A LIST video (the ragged uint8 wire format) is sliced by clip as well, each chunk planned by its own prepare_batch, and every
    chunk gets num_frames = the whole batch's T."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"split_batch: n {n!r} must be an int >= 1")
    video = data["video"]
    ragged = isinstance(video, (list, tuple))  # (the ragged uint8 wire format: B clips [T_b, Hs_b, Ws_b, 3], sliced by clip)
    if not ragged and video.dim() < 4:
        raise ValueError(f"split_batch: video {tuple(video.shape)} has no clip dimension")
    B = len(video) if ragged else int(video.shape[0])
    if ragged:
        if B < 1:
            raise ValueError("split_batch: video is an empty list of clips")
        if any(not torch.is_tensor(c) or c.dim() != 4 for c in video):
            raise ValueError("split_batch: a list video holds uint8 clips [T, Hs, Ws, 3]")
        T = int(data["num_frames"]) if data.get("num_frames") is not None else max(int(c.shape[0]) for c in video)
    if B % n:
        raise ValueError(f"split_batch: micro_batches {n} does not divide the batch of {B} clips (unequal chunks are not built)")
    b = B // n
    text = data["text"]
    if text.dim() != 2 or text.shape[0] == 0 or text.shape[0] % B:
        raise ValueError(f"split_batch: text {tuple(text.shape)}: expected n_trans * {B} token rows (transcript-major)")
    NT, L = text.shape[0] // B, text.shape[1]
    for key in _PER_CLIP[1:]:
        t = data.get(key)
        if torch.is_tensor(t) and not (key == "keep_ind" and t.shape[0] == 1) and (t.dim() == 0 or t.shape[0] != B):
            raise ValueError(f"split_batch: {key} {tuple(t.shape)} is not per clip (expected {B} rows)")
    out = []
    for k in range(n):
        lo, hi = k * b, (k + 1) * b
        d = {}
        for key, val in data.items():
            if key == "text":
                d[key] = text.reshape(NT, B, L)[:, lo:hi].reshape(NT * b, L)
            elif key in _PER_CLIP and torch.is_tensor(val) and not (key == "keep_ind" and val.shape[0] == 1):
                d[key] = val[lo:hi]
            elif key == "video" and ragged:
                d[key] = list(val[lo:hi])
            elif key == "sample_offset":
                continue
            else:
                d[key] = val
        if "mask_seed" in data and "keep_ind" not in data:
            d["sample_offset"] = int(data.get("sample_offset", 0)) + lo
        elif "sample_offset" in data:
            d["sample_offset"] = data["sample_offset"]
        if ragged:  # every chunk pads its short clips to the WHOLE batch's T, so the chunks agree on the token rows per clip
            d["num_frames"] = T
        out.append(d)
    return out


class StepRunner:
    def __init__(self, model, optimizer, loss_head: Optional[LossHead] = None, clip_grad: Optional[float] = None,
                 skip_nonfinite: bool = False, micro_batches: int = 1):
        """clip_grad (max_norm of torch.nn.utils.clip_grad_norm_ over the trainable tensors, None / 0: off) and skip_nonfinite (the
        overflow guard: a step whose global gradient norm is not finite changes no bit of the weights, the moments, the shadows or
        the e4m3 scales, and counts in ``skipped``) are both decided on the device: tvts_grad_sumsq behind the gradient exchange
        leaves norm and coefficient in ``norm_coef``, FusedHFAdamW reads them there.  The norm is that of the AVERAGED gradient,
        the number clip_grad_norm_ sees behind DDP, and every rank computes it from the same reduced buffer: no collective is
        added.  With both off the step is launch for launch the one without these arguments.
        micro_batches = n > 1: the step of a batch of B clips from n chunks of B / n, with the InfoNCE over the WHOLE
        batch -- every chunk forward once for its [b, E] embeddings (two [B, E] caches), one gather + loss + dE over all rows, then
        each chunk forward again and backward with its rows of dE into the same gradient buffer; one exchange, one update.  The
        activations held are those of one chunk.  1: launch for launch the unsplit step."""
        self.model, self.opt = model, optimizer
        self.eng, self.store = model.engine, model.store
        self.head = loss_head or LossHead(self.store.device)
        self.sync = D.GradSync(self.store.grad)
        self.fused = hasattr(optimizer, "chunk_group")
        self.eng.grad_ready = self.sync.reduce_range if (self.sync.W > 1 or self.sync.native) else None
        self.gather = D.EmbedGather()
        # OPT-IN (arch["adamw_ranges"] / TVTS_ADAMW_RANGES=1): the fused optimizer's update range by range beside the backward
        # (FusedHFAdamW.step_range), each range as soon as its gradient is final.  Built for the reference's per-GPU batches, where
        # the single AdamW launch + the transposes are 1.0 of 15.6 ms, and MEASURED SLOWER at every batch (profiles/r05_adamw_ranges.txt:
        # 12 / 24 / 192 pairs 757 / 987 / 1354 pairs/s with it against 774 / 1022 / 1363 without): an HBM-bound 4.7 GB pass takes the
        # bandwidth and the CUs it runs on away from the backward it was meant to hide under, and its ~18 fork edges cost the replayed
        # graph what the r04 side-stream experiments already showed.  Same bits either way (tests/test_bench_path_gpu.py).
        self.ranged = self.fused and hasattr(optimizer, "step_range") and bool(self.eng.arch.get("adamw_ranges", os.environ.get("TVTS_ADAMW_RANGES", "0") == "1"))
        # exchange diagnostics (bench.py at world > 1, eager launches only): event pairs on the compute stream around the two places where
        # it waits for a collective -- {"gather": [...], "allreduce": [...]} when switched on, None otherwise
        self.diag = None
        self.clip_grad, self.skip_nonfinite = guard_options(clip_grad, skip_nonfinite, fused=self.fused and hasattr(optimizer, "begin_ranges"),
                                                            ranged=self.ranged, optimizer=type(optimizer).__name__)
        self.guarding = self.clip_grad is not None or self.skip_nonfinite
        self.micro_batches = micro_batch_option(micro_batches, fused=self.fused, ranged=self.ranged, family=self.eng.arch.get("family"),
                                                optimizer=type(optimizer).__name__)
        self.micro_observer = None  # optional callback(k, text_emb, video_emb) behind chunk k's second forward (tests: cache identity)
        self._emb_cache = None      # the two [B, E] fp32 embedding caches of the micro-batched step (text, video), grown on demand
        # every rank enters this, with or without the options: a rank that guards beside one that does not would skip alone
        # (only where a process group exists: the check is a collective)
        if D.dist.is_available() and D.dist.is_initialized():
            D.agree(repr(("clip_grad", self.clip_grad, "skip_nonfinite", self.skip_nonfinite)).encode(),
                    "StepRunner: clip_grad or skip_nonfinite")
            # (a rank that splits beside one that does not would run the same collectives, but a chunk count is part of what the
            # ranks must have in common: the batch each one hands over has to divide by it)
            D.agree(repr(("micro_batches", self.micro_batches)).encode(), "StepRunner: micro_batches")
            # (the packed and the padded v1 text tower round differently: ranks that disagree would average gradients of two models)
            D.agree(repr(("text_unpadded", bool(getattr(self.eng, "text_unpadded", False)))).encode(), "StepRunner: arch['text_unpadded']")
        if self.guarding:
            dev = self.store.device
            self.norm_coef = torch.zeros(2, dtype=torch.float32, device=dev)  # [global norm, clip coefficient] of the last step
            self._partial = torch.zeros(optimizer.chunk_group.numel(), dtype=torch.float32, device=dev)
            optimizer.norm_coef = self.norm_coef

    @property
    def skipped(self):
        """the optimizer's device int64 counter of the steps the overflow guard skipped (never read on the host by the step)"""
        return self.opt.skipped

    def _bracket(self, key, fn):
        """fn() between two events of the current stream when the diagnostics are on: the elapsed time is what the compute stream
        spent WAITING there (the exposed part of the collective), since fn only enqueues waits and small copies"""
        if self.diag is None or torch.cuda.is_current_stream_capturing():
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.diag.setdefault(key, []).append((e0, e1))
        return out

    def losses_and_grads(self, pb, te, ve, pred, labels):
        B = pb["B"]
        vg, tg = self._bracket("gather", self.gather.result)  # started by the engine before the sort head ran
        loss1, dv_all, dt_all = self.head.contrastive(vg, tg)
        if pred is not None:
            loss2, dpred = self.head.sorting(pred, labels)
        else:
            loss2, dpred = None, None
        return loss1, loss2, D.local_rows(dt_all, B), D.local_rows(dv_all, B), dpred

    MAX_STEPS_IN_FLIGHT = 2

    def _throttle(self):
        """The host may run at most MAX_STEPS_IN_FLIGHT steps ahead of the device.  With page-locked input batches nothing else holds
        it back: every batch it prepares ahead is a fresh device copy of the clip tensor (925 MB of fp32 at 192 pairs) waiting for its
        step, and the allocator grows -- and synchronises -- to hold them (measured: the 192-pair trainer epoch 4 % slower from pinned
        than from pageable memory).  Called at the top of a step; the step's own event is recorded by _stepped()."""
        q = self.__dict__.setdefault("_inflight", [])
        while len(q) >= self.MAX_STEPS_IN_FLIGHT:
            q.pop(0).synchronize()

    def _stepped(self):
        if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            ev = torch.cuda.Event()
            ev.record()
            self.__dict__.setdefault("_inflight", []).append(ev)

    def step(self, data: dict, device_step: bool = False, pb=None):
        out = self._step(data, device_step, pb)
        self._stepped()
        return out

    def _step(self, data: dict, device_step: bool = False, pb=None):
        self._throttle()
        m = self.model
        if hasattr(self.eng, "training"):  # v1: DistilBERT's dropout follows the module's train() / eval() flag
            self.eng.training = bool(m.training)
        m._fresh_shadows()
        m._sync_requires_grad()
        if self.micro_batches > 1:
            if pb is not None:
                raise ValueError("StepRunner(micro_batches > 1).step prepares its chunks itself: pass the batch dict, not a prepared batch")
            chunks = split_batch(data, self.micro_batches)
            pbs = [self.eng.prepare_batch(c) for c in chunks]  # once: both passes run on the same masks and index tables
            return self.run_micro(pbs, [self._labels(c, p) for c, p in zip(chunks, pbs)], device_step)
        if pb is None:
            pb = self.eng.prepare_batch(data)
        return self.run(pb, self._labels(data, pb), device_step)

    def _labels(self, data, pb):
        """int32 device labels of the sorting loss: prepare_batch stages them with the batch's other index tensors (v2 engine)"""
        if pb["NT"] == 1 or "label" not in data:
            return None
        if pb.get("labels") is not None:
            return pb["labels"]
        return data["label"].reshape(-1).to(torch.int32).to(self.store.device)

    def run(self, pb, labels, device_step=False):
        """The device-side part of the step (capturable in a hipGraph when world == 1)."""
        if self.sync.W > 1:
            D._apply_cu_reservation(pb["B"] * pb["S"])  # (decided once, from the first batch's token rows per GPU)
        K.zero_(self.store.grad)
        self.sync.bytes_sent = 0
        self.eng.embeds_ready = self.gather.start  # only the training step gathers; eval / autograd forwards do not
        try:
            te, ve, pred = self.eng.forward(pb)
        finally:
            self.eng.embeds_ready = None
        loss1, loss2, d_te, d_ve, dpred = self.losses_and_grads(pb, te, ve, pred, labels)
        if self.ranged:
            self.opt.grad_scale = 1.0 / self.sync.W
            self.opt.begin_ranges(device_step=device_step)
            self.eng.param_ready = self.opt.step_range
        try:
            self.eng.backward(d_te, d_ve, dpred)
        finally:
            self.eng.param_ready = None
        return self._update(loss1, loss2, device_step)

    def _caches(self, B, E):
        c = self._emb_cache
        if c is None or c[0].shape[0] < B or c[0].shape[1] != E:
            c = self._emb_cache = tuple(torch.empty(B, E, dtype=torch.float32, device=self.store.device) for _ in range(2))
        return c[0][:B], c[1][:B]

    def run_micro(self, pbs, labels, device_step=False):
        """The device-side part of the micro-batched step: pbs / labels are the chunks' prepared batches and sorting
        labels, in clip order.  Pass 1 is the training forward without the sort head (the forward-only video encoder runs the last
        block's CLS tail and the full-frame SPACE kernel of its own: not the training forward's bits), so its last chunk, run with
        the sort head, is also pass 2's first forward."""
        eng, n = self.eng, len(pbs)
        b, E = pbs[0]["B"], eng.arch["embed"]
        if any(p["B"] != b for p in pbs):
            raise ValueError("StepRunner.run_micro: chunks of unequal size")
        B = n * b
        if self.sync.W > 1:
            D._apply_cu_reservation(b * pbs[0]["S"])
        self.sync.bytes_sent = 0
        t_cache, v_cache = self._caches(B, E)
        fwd = None
        for k, pb in enumerate(pbs):  # pass 1: embeddings only (embeds_ready stays unarmed: the gather is of the whole batch's rows)
            fwd = eng.forward(pb, sort_head=(k == n - 1))
            t_cache[k * b:(k + 1) * b].copy_(fwd[0])
            v_cache[k * b:(k + 1) * b].copy_(fwd[1])
        self.gather.start(t_cache, v_cache)
        vg, tg = self._bracket("gather", self.gather.result)
        loss1, dv_all, dt_all = self.head.contrastive(vg, tg)
        d_te, d_ve = D.local_rows(dt_all, B), D.local_rows(dv_all, B)
        ready, eng.grad_ready = eng.grad_ready, None  # the range exchange is armed for the last backward only: an earlier
        loss2 = None                                  # all-reduce would sum partial gradients in place
        K.zero_(self.store.grad)
        try:
            for i, k in enumerate([n - 1] + list(range(n - 1))):  # pass 2, starting with the chunk whose forward is still held
                pb = pbs[k]
                te, ve, pred = fwd if i == 0 else eng.forward(pb)
                if self.micro_observer is not None:
                    self.micro_observer(k, te, ve)
                dpred = None
                if pred is not None:
                    loss2, dpred = self.head.sorting(pred, labels[k], scale=2.0 / n, add=i > 0)
                if i == n - 1:
                    eng.grad_ready = ready
                eng.backward(d_te[k * b:(k + 1) * b], d_ve[k * b:(k + 1) * b], dpred)
        finally:
            eng.grad_ready = ready
        return self._update(loss1, loss2, device_step)

    def _update(self, loss1, loss2, device_step):
        """Behind the (last) backward, once per step: the e4m3 scales, the end of the gradient exchange, the norm when guarding, the
        optimizer."""
        if hasattr(self.eng, "end_step") and not self.skip_nonfinite:
            self.eng.end_step()  # (e4m3 weight gradients: this step's amax values become the next step's per-tensor scales)
        scale = self._bracket("allreduce", self.sync.finish)
        if self.guarding:
            # the norm of the averaged gradient over the trainable chunks (frozen chunks carry group 255, the kernel's exclusion
            # rule) and the coefficient: one more read of the gradient buffer, everything stays on the device
            K.grad_sumsq(self.store.grad, self.opt.chunk_group, self._partial, self.norm_coef, max_norm=self.clip_grad, grad_scale=scale)
            if self.skip_nonfinite and hasattr(self.eng, "end_step"):
                self.eng.end_step(guard_norm=self.norm_coef)  # (behind the norm: a skipped step keeps the e4m3 scales as well)
            self.opt.grad_scale = scale
            self.opt.step(device_step=device_step, guard=self.skip_nonfinite)
            return dict(loss1=loss1, loss2=loss2, grad_norm=self.norm_coef[0])
        if self.fused:
            self.opt.grad_scale = scale
            self.opt.step(device_step=device_step)
        else:
            if scale != 1.0:
                self.store.grad.mul_(scale)
            self.model._install_grads()
            self.opt.step()
        return dict(loss1=loss1, loss2=loss2)


def _map_tensors(x, fn):
    """fn over every tensor of a (nested) batch structure; everything else is kept"""
    if torch.is_tensor(x):
        return fn(x)
    if isinstance(x, dict):
        return {k: _map_tensors(v, fn) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x)(_map_tensors(v, fn) for v in x)
    return x


def _signature(x):
    if torch.is_tensor(x):
        return ("t", tuple(x.shape), str(x.dtype))
    if isinstance(x, dict):
        return tuple((k, _signature(v)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(_signature(v) for v in x)
    return x if isinstance(x, (int, float, bool, str, type(None))) else type(x).__name__


def _copy_into(dst, src):
    if torch.is_tensor(dst):
        dst.copy_(src, non_blocking=True)
    elif isinstance(dst, dict):
        for k in dst:
            _copy_into(dst[k], src[k])
    elif isinstance(dst, (tuple, list)):
        for d, s_ in zip(dst, src):
            _copy_into(d, s_)


class GraphReplay:
    """The trainer loop's step as a replayed hipGraph (what bench.py does with its two resident batches, for batches that ARRIVE):
    one graph per batch signature -- the shapes and types of everything prepare_batch hands the device step; the reference's loop
    alternates a YT-Temporal and a WebVid loader (v2/trainer/trainer.py:463), i.e. two signatures, a last partial batch makes a third.

    A signature's first step runs eagerly (its workspaces are allocated there), its second is captured over device-side COPIES of the
    batch's tensors, and from then on a step is: prepare_batch (host-to-device on the engine's copy stream, under the previous step)
    -> device-to-device copy into the captured buffers (on the compute stream, i.e. behind the previous replay: 0.3 ms for a
    192-pair fp32 clip tensor) -> replay.  The learning rate and weight decay travel through FusedHFAdamW.sync_hyper (read by the
    captured AdamW launch from device memory), the step counter lives on the device.  Same launches, same order, same bits as the
    eager step (tests/test_trainer_gpu.py::test_graph_replay_in_the_trainer_loop_is_the_eager_loop).

    World 1 with the fused optimizer only (a captured multi-rank step has never run on hardware: bench.py keeps it opt-in too);
    anything else, and any failure to capture, falls back to StepRunner.step for good.  OPT-IN (TVTS_TRAINER_GRAPH=1): with
    prepare_batch free of synchronising copies the eager loop already keeps the device busy back to back, and the replayed loop
    measures 1 % (192 pairs) to 3 - 4 % (12 pairs) SLOWER than it (profiles/r06_bench_product_path*.txt)."""

    MAX_SIGNATURES = 6

    def __init__(self, runner: StepRunner):
        self.r = runner
        self.cache = {}
        # (skip_nonfinite: the guarded optimizer launch refuses a stream capture, so such a runner steps eagerly; clip_grad alone is
        # capturable -- the coefficient is a device scalar the replayed launches read; micro_batches > 1: the micro-batched step has
        # never been captured, such a runner steps eagerly as well)
        self.usable = (torch.cuda.is_available() and runner.fused and not runner.ranged and runner.sync.W == 1 and not runner.sync.native
                       and not runner.skip_nonfinite and runner.micro_batches == 1 and os.environ.get("TVTS_TRAINER_GRAPH", "0") == "1")
        self.replays = self.captures = self.eager = 0

    def step(self, data: dict):
        r = self.r
        if not self.usable:
            self.eager += 1
            return r.step(data)
        out = self._step(data)
        r._stepped()
        return out

    def _step(self, data: dict):
        r = self.r
        r._throttle()
        m = r.model
        if hasattr(r.eng, "training"):
            r.eng.training = bool(m.training)
        m._fresh_shadows()
        m._sync_requires_grad()
        pb = r.eng.prepare_batch(data)
        labels = r._labels(data, pb)
        if pb.get("seq_start") is not None or pb.get("gather") is not None:
            # packed captions (arch["text_packed"]): M and max_len change with every batch, a graph would never be replayed -- eager;
            # ragged uint8 clips (pb["gather"]): the packed buffer's size changes with every batch, eager as well
            self.eager += 1
            return r.run(pb, labels, device_step=True)
        sig = (_signature(pb), None if labels is None else tuple(labels.shape), bool(m.training),
               hash(tuple(r.eng.requires_grad.values())) if hasattr(r.eng, "requires_grad") else None,
               getattr(r.eng, "recompute", "none"), r.micro_batches)  # (a graph holds the launches of the mode it was captured in)
        ent = self.cache.get(sig)
        if ent is None:
            if len(self.cache) >= self.MAX_SIGNATURES:
                self.cache.pop(next(iter(self.cache)))
            self.cache[sig] = dict(graph=None)
            self.eager += 1
            return r.run(pb, labels, device_step=True)   # first sight: eager (allocates this signature's workspaces)
        self.cache[sig] = self.cache.pop(sig)            # most recently used last
        if ent["graph"] is None:
            try:
                ent["pb"] = _map_tensors(pb, lambda t: t.clone())
                ent["labels"] = None if labels is None else labels.clone()
                r.opt.sync_hyper()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    ent["out"] = r.run(ent["pb"], ent["labels"], device_step=True)
                ent["graph"] = g
                self.captures += 1
            except Exception as e:  # stay correct: eager from here on
                import warnings
                warnings.warn(f"hipGraph capture of the training step failed ({type(e).__name__}: {e}); the trainer continues with eager steps")
                self.usable = False
                self.cache.clear()
                torch.cuda.synchronize()
                self.eager += 1
                return r.run(pb, labels, device_step=True)
        else:
            _copy_into(ent["pb"], pb)
            if labels is not None:
                ent["labels"].copy_(labels, non_blocking=True)
            r.opt.global_step += 1  # (the replayed AdamW advances the DEVICE counter; the capture itself advanced the host's once)
        r.opt.sync_hyper()
        ent["graph"].replay()
        self.replays += 1
        return ent["out"]
