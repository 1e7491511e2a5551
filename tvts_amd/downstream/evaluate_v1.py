"""Scoring a fine-tuned v1 classifier on the reference's protocol: the evaluation half of v1/downstream/run_class_finetuning.py /
run_class_linear.py (engine_for_finetuning.py:142-285; the test views of ssv2.py:65-83,132-164) over the HIP engine.

    stats = validation_one_epoch(val_loader, model)                                # after every epoch: {"loss", "acc1", "acc5"}

    views = TestViews(input_size=224, short_side_size=224, test_num_segment=2, test_num_crop=3)
    merger = ViewMerger(num_videos, views.per_video, num_classes=174, device=model.store.device, num_crop=views.test_num_crop)
    stats = final_test(test_loader, model, None, file, views=views, merger=merger)  # batches: (frames_u8, target, ids)
    top1, top5 = merger.result()                                                   # per video, in percent

Validation: per batch the model's forward, tvts_soft_ce (labels, smoothing 0, no gradient) and tvts_class_ranks; every per-batch
result stays on the device and the host synchronises once, at the end.  The reference's averaging is kept: acc1 / acc5 are its
per-batch percentages weighted by the batch size (`meters[...].update(v, n=batch_size)`), ``loss`` is the PLAIN mean of the batch
means (`update(loss=...)` counts every batch once, so a short last batch weighs as much as a full one).

Test: with ``views=`` a batch carries uint8 SOURCE clips [Bs, Tsrc, H0, W0, 3], resized to the short side by the host; the
test_num_segment x test_num_crop views of every clip -- `buffer[chunk::2, start:start + short_side_size]` -- are formed inside the
tubelet gather (tvts_patch_gather_tube_u8_view) from ONE upload, no view is materialised.  The view logits land in the merger's
device buffer (tvts_view_store: the first line of a (video, chunk, split) wins, as merge's `continue`, :251-252);
``ViewMerger.result`` sums a video's views in a fixed order (tvts_view_sum) and ranks the label (tvts_class_ranks).  compute_video
takes the mean (:277): mean and sum rank identically, the division is left out.  Ties resolve towards the lower class index
(np.argmax's rule; the reference's top-5 `np.argsort(-feat)[:5]` leaves the order of equal logits to the sort).
``merge(eval_path, num_tasks)`` is the host drop-in that reads the per-rank files, for multi-process runs.

Several ranks (one process per GPU, torch.distributed initialised).  ``validation_one_epoch(loader, model, sync=None)``: after the
local loop ONE float64 all-reduce carries every rank's [sum acc1_b n_b, sum acc5_b n_b, sum n_b, sum loss_b, batches]
(dist.gather_rows: a [W, 5] table in which a rank fills its own row, so every rank sums the rows in rank order and returns the same
bits) and ``merge_meters`` -- a host function, per-rank tuples in, dict out -- does what
``SmoothedValue.synchronize_between_processes`` followed by ``global_avg`` does (utils.py:49-60): acc1 / acc5 weighted by sample
count over all ranks, loss the plain mean over all batches of all ranks.  A rank whose loader gave no batch is refused on every
rank.  ``ViewMerger.gather()``: merge without the files -- every rank contributes its seen slots (compact logits, labels, the
host keys (video id, chunk, split)), every rank rebuilds the union by ``add``-ing the contributions in rank order, and
tvts_view_store's first-line-wins rule resolves DistributedSampler's padding duplicates as the reference does with rank 0's file
read first; the caller runs ``merger.gather().result()``.  The per-rank file + ``merge`` path works as before.

Logits are the engine's fp32 (bf16 operands, fp32 accumulation).  The reference runs the model under fp16 autocast (:159,198): its
logits, and the loss computed from them, carry fp16 rounding that is not reproduced here.

OUT OF SCOPE (not built here): decoding, the short-side resize in front of the views (cv2 / PIL work on the host beside decoding, as
RandAugment is for training), the fp16 autocast rounding of the logits, and ``ModelEma`` (the scripts only save it and never
evaluate it).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import dist as D
from .. import hip as K


# ---------------------------------------------------------------------------------------------- meters
def _meter_avg(hits, sizes):
    """utils.accuracy + SmoothedValue.global_avg (engine_for_finetuning.py:163-168): per batch the fp32 percentage hits * (100 / n),
    then sum(value * n) / sum(n) in double"""
    total = sum(float(np.float32(h) * np.float32(100.0 / n)) * n for h, n in zip(hits, sizes))
    return total / sum(sizes)


def _labels(target, C):
    """the batch's labels, checked on the host (they are unchecked device data for the kernels) -> int32 tensor on the host"""
    t = torch.as_tensor(target)
    if t.dim() != 1 or t.is_floating_point() or t.numel() < 1:
        raise ValueError(f"target: integer labels [B], got {t.dtype} {tuple(t.shape)}")
    if int(t.min()) < 0 or int(t.max()) >= C:
        raise IndexError(f"labels must lie in [0, {C})")
    return t.to("cpu", torch.int32).contiguous()


class _Scores:
    """the device-side meters of one evaluation loop: per batch a loss cell and the label ranks, read back once"""

    def __init__(self, model):
        if model.num_classes <= 0:
            raise ValueError("evaluation needs a model with a head (num_classes > 0)")
        self.C, self.dev = model.num_classes, model.store.device
        self.loss, self.ranks, self.sizes = [], [], []

    def add(self, logits, labels_dev):
        B = logits.shape[0]
        cell = torch.empty(1, dtype=torch.float32, device=self.dev)
        K.zero_(cell)
        K.soft_ce(logits, cell, torch.empty(2 * B, dtype=torch.float32, device=self.dev), labels=labels_dev, smoothing=0.0)
        self.loss.append(cell)
        self.ranks.append(K.class_ranks(logits, labels_dev))
        self.sizes.append(B)

    def _read(self):
        """-> (loss per batch in double, top-1 hits per batch, top-5 hits per batch); the one synchronisation of the loop"""
        loss = torch.cat(self.loss).cpu().numpy().astype(np.float64)
        ranks = torch.cat(self.ranks).cpu().numpy()
        ends = np.cumsum(self.sizes)
        h1 = [int((ranks[e - n:e] < 1).sum()) for e, n in zip(ends, self.sizes)]
        h5 = [int((ranks[e - n:e] < 5).sum()) for e, n in zip(ends, self.sizes)]
        return loss, h1, h5

    def result(self):
        """-> ({"loss", "acc1", "acc5"}, (acc1, acc5) of the last batch); the one synchronisation of the loop"""
        if not self.sizes:
            raise ValueError("the data loader gave no batch")
        loss, h1, h5 = self._read()
        last = tuple(float(np.float32(h[-1]) * np.float32(100.0 / self.sizes[-1])) for h in (h1, h5))
        return dict(loss=float(loss.mean()), acc1=_meter_avg(h1, self.sizes), acc5=_meter_avg(h5, self.sizes)), last

    def totals(self):
        """this rank's meters as meter_totals() states them; a rank without a batch gives five zeros (it still has to enter the
        exchange, where merge_meters refuses it on every rank)"""
        if not self.sizes:
            return (0.0, 0.0, 0.0, 0.0, 0.0)
        loss, h1, h5 = self._read()
        return meter_totals(h1, h5, self.sizes, loss)


def meter_totals(h1, h5, sizes, loss):
    """one rank's SmoothedValue state after its loop, as (sum acc1_b n_b, sum acc5_b n_b, sum n_b, sum loss_b, batches): acc_b is
    the batch's fp32 percentage hits * (100 / n) (utils.accuracy), `total += value * n` and `count += n` run in Python doubles
    (utils.py:33-36); the loss meter counts every batch once"""
    a1 = sum(float(np.float32(h) * np.float32(100.0 / n)) * n for h, n in zip(h1, sizes))
    a5 = sum(float(np.float32(h) * np.float32(100.0 / n)) * n for h, n in zip(h5, sizes))
    return (a1, a5, float(sum(sizes)), float(sum(float(v) for v in loss)), float(len(sizes)))


def merge_meters(per_rank):
    """SmoothedValue.synchronize_between_processes followed by global_avg (utils.py:49-60,76-78) on the host: per_rank is one
    meter_totals() tuple per rank, in rank order -> {"loss", "acc1", "acc5"}.  count and total are summed over the ranks in
    double, in rank order; acc1 / acc5 = total / count with count the SAMPLES of all ranks, loss = total / count with count the
    BATCHES of all ranks.  A rank without a batch is refused, as the single-process loop refuses an empty loader (in the
    reference that rank has no meter to synchronise and fails alone)."""
    rows = [tuple(float(v) for v in r) for r in per_rank]
    if not rows or any(len(r) != 5 for r in rows):
        raise ValueError("per_rank: one (sum acc1 n, sum acc5 n, sum n, sum loss, batches) tuple per rank")
    empty = [i for i, r in enumerate(rows) if r[4] <= 0 or r[2] <= 0]
    if empty:
        raise ValueError(f"the data loader gave no batch on rank {empty[0]}")
    tot = [0.0] * 5
    for r in rows:
        tot = [t + v for t, v in zip(tot, r)]
    return dict(loss=tot[3] / tot[4], acc1=tot[0] / tot[2], acc5=tot[1] / tot[2])


def sync_meters(totals):
    """this rank's meter_totals() -> the merged {"loss", "acc1", "acc5"}, the same on every rank: ONE float64 all-reduce carries the
    five numbers of every rank (dist.gather_rows), merge_meters does the arithmetic"""
    return merge_meters(D.gather_rows(torch.tensor([float(v) for v in totals], dtype=torch.float64)).tolist())


def _use_ranks(sync):
    """sync None: on with more than one rank.  True without a process group is refused"""
    if sync and not (D.dist.is_available() and D.dist.is_initialized()):
        raise RuntimeError("sync=True needs an initialised torch.distributed process group")
    return D.world()[0] > 1 and (sync is None or bool(sync))


@torch.no_grad()
def validation_one_epoch(data_loader, model, device=None, sync=None):
    """engine_for_finetuning.py:142-174 -> {"loss", "acc1", "acc5"} (the reference's keys).  A batch is (videos, target, ...):
    videos fp32 [B, 3, T, H, W] or uint8 [B, T, H0, W0, 3] (centre crop and normalisation on the device), target integer [B].
    acc1 / acc5 in percent, weighted by batch size; loss the unweighted mean of the batch means (the reference's meters).  Nothing
    synchronises with the host until the loader is exhausted.  The logits are the engine's fp32: the reference computes them, and
    the loss, under fp16 autocast.  device: accepted for the reference's signature; the model's device is used.
    sync: None -- with more than one rank of torch.distributed the meters are merged over the ranks after the local loop
    (`metric_logger.synchronize_between_processes()`, :170: sync_meters, one float64 all-reduce) and every rank returns the same
    numbers -- acc1 / acc5 weighted by sample count over all ranks, loss the plain mean over all batches of all ranks; False --
    this rank's own numbers."""
    ranks = _use_ranks(sync)
    model.eval()
    sc = _Scores(model)
    for batch in data_loader:
        labels = _labels(batch[1], sc.C)
        logits = model(batch[0])
        if logits.shape[0] != labels.numel():
            raise ValueError(f"{labels.numel()} labels for {logits.shape[0]} clips")
        sc.add(logits, labels.to(sc.dev))
    if ranks:
        return sync_meters(sc.totals())
    return sc.result()[0]


# ---------------------------------------------------------------------------------------------- test views
class ViewPlan:
    """the views of one batch of source clips, on the host: view_i int32 [B, 8] = (src, t0, tstep, top, left, 0, 0, 0), the table of
    tvts_patch_gather_tube_u8_view (include/tvts_hip.h); video / chunk / split int32 [B]: the source clip of the batch and the
    (chunk_nb, split_nb) of every sample; T: the frames per view.  len(plan) = B."""

    def __init__(self, view_i, video, chunk, split, T):
        self.view_i, self.video, self.chunk, self.split, self.T = view_i, video, chunk, split, int(T)

    def __len__(self):
        return int(self.view_i.shape[0])


class TestViews:
    """The view arithmetic of SSVideoClsDataset in mode 'test' (ssv2.py:74-83,151-160) on clips that are already resized to the
    short side: view (chunk_nb, split_nb) of a clip buffer [Tsrc, H0, W0, 3] is
    `buffer[chunk_nb::2, start:start + short_side_size]` along the LONGER side (the height when H0 >= W0), with
    start = int(split_nb * spatial_step) and spatial_step = 1.0 * (max(H0, W0) - short_side_size) / (test_num_crop - 1).
    Refused: short_side_size != input_size (the view would not be input_size x input_size), test_num_crop < 2 (the reference
    divides by test_num_crop - 1 = 0 at ssv2.py:151-152), and in ``plan`` a min(H0, W0) that is not short_side_size and a
    test_num_segment whose views differ in length (`chunk_nb::2` gives equal lengths for chunks 0 and 1 of an even Tsrc only)."""
    __test__ = False  # (not a pytest class)

    def __init__(self, input_size=224, short_side_size=224, test_num_segment=2, test_num_crop=3):
        if short_side_size != input_size:
            raise ValueError(f"short_side_size {short_side_size} != input_size {input_size}: the views would not be input_size x input_size")
        if test_num_crop < 2:
            raise ValueError("test_num_crop < 2: the reference divides by test_num_crop - 1 (ssv2.py:151-152)")
        if test_num_segment < 1 or input_size < 1:
            raise ValueError("test_num_segment >= 1 and input_size >= 1")
        self.input_size, self.short_side_size = int(input_size), int(short_side_size)
        self.test_num_segment, self.test_num_crop = int(test_num_segment), int(test_num_crop)

    @property
    def per_video(self):
        return self.test_num_segment * self.test_num_crop

    def slot(self, chunk, split):
        """the view's place among a video's test_num_segment x test_num_crop views"""
        return chunk * self.test_num_crop + split

    def plan(self, Bs, Tsrc, H0, W0, chunk_nb=None, split_nb=None) -> ViewPlan:
        """the views of Bs source clips [Tsrc, H0, W0, 3].  chunk_nb / split_nb None: every view of every clip, clip-major, then
        chunk, then crop (Bs * per_video samples); given (one entry per clip): that one view of every clip (Bs samples)."""
        S, seg, crop = self.short_side_size, self.test_num_segment, self.test_num_crop
        if Bs < 1 or Tsrc < 1:
            raise ValueError("Bs >= 1 and Tsrc >= 1")
        if min(H0, W0) != S:
            raise ValueError(f"source frames {H0} x {W0}: the short side must be short_side_size = {S} (the resize is the host's)")
        lens = {len(range(c, Tsrc, 2)) for c in range(seg)}
        if len(lens) != 1 or 0 in lens:
            raise ValueError(f"test_num_segment = {seg} over {Tsrc} frames: `chunk::2` gives views of {sorted(lens)} frames "
                             "(equal lengths only for chunks 0 and 1 of an even frame count)")
        if (chunk_nb is None) != (split_nb is None):
            raise ValueError("chunk_nb and split_nb: both or neither")
        if chunk_nb is None:
            video = np.repeat(np.arange(Bs), seg * crop)
            chunk = np.tile(np.repeat(np.arange(seg), crop), Bs)
            split = np.tile(np.arange(crop), Bs * seg)
        else:
            chunk, split = np.asarray(chunk_nb).astype(np.int64).reshape(-1), np.asarray(split_nb).astype(np.int64).reshape(-1)
            if chunk.shape != (Bs,) or split.shape != (Bs,):
                raise ValueError(f"chunk_nb / split_nb: one entry per clip ({Bs})")
            if ((chunk < 0) | (chunk >= seg)).any() or ((split < 0) | (split >= crop)).any():
                raise ValueError(f"chunk_nb in [0, {seg}) and split_nb in [0, {crop})")
            video = np.arange(Bs)
        spatial_step = 1.0 * (max(H0, W0) - S) / (crop - 1)                   # ssv2.py:151-152
        view_i = np.zeros((len(video), 8), dtype=np.int32)
        view_i[:, 0], view_i[:, 1], view_i[:, 2] = video, chunk, 2           # temporal_start = chunk_nb, `temporal_start::2` (:153,156)
        start = np.array([int(s * spatial_step) for s in split.tolist()])    # (:154)
        view_i[:, 3 if H0 >= W0 else 4] = start                              # (:155-160)
        return ViewPlan(view_i, video.astype(np.int32), chunk.astype(np.int32), split.astype(np.int32), lens.pop())


# ---------------------------------------------------------------------------------------------- per-video merge on the device
class ViewMerger:
    """merge + compute_video (engine_for_finetuning.py:231-285) without the files: view_logits fp32 [N, V, C], seen uint8 [N, V] and
    labels int32 [N] on the device, filled by ``final_test(..., merger=m)``.  A video is known by its id; ids take the rows
    0 .. N - 1 in first-seen order (a host dictionary).  num_crop: the crops per segment, which places (chunk, split) at view
    chunk * num_crop + split."""

    def __init__(self, num_videos, views_per_video, num_classes, device, num_crop=3):
        if num_videos < 1 or views_per_video < 1 or num_classes < 1 or num_crop < 1 or views_per_video % num_crop:
            raise ValueError("num_videos, num_classes >= 1 and views_per_video a positive multiple of num_crop")
        self.N, self.V, self.C, self.num_crop, self.dev = int(num_videos), int(views_per_video), int(num_classes), int(num_crop), device
        self.view_logits = torch.empty(self.N, self.V, self.C, dtype=torch.float32, device=device)
        self.seen = torch.empty(self.N, self.V, dtype=torch.uint8, device=device)
        self.labels = torch.empty(self.N, dtype=torch.int32, device=device)
        for t in (self.view_logits, self.seen, self.labels):
            K.zero_(t)
        self.index = {}

    def index_of(self, video_id):
        i = self.index.get(video_id)
        if i is None:
            if len(self.index) >= self.N:
                raise IndexError(f"more than {self.N} different video ids")
            i = self.index[video_id] = len(self.index)
        return i

    def add(self, logits, labels_dev, ids, chunk, split):
        """one batch: logits fp32 [B, C] and labels int32 [B] on the device; ids, chunk, split: B host values each"""
        if logits.shape[1] != self.C:
            raise ValueError(f"logits of {logits.shape[1]} classes, the merger holds {self.C}")
        slot = np.empty(len(ids), dtype=np.int32)
        for b, (vid, c, s) in enumerate(zip(ids, chunk, split)):
            c, s = int(c), int(s)
            if not (0 <= s < self.num_crop and 0 <= c * self.num_crop + s < self.V):
                raise ValueError(f"view (chunk {c}, split {s}) outside the {self.V // self.num_crop} x {self.num_crop} views of a video")
            slot[b] = self.index_of(vid) * self.V + c * self.num_crop + s
        K.view_store(logits, torch.from_numpy(slot).to(self.dev), labels_dev, self.view_logits, self.seen, self.labels)

    def gather(self):
        """-> a ViewMerger that holds the views of EVERY rank, the same on every rank: merge (:231-270) without the files.  Each rank
        contributes only its seen slots -- compact logits [n_seen, C] and labels, and the host keys (video id, chunk, split) --
        and every rank rebuilds the union by ``add``-ing the contributions in rank order 0 .. W - 1, so tvts_view_store applies
        merge's rule unchanged: the first line of a (video, chunk, split) wins, rank 0's lines read first (the duplicates
        DistributedSampler pads the last batch with resolve as in the reference).  Video rows are assigned from the gathered keys
        in that order; the per-rank first-seen dictionaries differ and are not reused.  One rank: a copy of this merger's views."""
        W, _ = D.world()
        seen = self.seen.cpu().numpy().reshape(-1)
        slots = np.flatnonzero(seen)
        ids = {i: vid for vid, i in self.index.items()}
        keys = [(ids[int(s) // self.V], (int(s) % self.V) // self.num_crop, (int(s) % self.V) % self.num_crop) for s in slots]
        sl = torch.from_numpy(slots.astype(np.int64)).to(self.dev)
        logits = self.view_logits.view(self.N * self.V, self.C).index_select(0, sl)
        labels = self.labels.index_select(0, sl // self.V)
        if W == 1:
            parts = [(keys, logits, labels)]
        else:
            every = [None] * W
            D.dist.all_gather_object(every, keys)
            rows = max(1, max(len(k) for k in every))  # (every rank sends tensors of the longest contribution's size)
            lg = torch.zeros(rows, self.C, dtype=torch.float32, device=self.dev)
            lb = torch.zeros(rows, dtype=torch.int32, device=self.dev)
            lg[:len(keys)].copy_(logits)
            lb[:len(keys)].copy_(labels)
            all_lg = [torch.empty_like(lg) for _ in range(W)]
            all_lb = [torch.empty_like(lb) for _ in range(W)]
            D.dist.all_gather(all_lg, lg)
            D.dist.all_gather(all_lb, lb)
            parts = [(k, a[:len(k)], b[:len(k)]) for k, a, b in zip(every, all_lg, all_lb)]
        videos = {k[0] for ks, _, _ in parts for k in ks}
        out = ViewMerger(max(1, len(videos)), self.V, self.C, self.dev, num_crop=self.num_crop)
        for ks, lg, lb in parts:
            if ks:
                out.add(lg.contiguous(), lb.contiguous(), [k[0] for k in ks], [k[1] for k in ks], [k[2] for k in ks])
        return out

    def result(self):
        """-> (top1 * 100, top5 * 100) over the videos that have a view, as merge returns them (:265-270)"""
        total, count = torch.empty(self.N, self.C, dtype=torch.float32, device=self.dev), torch.empty(self.N, dtype=torch.int32, device=self.dev)
        K.view_sum(self.view_logits, self.seen, total, count)
        both = torch.stack([K.class_ranks(total, self.labels), count]).cpu().numpy()
        ranks = both[0][both[1] > 0]
        if ranks.size == 0:
            raise ValueError("no video has a view")
        return float(np.mean((ranks < 1) * 1.0)) * 100, float(np.mean((ranks < 5) * 1.0)) * 100


# ---------------------------------------------------------------------------------------------- final test
def _host_list(x):
    return x.tolist() if hasattr(x, "tolist") else list(x)


@torch.no_grad()
def final_test(data_loader, model, device, file, views=None, merger=None):
    """engine_for_finetuning.py:177-228 -> {"loss", "acc1", "acc5"} over the VIEWS (the reference's meters, as
    validation_one_epoch).  views None: a batch is the reference's (videos, target, ids, chunk_nb, split_nb) with clips that are
    cropped already (fp32 [B, 3, T, H, W] or uint8 [B, T, H, W, 3]).  views a TestViews: a batch is (frames_u8 [Bs, Tsrc, H0, W0, 3],
    target [Bs], ids [Bs]) and every view of every clip is formed inside the gather from the one upload, clip-major, then chunk,
    then crop.  file: the reference's text file -- first line "{acc1}, {acc5}" of the LAST batch (the reference writes the two
    tensors left over from its loop there, :220; ``merge`` skips the line), then one line per view `id [logits] label chunk split`;
    None: no file, and the logits never leave the device.  merger: a ViewMerger that takes every view's logits."""
    model.eval()
    sc = _Scores(model)
    lines, kept = [], []
    for batch in data_loader:
        ids = _host_list(batch[2])
        if views is None:
            labels = _labels(batch[1], sc.C)
            chunk, split = [int(c) for c in _host_list(batch[3])], [int(s) for s in _host_list(batch[4])]
            logits = model(batch[0])
            vids = ids
        else:
            frames = batch[0]
            if frames.dim() != 5:
                raise ValueError(f"frames: uint8 source clips [Bs, Tsrc, H0, W0, 3], got {tuple(frames.shape)}")
            plan = views.plan(*frames.shape[:4])
            target = _labels(batch[1], sc.C)
            if target.numel() != frames.shape[0] or len(ids) != frames.shape[0]:
                raise ValueError(f"target and ids: one entry per source clip ({frames.shape[0]})")
            labels = target[torch.from_numpy(plan.video.astype(np.int64))].contiguous()
            logits = model.forward_views(frames, plan.view_i, plan.T)
            vids, chunk, split = [ids[v] for v in plan.video.tolist()], plan.chunk.tolist(), plan.split.tolist()
        B = logits.shape[0]
        if not (labels.numel() == len(vids) == len(chunk) == len(split) == B):
            raise ValueError(f"batch of {B} views with {labels.numel()} labels, {len(vids)} ids, {len(chunk)} chunk and {len(split)} split numbers")
        labels_dev = labels.to(sc.dev)
        sc.add(logits, labels_dev)
        if merger is not None:
            merger.add(logits, labels_dev, vids, chunk, split)
        if file is not None:
            kept.append(logits)
            lines.append((vids, labels.tolist(), chunk, split))
    stats, last = sc.result()
    if file is not None:
        rows = torch.cat(kept).cpu().numpy()
        with open(file, "w") as f:
            f.write("{}, {}\n".format(*last))
            r = 0
            for vids, labs, chunk, split in lines:
                for vid, lab, c, s in zip(vids, labs, chunk, split):
                    f.write("{} {} {} {} {}\n".format(vid, str(rows[r].tolist()), str(int(lab)), str(int(c)), str(int(s))))
                    r += 1
    return stats


# ---------------------------------------------------------------------------------------------- host merge of the per-rank files
def compute_video(data, label):
    """compute_video (:273-284) on one video's view logits -> (pred, top1, top5) or None without a view: float64 mean, np.argmax,
    membership among the first five of np.argsort(-mean)"""
    if len(data) == 0:
        return None
    feat = np.mean(np.asarray(data, dtype=np.float64), axis=0)
    pred = int(np.argmax(feat))
    return pred, (pred == int(label)) * 1.0, (int(label) in np.argsort(-feat)[:5]) * 1.0


def merge(eval_path, num_tasks):
    """engine_for_finetuning.py:231-270: reads `<eval_path>/<rank>.txt` for rank 0 .. num_tasks - 1 as final_test wrote them, keeps
    the first line of every (video, chunk, split), -> (top1 * 100, top5 * 100) over the videos.  The arithmetic is the
    reference's (float64; its `np.float` is `float`), in one plain loop instead of a 64-process pool."""
    feats, label, pos = {}, {}, {}
    for x in range(num_tasks):
        with open(os.path.join(eval_path, str(x) + ".txt"), "r") as f:
            lines = f.readlines()[1:]
        for line in lines:
            line = line.strip()
            if not line:
                continue
            name = line.split("[")[0]
            tail = line.split("]")[1].split(" ")
            lab, chunk_nb, split_nb = tail[1], tail[2], tail[3]
            data = np.array([float(v) for v in line.split("[")[1].split("]")[0].split(",")], dtype=np.float64)
            if name not in feats:
                feats[name], label[name], pos[name] = [], 0, []
            if chunk_nb + split_nb in pos[name]:
                continue
            feats[name].append(data)
            pos[name].append(chunk_nb + split_nb)
            label[name] = lab
    ans = [compute_video(feats[name], label[name]) for name in feats]
    ans = [a for a in ans if a is not None]
    if not ans:
        raise ValueError("no view lines in the files")
    return float(np.mean([a[1] for a in ans])) * 100, float(np.mean([a[2] for a in ans])) * 100
