"""The host side of the v1 fine-tuning step across ranks (no GPU): the meter merge of validation_one_epoch over two gloo ranks on
CPU tensors against a restatement of the reference's SmoothedValue (utils.py:22-78: count / total in double,
synchronize_between_processes, global_avg), and the argument refusals of FinetuneStep.

Run as a script (`python tests/test_v1_finetune_dist_cpu.py RANK PORT CASE`) this file is one rank of the two-rank test."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# per rank: the batches as (top-1 hits, top-5 hits, batch size, loss).  "two_ranks": rank 1 has two short batches, both all right --
# 50 % by samples, 62.5 % by batches.  "empty": rank 1 has no batch
CASES = {"two_ranks": [[(3, 7, 8, 1.25), (5, 8, 8, 0.8125)], [(1, 6, 8, 2.0625), (3, 3, 3, 0.4375), (3, 3, 3, 0.1)]],
         "empty": [[(3, 7, 8, 1.25)], []]}


class SmoothedValue:
    """the two fields of the reference's meter that global_avg reads, and what synchronize_between_processes does to them"""

    def __init__(self):
        self.count, self.total = 0, 0.0

    def update(self, value, n=1):
        self.count += n
        self.total += value * n

    @staticmethod
    def synchronized(meters):
        """all_reduce(SUM) of [count, total] in float64, count back to int (utils.py:49-60)"""
        out = SmoothedValue()
        t = np.zeros(2, dtype=np.float64)
        for m in meters:
            t = t + np.array([m.count, m.total], dtype=np.float64)
        out.count, out.total = int(t[0]), float(t[1])
        return out

    @property
    def global_avg(self):
        return self.total / self.count


def reference(per_rank):
    """validation_one_epoch's meters (engine_for_finetuning.py:163-170) rank by rank, then synchronised"""
    meters = {k: [] for k in ("loss", "acc1", "acc5")}
    for batches in per_rank:
        m = {k: SmoothedValue() for k in meters}
        for h1, h5, n, loss in batches:
            m["loss"].update(loss)  # (metric_logger.update(loss=...): n = 1)
            m["acc1"].update(float(np.float32(h1) * np.float32(100.0 / n)), n=n)  # utils.accuracy's fp32 percentage
            m["acc5"].update(float(np.float32(h5) * np.float32(100.0 / n)), n=n)
        for k in meters:
            meters[k].append(m[k])
    return {k: SmoothedValue.synchronized(v).global_avg for k, v in meters.items()}


def totals(batches):
    from tvts_amd.downstream.evaluate_v1 import meter_totals
    if not batches:
        return (0.0, 0.0, 0.0, 0.0, 0.0)  # what _Scores.totals hands over for a rank whose loader gave nothing
    return meter_totals([b[0] for b in batches], [b[1] for b in batches], [b[2] for b in batches], [b[3] for b in batches])


def rank_main(rank, port, case):
    """one of the two ranks: the merge over gloo on CPU tensors -> one JSON line"""
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from tvts_amd.downstream.evaluate_v1 import sync_meters
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        out = dict(result=sync_meters(totals(CASES[case][rank])))
    except ValueError as e:
        out = dict(error=str(e))
    dist.barrier()  # (both ranks are out of the exchange, whatever it returned)
    dist.destroy_process_group()
    print("RESULT " + json.dumps(out), flush=True)


def two_ranks(case):
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), str(r), str(port), case], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, cwd=ROOT) for r in range(2)]
    outs = []
    for p in procs:
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, so[-2000:] + se[-2000:]
        outs.append(json.loads([l for l in so.splitlines() if l.startswith("RESULT ")][-1][7:]))
    return outs


def test_meter_merge_over_two_gloo_ranks_matches_smoothed_value():
    from tvts_amd.downstream.evaluate_v1 import merge_meters
    per_rank = CASES["two_ranks"]
    want = reference(per_rank)
    # the host function alone: per-rank tuples in, dict out
    got = merge_meters([totals(b) for b in per_rank])
    outs = two_ranks("two_ranks")
    assert outs[0] == outs[1], outs  # every rank returns the same numbers
    for res in (got, outs[0]["result"]):
        assert set(res) == {"loss", "acc1", "acc5"}
        for k in want:
            assert abs(res[k] - want[k]) <= 1e-12 * abs(want[k]), (k, res[k], want[k])
    # weighted by samples over all ranks, not by batches and not by ranks; the loss by batches
    rows = [b for r in per_rank for b in r]
    assert abs(want["acc1"] - 100.0 * sum(b[0] for b in rows) / sum(b[2] for b in rows)) < 1e-4
    assert abs(want["acc1"] - np.mean([100.0 * b[0] / b[2] for b in rows])) > 1.0
    assert abs(want["loss"] - np.mean([b[3] for b in rows])) < 1e-12
    assert abs(want["loss"] - np.mean([np.mean([b[3] for b in r]) for r in per_rank])) > 1e-3


def test_rank_without_a_batch_is_refused_on_every_rank():
    from tvts_amd.downstream.evaluate_v1 import merge_meters
    with pytest.raises(ValueError, match="gave no batch on rank 1"):
        merge_meters([totals(b) for b in CASES["empty"]])
    with pytest.raises(ValueError, match="one .* tuple per rank"):
        merge_meters([])
    outs = two_ranks("empty")
    assert all("gave no batch on rank 1" in o.get("error", "") for o in outs), outs


def test_finetune_step_argument_refusals():
    """both are refused in front of anything that touches the model or the device"""
    from tvts_amd.downstream.finetune_v1 import FinetuneStep
    with pytest.raises(ValueError, match="payload 'fp16': expected 'fp32' or 'bf16'"):
        FinetuneStep(None, None, payload="fp16")
    with pytest.raises(RuntimeError, match="data_parallel=True needs an initialised torch.distributed process group"):
        FinetuneStep(None, None, data_parallel=True)
    from tvts_amd.downstream.evaluate_v1 import validation_one_epoch
    with pytest.raises(RuntimeError, match="sync=True needs an initialised torch.distributed process group"):
        validation_one_epoch([], None, sync=True)


if __name__ == "__main__":
    rank_main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
