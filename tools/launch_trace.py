"""Launch trace of the engine: one line per call into tvts_amd.hip (name; every tensor argument as shape : dtype : strides @ first-seen
buffer index + byte offset; every scalar / keyword argument, defaults applied; scratch lane) over fixed scenarios on synthetic weights,
and a SHA-256 per scenario.  Equal traces = the same launches on the same buffers in the same order; run it at two commits and diff.
Without a GPU the wrappers record and do not call through (the same trace; no kernel runs).
    python tools/launch_trace.py [--out DIR]      # DIR/<scenario>.txt; the hashes go to stdout"""
import argparse
import hashlib
import inspect
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import tvts_oracle as O, tvts_v1_oracle as V  # noqa: E402
from tvts_amd import arch as A, hip as K  # noqa: E402
from tvts_amd.engine import Engine, ParamStore  # noqa: E402
from tvts_amd.engine_v1 import EngineV1  # noqa: E402
from tvts_amd.model._common import pack_captions  # noqa: E402

DRY = not torch.cuda.is_available()
DEV = torch.device("cpu" if DRY else "cuda:0")
HOST_SIDE = ("token_sort", "quantize_fp8_multi_table")  # no launch: the engine uses what they return
LINES, BUFS, ALIVE, DEPTH, LANE = [], {}, [], [0], K.current_lane


def desc(v):
    if isinstance(v, torch.Tensor):
        base = v.untyped_storage().data_ptr()
        if base not in BUFS:
            BUFS[base] = len(BUFS)
            ALIVE.append(v)  # (a freed buffer's address could come back as another buffer's)
        return f"{tuple(v.shape)}:{str(v.dtype)[6:]}:{v.stride()}@{BUFS[base]}+{v.data_ptr() - base}"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}={desc(x)}" for k, x in v.items()) + "}"
    if isinstance(v, (tuple, list)):
        return "[" + ", ".join(desc(x) for x in v) + "]"
    return repr(v)


def record(name, fn, through, args_of):
    def wrapped(*a, **k):
        if DEPTH[0] == 0:  # (what one wrapper calls inside another is that launch's own business)
            LINES.append(f"{name}({args_of(*a, **k)}) lane={LANE()}")
        DEPTH[0] += 1
        try:
            return fn(*a, **k) if through else None
        finally:
            DEPTH[0] -= 1
    return wrapped


def bound(sig):
    def args_of(*a, **k):
        b = sig.bind(*a, **k)
        b.apply_defaults()
        return ", ".join(f"{p}={desc(x)}" for p, x in b.arguments.items())
    return args_of


def install():
    for name, fn in list(vars(K).items()):
        if inspect.isfunction(fn) and not name.startswith("_") and fn.__module__ == K.__name__ and fn is not LANE:
            setattr(K, name, record(name, fn, not DRY or name in HOST_SIDE, bound(inspect.signature(fn))))
    K.TnGroup.run = record("TnGroup.run", K.TnGroup.run, not DRY, lambda self: desc(self.keep))
    if DRY:  # no device: a plan is its problems, and there is nothing for streams and events to order
        K.TnGroup.__init__ = lambda self, problems, workspace, splits=0: setattr(self, "keep", problems)
        stub = type("Stub", (), dict(__init__=lambda self, *a, **k: None, __enter__=lambda self: self, __exit__=lambda self, *e: False))
        stub.wait_stream = stub.wait_event = stub.record = stub.synchronize = lambda self, *a: None
        torch.cuda.Stream = torch.cuda.Event = torch.cuda.stream = stub
        torch.cuda.current_stream = lambda *a: stub()


def engine(arch, params, cls=Engine):
    store = ParamStore(arch, DEV)
    for k, v in params.items():
        store.p(k).copy_(v)
    store.refresh_shadows()
    return cls(store)


def train(arch, steps=1, v1=False, n_trans=None, training=True, between=None):
    """between(eng): called between two steps (what runs there must leave the next step's launches and buffers alone)"""
    mod = V if v1 else O
    eng = engine(arch, mod.synth_params(arch, seed=5), EngineV1 if v1 else Engine)
    eng.training = training  # (read by the v1 engine only: False = the text tower's dropout off)
    batch = mod.synth_batch(arch, B=4, T=4, seed=6, n_trans=n_trans, caption_len=11)
    for i in range(steps):
        if i and between is not None:
            between(eng)
        te, ve, pred = eng.forward(eng.prepare_batch(batch))
        d_pred = None if pred is None else torch.full_like(pred, 0.01)  # (one transcript per clip: no sorting loss)
        eng.backward(torch.full_like(te, 0.01), torch.full_like(ve, 0.01), d_pred)
        eng.end_step()


def enc_video():
    for arch in (A.small_arch(sort_head=False), A.small_arch_h(sort_head=False)):  # the B tail and the pooled tail
        eng = engine(arch, O.synth_params(arch, seed=5))
        b = O.synth_batch(arch, B=3, T=4, seed=7, n_trans=1)
        keep = b["keep_ind"].to(DEV, torch.int32).contiguous()
        frames = torch.randint(0, 256, (3, 4, arch["image"], arch["image"], 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
        eng.encode_video(b["video"].to(DEV), keep, 3, 4)
        eng.encode_video(frames.to(DEV), keep, 3, 4)


def enc_text():
    arch = A.small_arch(sort_head=False)
    eng = engine(arch, O.synth_params(arch, seed=5))
    g = torch.Generator().manual_seed(9)
    ids = torch.zeros(6, arch["context"], dtype=torch.int64)
    for r, cl in enumerate((5, 9, 11, 7, 16, 9)):  # captions of mixed lengths: start token, cl - 2 words, EOT (the largest id)
        ids[r, 0], ids[r, cl - 1] = arch["vocab"] - 2, arch["vocab"] - 1
        ids[r, 1:cl - 1] = torch.randint(1, arch["vocab"] - 2, (cl - 2,), generator=g)
    eot = ids.argmax(-1)
    L, N = int(eot.max()) + 1, ids.shape[0]
    rows, ids_dev = (torch.arange(N) * L + eot).to(torch.int32).to(DEV), ids[:, :L].to(torch.int32).contiguous().to(DEV)
    eng.encode_text(ids_dev, rows, N, L, eot_index=(None, eot.to(torch.int32).to(DEV)))
    eng.encode_text(ids_dev, rows, N, L)
    packed, seq_start, _, max_len = pack_captions(ids, eot)
    eng.encode_text_packed(packed.to(DEV), seq_start.to(DEV), N, max_len)


def v1_video_calls(eng, arch):
    """every input form of EngineV1.encode_video at B = 3, T = 4"""
    B, T, tubes, img = 3, 4, 4 // arch["tubelet"], arch["image"]
    b = V.synth_batch(arch, B=B, T=T, seed=7, n_trans=1)
    keep = b["keep_ind"].to(DEV, torch.int32).contiguous()
    g = torch.Generator().manual_seed(8)
    frames = torch.randint(0, 256, (B, T, img + 16, img + 32, 3), generator=g, dtype=torch.uint8).to(DEV)
    crop = torch.stack([torch.randint(0, 17, (B,), generator=g), torch.randint(0, 33, (B,), generator=g)], 1).to(torch.int32).to(DEV)
    clip = b["video"].to(DEV)
    eng.encode_video(clip, keep, B, tubes)
    eng.encode_video(clip.permute(0, 2, 1, 3, 4).contiguous(), keep, B, tubes, channel_major=True)
    eng.encode_video(frames, keep, B, tubes)  # (crop None: the centre crop)
    eng.encode_video(frames, keep, B, tubes, crop=crop)
    eng.encode_video(clip, keep, B, tubes, project=False)
    ppf = (img // arch["patch"]) ** 2
    eng.encode_video(clip, torch.arange(ppf, dtype=torch.int32).expand(B, tubes, ppf).contiguous().to(DEV), B, tubes)


def v1_captions(arch):
    """N = 6 right-padded captions of enc_text's lengths ([CLS], words, [SEP]) -> the arguments of EngineV1.encode_text"""
    g, lens = torch.Generator().manual_seed(9), torch.tensor((5, 9, 11, 7, 16, 9))
    N, L = lens.numel(), int(lens.max())
    ids = torch.zeros(N, L, dtype=torch.int64)
    for r, cl in enumerate(lens.tolist()):
        ids[r, 0], ids[r, cl - 1] = arch["vocab"] - 2, arch["vocab"] - 1
        ids[r, 1:cl - 1] = torch.randint(1, arch["vocab"] - 2, (cl - 2,), generator=g)
    return ids.to(torch.int32).to(DEV), lens.to(torch.int32).to(DEV), N, L


def enc_v1_video():
    arch = A.small_arch_v1()
    v1_video_calls(engine(arch, V.synth_params(arch, seed=5), EngineV1), arch)


def enc_v1_text():
    arch = A.small_arch_v1()
    eng = engine(arch, V.synth_params(arch, seed=5), EngineV1)
    halves, caps = [], v1_captions(arch)
    for eng.training in (True, False):  # an encoder call never applies dropout: the same launches either way
        n = len(LINES)
        eng.encode_text(*caps)
        halves.append(LINES[n:])
    assert halves[0] == halves[1], "encode_text depends on engine.training"


def train_v1_enc_train():
    """an encoder call of either tower between two steps: the second step's lines show the first step's buffers"""
    arch = A.small_arch_v1()
    train(arch, steps=2, v1=True, between=lambda eng: (eng.encode_text(*v1_captions(arch)), v1_video_calls(eng, arch)))


SCENARIOS = {
    "train-small": lambda: train(A.small_arch()),
    "train-small-fp32": lambda: train(A.small_arch(hybrid_stream=False)),
    "train-h-tiny": lambda: train(A.small_arch_h(tn_grouped=True)),  # (grouped weight gradients on: TnGroup.run is in the trace)
    "train-fp8": lambda: train(A.small_arch(fp8_wgrad=True), steps=2),  # calibration step, end_step(), tensor-mode step
    "train-v1": lambda: train(A.small_arch_v1(), v1=True),
    "train-dense-last": lambda: train(A.small_arch(sort_used_rows_only=False, text_used_rows_only=False)),  # last blocks on every row
    "train-wgrad-side": lambda: train(A.small_arch(wgrad_stream=True)),
    "train-fp8-dgrad": lambda: train(A.small_arch(fp8=True, fp8_dgrad=True)),  # per-token e4m3 with input gradients
    "train-h-fp32": lambda: train(A.small_arch_h(hybrid_stream=False)),  # the two non-hybrid pooled tails
    "train-h-bf16res": lambda: train(A.small_arch_h(bf16_residual=True)),
    "train-nt1": lambda: train(A.small_arch(), n_trans=1),  # no sort head: pred is None
    "train-h-nt1": lambda: train(A.small_arch_h(), n_trans=1),  # ... and the pooled tail then has no token gradient
    "train-v1-dense": lambda: train(A.small_arch_v1(sort_used_rows_only=False), v1=True),
    "enc-video": enc_video,
    "enc-text": enc_text,
    "enc-v1-video": enc_v1_video,
    "enc-v1-text": enc_v1_text,
    "train-v1-eval": lambda: train(A.small_arch_v1(), v1=True, training=False),  # the dp == 0 branches of _pln_fwd / _pln_bwd
    "train-v1-enc-train": train_v1_enc_train,
}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for one trace file per scenario")
    args = ap.parse_args()
    install()
    for name, run in SCENARIOS.items():
        LINES.clear(), BUFS.clear(), ALIVE.clear()
        run()
        if not DRY:
            torch.cuda.synchronize()
        text = "\n".join(LINES) + "\n"
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            open(os.path.join(args.out, name + ".txt"), "w").write(text)
        print(f"{name:18s} {len(LINES):5d} launches  sha256 {hashlib.sha256(text.encode()).hexdigest()}  ({'dry' if DRY else 'gpu'})")
