"""Step engine: explicit forward / backward of the TVTSv2 model over hand-written HIP kernels.

No autograd graph is built here: every activation that the backward pass needs is kept in a named
workspace buffer and the backward is written out by hand, kernel by kernel (tvts_amd.hip).  The
module classes in tvts_amd/model wrap this engine behind the reference's nn.Module surface.

Numerics: bf16 MFMA operands with fp32 accumulation; the residual stream, LayerNorm statistics,
embeddings, losses, gradients of parameters, master weights and optimizer state are fp32.

Reference being restated (file:line under v2/):
  forward wiring            model/model_dist_TVTSv2_ViT_B_16.py:61-116
  space-time ViT            model/video_encoder_ViT_B_16.py:94-124,176-235
  CLIP text tower           CLIP/clip/model.py:171-203,345-358
  transcript sorting head   model/sort_transformer.py:61-80,124-142
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import os

import torch

from . import hip as K
from .arch import check_recompute, is_mfma_weight, n_keep, param_shapes, patches_per_frame

CH = 1024  # flat-buffer alignment / optimizer chunk (elements)


class ParamStore:
    """All parameters in ONE flat fp32 buffer (+ flat grad, bf16 shadow, transposed bf16 shadow).

    nn.Parameters handed to the outside world are views into ``flat``; ``grad`` views are installed as
    ``.grad`` so an external optimizer (the reference entrypoint builds transformers.AdamW) sees them.
    """

    def __init__(self, arch: dict, device: torch.device):
        if arch.get("fp8_wgrad"):  # e4m3 weight gradients ride on the e4m3 forward and input-gradient operand copies
            arch["fp8"] = arch["fp8_dgrad"] = True
        self.arch = arch
        self.device = device
        self.shapes = param_shapes(arch)
        self.off: Dict[str, int] = {}
        off = 0
        for name, shape in self.shapes.items():
            self.off[name] = off
            off += -(-int(np.prod(shape)) // CH) * CH
        self.total = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=device)
        self.grad = torch.zeros(off, dtype=torch.float32, device=device)
        self.shadow = torch.zeros(off, dtype=torch.bfloat16, device=device)
        # transposed copies of the MFMA weights
        self.toff: Dict[str, int] = {}
        toff, tiles = 0, []
        for name, shape in self.shapes.items():
            if not is_mfma_weight(name, shape, arch):
                continue
            R, C = shape[0], int(np.prod(shape[1:]))
            self.toff[name] = toff
            for tr in range(-(-R // 64)):
                for tc in range(-(-C // 64)):
                    tiles.append((self.off[name], toff, R, C, tr, tc))
            toff += -(-R * C // CH) * CH
        self.shadow_t = torch.zeros(max(toff, 8), dtype=torch.bfloat16, device=device)
        rec = np.zeros(len(tiles), dtype=[("s", "<i8"), ("d", "<i8"), ("R", "<i4"), ("C", "<i4"), ("tr", "<i4"), ("tc", "<i4")])
        for i, t in enumerate(tiles):
            rec[i] = t
        self.n_tiles = len(tiles)
        self.tile_src = [t[0] for t in tiles]  # (ascending: parameter order) -> tiles of a flat range by bisection
        self.tile_table = torch.from_numpy(rec.view(np.uint8).copy()).to(device)
        # patch-embedding GEMM: K = 3*p*p must be a multiple of 64 for the MFMA kernel; H/14 (588) gets a zero-padded copy
        self.conv_name = "video_model.patch_embed.proj.weight" if arch.get("family") == "v1" else "video_model.conv1.weight"
        kc = 3 * arch.get("tubelet", 1) * arch["patch"] ** 2
        self.conv_k = kc
        self.conv_kpad = -(-kc // 64) * 64
        self.conv_pad = (torch.zeros(arch["width"], self.conv_kpad, dtype=torch.bfloat16, device=device)
                         if self.conv_kpad != kc else None)
        self.w8: Dict[str, tuple] = {}
        self.w8t: Dict[str, tuple] = {}
        self._q8_table = None
        self.fp8_names = [n for n in self.shapes if n.startswith("video_model.transformer.resblocks.") and
                          n.endswith(("qkv.weight", "proj.weight", "c_fc.weight", "c_proj.weight"))]
        self.m: Optional[torch.Tensor] = None
        self.v: Optional[torch.Tensor] = None
        self.shadow_version = -1
        self._views: Dict[str, torch.Tensor] = {}
        self._gviews: Dict[str, torch.Tensor] = {}

    def _n(self, name):
        return int(np.prod(self.shapes[name]))

    def p(self, name) -> torch.Tensor:
        v = self._views.get(name)
        if v is None:
            o = self.off[name]
            v = self._views[name] = self.flat[o:o + self._n(name)].view(self.shapes[name])
        return v

    def g(self, name) -> torch.Tensor:
        v = self._gviews.get(name)
        if v is None:
            o = self.off[name]
            v = self._gviews[name] = self.grad[o:o + self._n(name)].view(self.shapes[name])
        return v

    def g2d(self, name) -> torch.Tensor:
        s = self.shapes[name]
        return self.g(name).view(s[0], -1)

    def w(self, name) -> torch.Tensor:
        """bf16 shadow, 2-D [shape[0], rest] as stored."""
        o, s = self.off[name], self.shapes[name]
        return self.shadow[o:o + self._n(name)].view(s[0], -1)

    def wt(self, name) -> torch.Tensor:
        """bf16 shadow transposed, [rest, shape[0]]."""
        o, s = self.toff[name], self.shapes[name]
        return self.shadow_t[o:o + self._n(name)].view(-1, s[0])

    def refresh_transposed(self, s: int, e: int):
        """the transposed shadows of the MFMA weights inside the flat element range [s, e) (tiles are stored in parameter order)"""
        import bisect
        lo, hi = bisect.bisect_left(self.tile_src, s), bisect.bisect_left(self.tile_src, e)
        if hi > lo:
            K.transpose_batched(self.shadow, self.shadow_t, self.tile_table[lo * 32:hi * 32], hi - lo)

    def refresh_shadows(self, cast: bool = True, transposed: bool = True):
        """fp32 master -> bf16 shadow (+ transposed copies).  cast=False when the fused AdamW kernel
        already wrote the plain shadow; transposed=False when refresh_transposed has covered every range."""
        if cast:
            K.cast_f32_bf16(self.flat, self.shadow)
        if self.n_tiles and transposed:
            K.transpose_batched(self.shadow, self.shadow_t, self.tile_table, self.n_tiles)
        if self.conv_pad is not None:
            K.pad_rows_bf16(self.w(self.conv_name), self.conv_pad)
        if self.arch.get("fp8"):  # BASELINE config 4: e4m3 copies (+ per-tensor scales) of the ViT blocks' linear weights
            # ... and (fp8_dgrad) of their transposes, the input-gradient operands: the bf16 transposed shadow under the scale of the
            # master weight (a bf16 rounding past its amax saturates at +-448).  One table, three launches for all of them.
            if self._q8_table is None:
                dg = bool(self.arch.get("fp8_dgrad"))
                nw = len(self.fp8_names)
                scal = torch.zeros(3 * nw, dtype=torch.float32, device=self.device)  # amax | scale | scale_t per weight
                ents = []
                for i, name in enumerate(self.fp8_names):
                    s0 = self.shapes[name]
                    rows, cols = s0[0], int(np.prod(s0[1:]))
                    q = torch.empty(rows, cols, dtype=torch.uint8, device=self.device)
                    am, sc, sct = scal[3 * i:3 * i + 1], scal[3 * i + 1:3 * i + 2], scal[3 * i + 2:3 * i + 3]
                    self.w8[name] = (q, sc, am)
                    qt = None
                    if dg:
                        qt = torch.empty(cols, rows, dtype=torch.uint8, device=self.device)
                        self.w8t[name] = (qt, sct)
                    ents.append((self.p(name).view(rows, cols), q, self.wt(name) if dg else None, qt, am, sc, sct if dg else None))
                self._q8_table = K.quantize_fp8_multi_table(ents, self.device)
            K.quantize_fp8_multi(*self._q8_table)

    def w_conv(self) -> torch.Tensor:
        """bf16 patch-embedding weight [W, K padded to 64]."""
        return self.conv_pad if self.conv_pad is not None else self.w(self.conv_name)


_TEXT_NAMES = dict(ln1="ln_1", qkv_w="attn.in_proj_weight", qkv_b="attn.in_proj_bias", o_w="attn.out_proj.weight",
                   o_b="attn.out_proj.bias", ln2="ln_2", fc_w="mlp.c_fc.weight", fc_b="mlp.c_fc.bias",
                   pj_w="mlp.c_proj.weight", pj_b="mlp.c_proj.bias")
_SORT_NAMES = dict(ln1="norm1", qkv_w="attn.qkv.weight", qkv_b="attn.qkv.bias", o_w="attn.proj.weight",
                   o_b="attn.proj.bias", ln2="norm2", fc_w="mlp.fc1.weight", fc_b="mlp.fc1.bias",
                   pj_w="mlp.fc2.weight", pj_b="mlp.fc2.bias")


class Engine:
    def __init__(self, store: ParamStore):
        self.P = store
        self.arch = store.arch
        a = self.arch
        if a["tail"] not in ("all_tokens", "pooled_and_patches"):
            raise ValueError(f"unknown tail {a['tail']!r}")
        self.dh = a["width"] // a["heads"]            # ViT head dim: 64 (B/32, B/16) or 80 (H/14)
        self.dh_text = a["text_width"] // a["text_heads"]
        self.sort_width = a.get("sort_width", a["embed"])  # v2: the sort head works on the projected tokens (E); v1: on the ViT width
        self.dh_sort = self.sort_width // a["sort_heads"]
        for d, w, h in ((self.dh, a["width"], a["heads"]), (self.dh_text, a["text_width"], a["text_heads"]),
                        (self.dh_sort, self.sort_width, a["sort_heads"])):
            if d not in (64, 80) or d * h != w:
                raise NotImplementedError(f"attention kernels are built for head dim 64 and 80, not {w}/{h}")
        self.pooled_tail = a["tail"] == "pooled_and_patches"
        self.sort_used_rows_only = bool(a.get("sort_used_rows_only", True))  # last sort block on the rows the head reads (sort_forward)
        self.text_used_rows_only = bool(a.get("text_used_rows_only", a.get("sort_used_rows_only", True)))  # last text block: EOT rows
        self.has_sort_head = bool(a.get("sort_head", True))
        # the training step's text tower over PACKED captions (opt-in): M = sum L_i token rows instead of N * max L_i
        tp = a.get("text_packed")
        if tp is None and a.get("family") != "v1" and os.environ.get("TVTS_TEXT_PACKED"):  # (the reference entrypoint builds no arch dict)
            tp = os.environ["TVTS_TEXT_PACKED"] != "0"
        self.text_packed = bool(tp)
        if self.text_packed:
            if a.get("family") == "v1":
                raise ValueError("text_packed: the v1 text tower masks padded keys, it is not causal -- rows behind a caption's end "
                                 "are no dead rows there")
            if self.dh_text != 64:
                raise NotImplementedError("text_packed: the packed attention kernels are built for head dim 64")
        # the v1 counterpart (opt-in, DESIGN.md 8b "v1"): the DistilBERT tower over M = sum(len_i) rows, bidirectional packed attention
        self.text_unpadded = bool(a.get("text_unpadded"))
        if self.text_unpadded and a.get("family") != "v1":
            raise ValueError("text_unpadded is the v1 (DistilBERT) option; the CLIP text tower of v2 packs with text_packed")
        # Precision of the space-time blocks' residual stream (round 3).  Every consumer but the residual adds themselves reads
        # these tensors as bf16 anyway (LayerNorm outputs and GEMM operands are bf16): fp32 buys exact accumulation along the
        # 12 / 32 blocks, at 2.1 GB per block of HBM traffic in the forward + saved activations and 1.4 GB in the backward chain
        # (192 pairs).  Measured on B/16 against the fp32 oracle (experiments/dbg/grad_margins.py, profiles/r03_bf16_streams_ab.txt):
        #   gradient stream bf16 (OPT-IN since round 4, arch["bf16_grad_stream"], bench.py --bf16-grad-stream; round 3 had it on):
        #     +1.4 %; forward untouched; gradient norm -0.25 %, worst tensor cosine 0.9983 -- but the embedding-side gradients
        #     behind ln_pre's cancellation carry 2.4x the error of the fp32 chain (5.8 % rel-L2 instead of 2.4 %), and the golden
        #     gradient slices needed their gate widened from 0.08 to 0.12 to pass: parity is the first gate, 1 % is not worth it;
        #   residual stream bf16 as well (OPT-IN, arch["bf16_residual"], bench.py --bf16-residual): +5 % in total (1354-1372
        #     pairs/s); video embedding rel-L2 0.89 % (gate 2 %; 0.39 % in fp32), row cosine 0.99995 (gate 0.9995), but the
        #     |d loss| <= 1e-2 gate fails on one small 3-pair NT = 1 configuration (0.0155) -- parity is the first gate, so it
        #     is not the default.
        # Round 5, the HYBRID stream (arch["hybrid_stream"], the default for v2): both streams bf16, EXCEPT the CLS token's row of
        # every clip, which is carried in fp32 in compact [B, W] side arrays.  experiments/dbg/bf16_residual_rows.py (the fp32 oracle
        # with bf16 roundings at the engine's stream points) shows where the error of a bf16 stream comes from: rounding the 784
        # patch rows of a clip costs |d loss1| 2e-4 ... 1.7e-3 (2 ... 12 blocks), rounding the ONE CLS row 3.4e-3 ... 5e-3 -- the video
        # embedding is read from that row, and its error reaches every other token through the attention, while the patch rows'
        # independent errors average out in it; for the gradient stream likewise (positional-embedding gradient rel-L2 1e-4 ... 1.3e-3
        # with the CLS row exact against 2 ... 3.7e-2 with every row rounded).  So 784 of 785 rows take the bf16 bytes and the loss /
        # gradient errors stay at the fp32 streams' level: the forward CLS rows through two [B, K] GEMMs per block with fp32 residual
        # (`_cls_lin`), the LayerNorms read / write them beside the stream (tvts_layernorm_{fwd,bwd}_cls).
        hybrid = a.get("hybrid_stream", None)
        if hybrid is None and os.environ.get("TVTS_HYBRID_STREAM"):
            hybrid = os.environ["TVTS_HYBRID_STREAM"] != "0"
        if hybrid is None:  # default: on, unless one of the older stream options is asked for explicitly
            hybrid = a.get("family") != "v1" and "bf16_residual" not in a and "bf16_grad_stream" not in a
        self.cls32 = bool(hybrid) and a.get("family") != "v1"
        self.bf16_residual = (bool(a.get("bf16_residual", False)) or self.cls32) and a.get("family") != "v1"
        self.bf16_grad_stream = bool(a.get("bf16_grad_stream", False)) or self.bf16_residual
        # Weight gradients of the space-time blocks on a SIDE STREAM (round 4).  dW = dY^T X depends on dY only, not on the
        # input-gradient chain that continues from dY, so the weight-gradient kernels can run beside the chain's NT GEMMs,
        # attention and LayerNorm backwards.  At the reference's own per-GPU batches (12 / 24 pairs: 111 ... 444 output tiles
        # for 256 persistent blocks) the chain leaves a third to a half of the CUs idle; the side stream's kernels fill them.
        # MEASURED (profiles/r04_wgrad_side_stream.txt) and NOT the default: the kernels do overlap in the replayed graph, but a
        # weight-gradient block (64 KiB LDS, two per CU) and an NT block (160 KiB, the whole CU) cannot share a CU, so the pairs
        # mostly take turns (NT 63 us + TN 50 us alone -> 112 us side by side), and every fork / join edge between the two
        # streams costs the graph 5-15 us: 12 / 24 / 48 / 192 pairs run 667.9 / 933.4 / 1130 / 1325 pairs/s with it against
        # 692.9 / 958.5 / 1154 / 1351 without.  arch["wgrad_stream"] = True switches it on (bit-identical gradients,
        # tests/test_bench_path_gpu.py::test_wgrad_side_stream_gives_the_same_bits).
        self.wgrad_stream = a.get("wgrad_stream", False)
        # The MLPs' saved tensor is act'(pre-activation), not the pre-activation (round 5, TVTS_GEMM_SIDE_DERIV; arch["gate_deriv"] =
        # False stores the pre-activation as rounds 1-4 did): the forward epilogue evaluates the sigmoid / erf parts for the
        # activation anyway and adds two multiply-adds for the derivative; the input gradient's gate epilogue then multiplies by the
        # stored bf16 value instead of evaluating the transcendentals again.  Nothing else reads the tensor.
        self.gate_deriv = bool(a.get("gate_deriv", os.environ.get("TVTS_GATE_DERIV", "1") != "0"))
        # The text tower on its own stream beside the ViT (round 5).  The two towers share nothing until the loss (the sort head reads
        # DETACHED caption embeddings, model_dist_TVTSv2_ViT_B_16.py:61-95): the text tower's forward (12 blocks of 5-25 us kernels
        # on <= 48 tiles) and its three trainable blocks' backward are latency-bound chains -- in the replayed 12-pair step every one
        # of their ~150 kernels waits 10-20 us for its predecessor's completion signal (profiles/r04_timeline_b12.txt) -- that fit
        # beside the ViT's kernels: ONE fork and ONE join per direction, scratch buffers of their own (hip.lane).
        # arch["text_side"]: True / False, None = on
        ts = a.get("text_side", None)
        if ts is None and os.environ.get("TVTS_TEXT_SIDE"):  # (A/B runs of whole test files / tools without touching their arch dicts)
            ts = os.environ["TVTS_TEXT_SIDE"] != "0"
        self.text_side = (True if ts is None else bool(ts)) and a.get("family") != "v1"
        self._txt_stream = None
        # The six weight gradients of a ViT block in ONE grouped launch + one reduce launch (round 4, tvts_gemm_tn_bf16_grouped):
        # arch["tn_grouped"] True / False, None = automatic (up to TN_GROUPED_MAX_ROWS token rows per GPU, where a single weight
        # gradient fills a fraction of a round of the chip and its launch ramp is a third of its time)
        self.tn_grouped = a.get("tn_grouped", None)
        self._tn_groups: Dict[object, object] = {}
        self._tn_group_ws = None
        # e4m3 weight gradients (BASELINE config 5): per-tensor delayed scaling of every e4m3 operand copy, see _q8 below
        self.fp8_wgrad = bool(a.get("fp8_wgrad", False))
        self.fp8_q8_only = self.fp8_wgrad and bool(a.get("fp8_q8_only", True))
        self._x8_only = set()
        self._f8_ids: Dict[str, int] = {}
        self._f8_scale = self._f8_amax = None
        self._f8_tensor_mode = False
        self._x8: Dict[str, tuple] = {}
        self._x8_ready: Dict[str, tuple] = {}   # operand copies written by a producer's epilogue, waiting for their consumer
        self._dy8_ready: Dict[str, tuple] = {}
        self._wg_stream = None
        self._wg_ws = None
        # Activation recomputation of the VIDEO tower (DESIGN.md "Activation recomputation"): arch["recompute"] "none" | "mlp" | "block".
        #   "block"  the forward keeps the residual stream behind every block (x<l>, xc<l>); every other tensor a block saves goes
        #            into ONE slot shared by all blocks (two, by layer parity, beside the weight-gradient side stream), and the
        #            backward re-runs block l's training forward from x<l> into the slot just before block l's backward;
        #   "mlp"    everything is kept but the two [M, 4W] tensors of the MLP (act'(x) and the activation), which share one pair of
        #            buffers; the backward re-runs fc1 from the kept ln2.
        # The second evaluation launches the kernels of the first on the same operand bytes, so it leaves the same bits.
        self.recompute = check_recompute(a)
        self.recompute_count = 0                  # block (or fc1) re-evaluations of the last backward
        self._rc_fwd: Dict[str, str] = {}         # tower tag -> the mode its last forward ran in (its backward follows that)
        self._rc_held: Dict[str, int] = {}        # slot tag -> the block whose tensors it holds
        self.dev = store.device
        if self.dev.type == "cuda":
            K.warm_scratch(self.dev)
        self.buf: Dict[str, torch.Tensor] = {}
        self._back: Dict[str, torch.Tensor] = {}  # the allocations behind buf (grow-only, see _b)
        self._seen: Dict[str, int] = {}           # name -> the forward() count at which its shape last changed
        self._tick = 0
        self._inf: Dict[str, torch.Tensor] = {}   # the forward-only encoders' workspaces, by role (see _ib)
        self.requires_grad = {name: True for name in store.shapes}
        self.ctx: dict = {}
        self.grad_ready = None  # optional callback(start, end): flat grad range is final (GradSync.reduce_range); may return a wait()
        self.param_ready = None  # optional callback(start, end, wait): the range may be stepped (FusedHFAdamW.step_range)
        self.embeds_ready = None  # optional callback(text_emb, video_emb): both embeddings exist, the sort head has not run yet
        self._ranges: dict = {}

    def _ready(self, *prefixes: str):
        """The gradients of every parameter whose name starts with one of `prefixes` are final: hand their flat ranges
        (contiguous in state-dict order, whichever registration order the architecture uses) to the gradient sync --
        maximal runs of TRAINABLE tensors only: the frozen text layers below the tune range (train_dist..:89-96, ~28 M
        parameters of all-zero gradient for ViT-B/16) never travel."""
        if self.grad_ready is None and self.param_ready is None:
            return
        for lo, hi in self.trainable_runs(prefixes):
            wait = self.grad_ready(lo, hi) if self.grad_ready is not None else None
            if self.param_ready is not None:  # the optimizer's update of the range, beside the remaining backward
                self.param_ready(lo, hi, wait)

    def trainable_runs(self, prefixes):
        P = self.P
        ent = self._ranges.get(prefixes)
        if ent is None:
            names = [n for n in P.shapes if n.startswith(prefixes)]
            lo = min(P.off[n] for n in names)
            hi = max(P.off[n] + -(-P._n(n) // CH) * CH for n in names)
            inside = [n for n in P.shapes if lo <= P.off[n] < hi]
            assert inside == names, f"parameters {prefixes} are not contiguous in the flat buffer"
            ent = self._ranges[prefixes] = dict(names=names, sig=None, runs=None)
        sig = tuple(self.requires_grad[n] for n in ent["names"])
        if sig != ent["sig"]:
            runs = []
            for n, tr in zip(ent["names"], sig):
                if not tr:
                    continue
                s, e = P.off[n], P.off[n] + -(-P._n(n) // CH) * CH
                if runs and runs[-1][1] == s:
                    runs[-1][1] = e
                else:
                    runs.append([s, e])
            ent["sig"], ent["runs"] = sig, [tuple(r) for r in runs]
        return ent["runs"]

    # ------------------------------------------------------------------ workspace
    def _b(self, name, shape, dtype=torch.bfloat16, zero=False):
        """A named workspace tensor.  Its storage only ever GROWS: a smaller shape is a view of the first elements of the same
        allocation, so a loop that alternates batches of two sizes (the reference's YT / WebVid loaders, trainer.py:463) keeps
        every buffer's address -- no allocator traffic after the first pass over both, and plans keyed by buffer addresses (the
        grouped weight gradients) stay valid."""
        t = self.buf.get(name)
        shape = tuple(int(s) for s in shape)
        if t is not None and tuple(t.shape) == shape and t.dtype == dtype:
            self._seen[name] = self._tick  # (live in this step: a later request for ANOTHER shape under this name must not alias it)
            if zero:
                K.zero_(t)
            return t
        n = 1
        for s in shape:
            n *= s
        seen, self._seen[name] = self._seen.get(name), self._tick
        if seen == self._tick:
            # the name changes shape WITHIN one forward / backward pair: both tensors may be live, so they must not share memory
            t = self.buf[name] = torch.empty(shape, dtype=dtype, device=self.dev)
        else:
            back = self._back.get(name)
            if back is None or back.dtype != dtype or back.numel() < n:
                back = self._back[name] = torch.empty(max(n, 1), dtype=dtype, device=self.dev)
            t = self.buf[name] = back[:n].view(shape)
        if zero:
            K.zero_(t)
        return t

    def _f(self, name, shape, zero=False):
        return self._b(name, shape, torch.float32, zero)

    def _ib(self, role, shape, dtype=torch.bfloat16):
        """encoder workspace `role`: a view of a grow-only byte buffer (roles are reused with other shapes / dtypes)"""
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        back = self._inf.get(role)
        if back is None or back.numel() < n:
            self._inf.pop(role, None)  # (the smaller buffer goes first)
            back = self._inf[role] = torch.empty(max(n, 16), dtype=torch.uint8, device=self.dev)
        return back[:n].view(dtype).view(shape)

    def _w(self, tag, name, role, shape, dtype=torch.bfloat16):
        """A buffer of the forward wiring, which both passes run ("The two passes of the forward" below): the training step's named
        tensor tag + name, which its backward reads -- or, forward-only (tag None), the encoder workspace `role`."""
        if tag is None:
            return self._ib(role, shape, dtype)
        return self._b(tag + name, shape, dtype)

    def _ones(self, n):
        """a vector of n ones (the bias gradients as 1^T dy products): a constant made once per length, never written again"""
        t = self.buf.get(("ones", n))
        if t is None:
            t = self.buf[("ones", n)] = torch.ones(n, dtype=torch.float32, device=self.dev)
        return t

    def set_recompute(self, mode):
        """switch the recomputation mode between steps (validated as at construction); buffers only grow, nothing is freed"""
        self.recompute = self.arch["recompute"] = check_recompute(self.arch, mode)

    def workspace_bytes(self) -> int:
        """the bytes behind every named workspace: the grow-only allocations of _b, the fresh tensors in buf, and the encoders'"""
        seen = {}
        for t in list(self._back.values()) + list(self.buf.values()) + list(self._inf.values()):
            st = t.untyped_storage()
            seen[st.data_ptr()] = st.nbytes()
        return sum(seen.values())

    @staticmethod
    def _rc_tags(tag, l, mode, parity=False):
        """-> (tag of the tensors block l of tower `tag` saves, tag of its MLP pair h / a) under recomputation mode `mode`: the
        block's own tag + "<l>", or the shared slot tag + ".rc" (parity: one slot per layer parity, for the side stream's weight
        gradients of block l + 1, which still read their operands while block l is evaluated again)"""
        own = f"{tag}{l}"
        if mode == "none":
            return own, own
        slot = f"{tag}.rc{l % 2}" if parity else f"{tag}.rc"
        return (slot, slot) if mode == "block" else (own, slot)

    def _row_starts(self, role, count, stride):
        """encoder workspace `role`: int32 [count], the first row of every sequence of `stride` rows (its CLS / [CLS] token)"""
        t = self._ib(role, (count,), torch.int32)
        t.copy_(torch.arange(count, device=self.dev, dtype=torch.int32) * stride)
        return t

    # small dense heads (an nn.Linear with bias on a few rows, fp32: txt_proj / vid_proj of the v1 model, the sort head's classifier)
    def _head_lin(self, x, wname, bname, out, R):
        """out [R, O] = x [R, I] W^T + b, W = the parameter wname [O, I]"""
        O, I = self.P.shapes[wname]
        K.gemm_small(x, self.P.p(wname), out, M=R, N=O, K=I, sa=(I, 1), sb=(1, I), bias=self.P.p(bname))

    def _head_lin_bwd(self, dy, x, wname, bname, dx, R):
        """its backward, three launches in this order: dW += dy^T x, db += 1^T dy, dx = dy W"""
        O, I = self.P.shapes[wname]
        K.gemm_small(dy, x, self.P.g(wname), M=O, N=I, K=R, sa=(1, O), sb=(I, 1), accumulate=True)
        K.gemm_small(self._ones(R), dy, self.P.g(bname).view(1, O), M=1, N=O, K=R, sa=(0, 1), sb=(O, 1), accumulate=True)
        K.gemm_small(dy, self.P.p(wname), dx, M=R, N=I, K=O, sa=(O, 1), sb=(I, 1))

    # ------------------------------------------------------------------ e4m3 copies (BASELINE config 4 / 5)
    # Two regimes of the e4m3 operand copies:
    #   per TOKEN  (arch["fp8"], arch["fp8_dgrad"]): one scale per row, written by the producing LayerNorm or by a one-pass row
    #              quantiser, applied per row in the GEMM epilogue; the weight gradients stay bf16;
    #   per TENSOR (arch["fp8_wgrad"], round 4): the weight gradient contracts over the tokens, so its operands can only carry one
    #              scale per tensor -- and a copy under one scale serves the forward / input-gradient GEMMs as well.  Delayed
    #              scaling: every producer quantises under the tensor's scale of LAST step (amax / 448) and records this step's
    #              amax; end_step() turns the maxima into the next scales.  The first step has no scales yet: it runs per token
    #              with bf16 weight gradients while the maxima are recorded ("calibration"), and end_step() switches over.
    def _f8_slot(self, name):
        """(scale, amax) device scalars of tensor `name` (views of two flat arrays, so that one kernel updates all of them)"""
        i = self._f8_ids.get(name)
        if i is None:
            if self._f8_scale is None:
                cap = 16 * (self.arch["layers"] + 2)
                self._f8_scale = torch.zeros(cap, dtype=torch.float32, device=self.dev)
                self._f8_amax = torch.zeros(cap, dtype=torch.float32, device=self.dev)
            i = self._f8_ids[name] = len(self._f8_ids)
            assert i < self._f8_scale.numel(), "more e4m3 tensors than the scale table holds"
        return self._f8_scale[i:i + 1], self._f8_amax[i:i + 1]

    def end_step(self, guard_norm=None):
        """Called once per optimisation step (StepRunner.run) after the backward: this step's amax values become the per-tensor
        scales of the next step, and from the second step on the e4m3 copies are per-tensor and the weight gradients e4m3.
        guard_norm (StepRunner(skip_nonfinite=True): the device norm of the step's gradient): the guarded update -- a maximum that
        is not finite never becomes a scale, a step whose norm is not finite keeps every scale, and a slot without a usable scale
        (the calibration step was the bad one) gets 1.0 (tvts_fp8_update_scales_guarded)."""
        if self.fp8_wgrad and self._f8_scale is not None:
            if guard_norm is not None:
                K.fp8_update_scales_guarded(self._f8_amax, self._f8_scale, guard_norm)
            else:
                K.fp8_update_scales(self._f8_amax, self._f8_scale)
            self._f8_tensor_mode = True

    def _q8(self, M, W, name, persistent=False):
        """Buffers for the e4m3 copy of tensor `name` [M, W]: (bytes, scale operand for the GEMMs, kwargs for the producing kernel).
        persistent: the bytes outlive the next producer of the same width (an activation the weight gradient reads in the backward).
        name None: forward-only (the encoders).  Always the per-token regime, which has no state: the bytes and the row scales are
        encoder workspaces keyed by role and width, reused by every layer; no scale slot is looked up, made or written."""
        if name is None:
            q = self._ib("q8.%d" % W, (M, W), torch.uint8)
            rs = self._ib("q8.row_scale", (max(M, 2),), torch.float32)  # (never a 1-element tensor, as below)
            return q, rs, dict(row_scale=rs)
        q = self._b(("fp8.x." + name) if (persistent and self.fp8_wgrad) else "fp8.q%d" % W, (M, W), torch.uint8)
        if not self.fp8_wgrad:
            rs = self._f("fp8.row_scale", (max(M, 2),))  # never a 1-element tensor: that means "one scale for the tensor"
            return q, rs, dict(row_scale=rs)
        sc, am = self._f8_slot(name)
        if self._f8_tensor_mode:
            return q, sc, dict(tscale=sc, amax=am)
        rs = self._f("fp8.row_scale", (max(M, 2),))
        return q, rs, dict(row_scale=rs, amax=am)

    # ------------------------------------------------------------------ linear helpers
    def _wgrad_side(self, M) -> bool:
        return bool(self.wgrad_stream)

    def _side(self):
        """(side stream, its own split-partial workspace): the weight-gradient kernels of one stream share one workspace, the two
        streams never do"""
        if self._wg_stream is None:
            self._wg_stream = torch.cuda.Stream(device=self.dev)
            self._wg_ws = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device=self.dev)
        return self._wg_stream, self._wg_ws

    def _q8_out(self, M, W, name, persistent=False):
        """kwargs that make an e4m3 GEMM's epilogue write the per-tensor e4m3 copy of its bf16 result (tensor mode only), and the
        (bytes, scale) pair its consumers take"""
        # OPT-IN (arch["fp8_epilogue_copies"]): measured on H/14, 16 frames, 48 pairs (profiles/r04_kernel_summary_h14_b48_fp8_wgrad.txt):
        # the two quantiser passes it removes are worth 8.6 ms per step, the two epilogues that take their work over get 105 / 120 us
        # slower per launch (7.2 ms: they are the epilogue-bound GELU / gate forms, and the extra stores spill 30-40 bytes more) --
        # 295.3 against 295.8 ms per step, not worth a second path by default
        # Round 5, arch["fp8_q8_only"] (default with fp8_wgrad): the epilogue writes the e4m3 copy INSTEAD of the bf16 result -- in the
        # per-tensor regime every consumer of the MLP's GELU output (fc2 forward, fc2 weight gradient) and of the gated hidden gradient
        # (fc1 input and weight gradient, bias gradient on the matrix pipe) multiplies the e4m3 bytes: one byte per element leaves
        # the epilogue where round 4 wrote two and a quantiser pass read them again
        if not (self.fp8_wgrad and self._f8_tensor_mode and (self.arch.get("fp8_epilogue_copies") or self.fp8_q8_only)):
            return {}, None
        q, sc, kw = self._q8(M, W, name, persistent=persistent)
        return dict(q8out=q, q8_scale=sc, q8_amax=kw["amax"]), (q, sc)

    def _lin(self, a, wname, bname, out, M, a8=None, q8_for=None, fwd_only=False, **epi):
        """q8_for: the weight whose GEMMs read `out` as their activation; in the per-tensor e4m3 regime the epilogue of this GEMM
        then writes that operand copy itself (the MLP's GELU output), instead of a quantiser pass over `out`.
        fwd_only (the encoders' blocks, tag None): an e4m3 layer runs in the per-token regime whatever _f8_tensor_mode says, on
        encoder workspaces, and leaves the backward's bookkeeping (_x8, _x8_ready, _x8_only) and the scale table alone."""
        if epi.get("act") is not None and self.gate_deriv:
            # the side output `preact` holds act'(x), which the gate of the backward multiplies by as is (every call of the training
            # step that passes act passes preact); forward-only there is no preact: the same epilogue instantiation, side output skipped
            epi["side_deriv"] = True
        if wname in self.P.w8 and fwd_only:
            w8, ws, _ = self.P.w8[wname]
            if a8 is None:  # activations that do not come out of a LayerNorm: one pass
                q, sa, kw = self._q8(M, a.shape[1], None)
                K.quantize_fp8_rows(a[:M], q=q, **kw)
                a8 = (q, sa)
            K.gemm_nt_fp8(a8[0], a8[1], w8, ws, out[:M], bias=self.P.p(bname) if bname else None, **epi)
            return
        if wname in self.P.w8:  # fp8 weight/activation path (BASELINE config 4): forward GEMMs of the ViT blocks
            w8, ws, _ = self.P.w8[wname]
            if a8 is None:
                a8 = self._x8_ready.pop(wname, None)
            if q8_for is not None and q8_for in self.P.w8:
                kw8, nxt = self._q8_out(M, out.shape[1], "x." + q8_for, persistent=True)
                epi = dict(epi, **kw8)
                if nxt is not None:
                    self._x8_ready[q8_for] = nxt
                    if self.fp8_q8_only and self.requires_grad[q8_for]:
                        epi["store_out"] = False       # `out` (bf16) is not written: its consumers read nxt
                        self._x8_only.add(q8_for)
            if a8 is None:  # activations that do not come out of a LayerNorm: one pass
                q, sa, kw = self._q8(M, a.shape[1], "x." + wname, persistent=True)
                K.quantize_fp8_rows(a[:M], q=q, **kw)
                a8 = (q, sa)
            self._x8[wname] = a8
            K.gemm_nt_fp8(a8[0], a8[1], w8, ws, out[:M], bias=self.P.p(bname) if bname else None, **epi)
            return
        K.gemm_nt(a, self.P.w(wname), out, M=M, bias=self.P.p(bname) if bname else None, **epi)

    def _cls_lin(self, a, S, wname, bname, res_c, out_c, fwd_only=False):
        """The CLS rows of the hybrid stream through a residual-adding linear layer: out_c [B, N] = res_c + a[b * S, :] @ W^T + bias,
        fp32 result and fp32 residual (the stream's own rows take the bf16 residual epilogue).  a: the [B * S, K] bf16 operand of the
        block's GEMM; its CLS rows are addressed as a [B, K] matrix with the row stride S * K -- the same operand bytes and the same
        bf16 weight shadow, always on the bf16 MFMA path (also when the block's GEMMs multiply e4m3 copies).  fwd_only: an encoder
        call, whose operands always exist in bf16 (per-token regime) and which reads nothing the training step recorded."""
        Bc = out_c.shape[0]
        if wname in self._x8_only and not fwd_only:  # the operand only exists as e4m3 bytes (arch["fp8_q8_only"]): the same rows of that copy
            q, sa = self._x8[wname]
            w8, ws, _ = self.P.w8[wname]
            K.gemm_nt_fp8(q[:Bc * S].view(Bc, -1)[:, :q.shape[1]], sa, w8, ws, out_c, bias=self.P.p(bname) if bname else None, residual=res_c)
            return
        a_c = a[:Bc * S].view(Bc, -1)[:, :a.shape[1]]
        K.rows_linear(a_c, self.P.w(wname), out_c, bias=self.P.p(bname) if bname else None, residual=res_c)

    # measured (profiles/r04_tn_grouped.txt): B/16 +1.5 % at 12 pairs (M = 9 420), -0.4 % at 24, -2 % at 48; B/32 +1.2 % at its 24 pairs
    # (M = 9 432); H/14 at its 2 pairs (M = 2 434, 1 600 tiles of 128 x 128 per block of the model) -9 %: the window is where it pays
    TN_GROUPED_MIN_ROWS, TN_GROUPED_MAX_ROWS = 6000, 12000

    def _tn_grouped_on(self, M) -> bool:
        on = self.tn_grouped
        if on is None:
            on = self.TN_GROUPED_MIN_ROWS <= M <= self.TN_GROUPED_MAX_ROWS
        return bool(on) and not self.fp8_wgrad and not self.wgrad_stream

    def _tn_group_run(self, key, problems):
        """launch the deferred weight gradients of one block together.  Plans are cached per (block, problem signature): the
        reference's loop alternates two loaders with different clip lengths (trainer.py:463), so a block sees two signatures in
        turn -- replacing the plan would rebuild and re-upload it twelve times per step; a bounded number is kept per block."""
        if not problems:
            return
        sig = tuple((pr["p"].data_ptr(), pr["q"].data_ptr(), pr["out"].data_ptr(), pr["M"],
                     pr["colsum"].data_ptr() if pr["colsum"] is not None else 0) for pr in problems)
        plans = self._tn_groups.setdefault(key, {})
        grp = plans.get(sig)
        if grp is None:
            if self._tn_group_ws is None:
                self._tn_group_ws = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device=self.dev)
            if len(plans) >= self.TN_GROUP_PLANS_PER_BLOCK:
                # the oldest plan no hipGraph refers to (a last partial batch, a loader that is gone); a captured plan's device table
                # and staging memory are addresses inside the graph, so it stays
                old = next((k for k, g in plans.items() if not g.captured), None)
                if old is not None:
                    plans.pop(old)
            grp = plans[sig] = K.TnGroup(problems, self._tn_group_ws, splits=int(self.arch.get("tn_group_splits", 0)))
        grp.run()

    TN_GROUP_PLANS_PER_BLOCK = 4

    def _lin_bwd(self, dy, a_in, wname, bname, d_in, M, dy8=None, side=False, q8_for=None, defer=None, **epi):
        """dW += dy^T a_in, db += colsum(dy) (if trainable); d_in = dy W (optional, with epilogue).  dy8: the e4m3 copy of dy
        when its producer already wrote one (_ln_bwd with fp8_for).  side: the weight gradient is launched on the side stream
        behind everything the current stream has queued so far (dy is complete there); the caller keeps dy and a_in untouched
        until it has joined the side stream."""
        want_b = bool(bname) and self.requires_grad[bname]
        if epi.get("gate_h") is not None and epi.get("gate_act") not in (None, "add") and self.gate_deriv:
            epi["side_deriv"] = True  # gate_h is the derivative the forward's epilogue stored (see _lin)
        f8w = self.fp8_wgrad and self._f8_tensor_mode and wname in self.P.w8t and wname in self._x8
        if dy8 is None:
            dy8 = self._dy8_ready.pop(wname, None)
        if (f8w or (d_in is not None and wname in self.P.w8t)) and dy8 is None:
            q, sa, kw = self._q8(M, dy.shape[1], "dy." + wname)
            K.quantize_fp8_rows(dy[:M], q=q, **kw)
            dy8 = (q, sa)
        if self.requires_grad[wname]:  # bias gradient (column sums of dy) rides along in the same kernel
            if defer is not None and not f8w:  # launched with the block's other weight gradients (the caller keeps dy untouched till then)
                defer.append(dict(p=dy, q=a_in, out=self.P.g2d(wname), M=M, accumulate=True, colsum=self.P.g(bname) if want_b else None))
            elif f8w:  # e4m3 weight gradient: both operands under one scale per tensor, the bias gradient from the same bytes
                x8 = self._x8[wname]
                K.gemm_tn_fp8(dy8[0], dy8[1], x8[0], x8[1], self.P.g2d(wname), M=M, accumulate=True,
                              colsum=self.P.g(bname) if want_b else None)
            elif side:
                ws, scratch = self._side()
                ws.wait_stream(torch.cuda.current_stream(self.dev))
                with torch.cuda.stream(ws):
                    K.gemm_tn(dy, a_in, self.P.g2d(wname), M=M, accumulate=True, colsum=self.P.g(bname) if want_b else None,
                              workspace=scratch)
            else:
                K.gemm_tn(dy, a_in, self.P.g2d(wname), M=M, accumulate=True, colsum=self.P.g(bname) if want_b else None)
        elif want_b:
            K.colsum(dy, self.P.g(bname), M=M)
        if d_in is not None:
            if wname in self.P.w8t:  # e4m3 input gradient (arch["fp8_dgrad"]): the transposed weight's e4m3 copy
                w8t, wst = self.P.w8t[wname]
                if q8_for is not None and q8_for in self.P.w8t and epi.get("gate_h") is not None:
                    # the gated input gradient is the output gradient of layer q8_for: its per-tensor e4m3 copy leaves this epilogue
                    kw8, nxt = self._q8_out(M, d_in.shape[1], "dy." + q8_for)
                    epi = dict(epi, **kw8)
                    if nxt is not None:
                        self._dy8_ready[q8_for] = nxt
                        if self.fp8_q8_only and self.requires_grad[q8_for] and q8_for in self._x8:
                            epi["store_out"] = False   # the gated gradient exists as e4m3 bytes only
                K.gemm_nt_fp8(dy8[0], dy8[1], w8t, wst, d_in[:M], **epi)
                return
            K.gemm_nt(dy, self.P.wt(wname), d_in, M=M, **epi)

    def _ln(self, x, name, eps, y, tag, rows=None, M=None, fp8_for=None, cls_x=None):
        """fp8_for: name of the weight the output feeds; when that GEMM runs in fp8 the LayerNorm also emits the e4m3 copy
        (returned, to be handed to _lin as a8).  cls_x: the fp32 CLS rows of the hybrid stream x (read instead of x's own CLS
        rows, which receive their bf16 rounding).  tag: the names of mean / rstd for the backward, None = forward-only, not kept."""
        M = (rows.numel() if rows is not None else x.shape[0]) if M is None else M
        if cls_x is not None:
            kw_cls = dict(cls_x=cls_x, cls_period=M // cls_x.shape[0])
        else:
            kw_cls = {}
        mean = rstd = None
        if tag is not None:
            mean, rstd = self._f(tag + ".mean", (M,)), self._f(tag + ".rstd", (M,))
        a8, kw = None, {}
        if fp8_for is not None and fp8_for in self.P.w8 and tag is None:
            # forward-only: per-token copy in an encoder workspace; its GEMM is the only reader of this LayerNorm's output, so where
            # the e4m3-only form of the kernel exists (bf16 rows, W % 8 == 0, W <= 1536) the bf16 tensor is not written at all
            q, sa, kw = self._q8(M, y.shape[1], None)
            a8, kw = (q, sa), dict(kw, q8=q)
            if rows is None and x.dtype == torch.bfloat16 and y.shape[1] % 8 == 0 and y.shape[1] <= 1536 and x.stride(0) % 8 == 0:
                y = None
        elif fp8_for is not None and fp8_for in self.P.w8:
            q, sa, kw = self._q8(M, y.shape[1], "x." + fp8_for, persistent=True)
            a8, kw = (q, sa), dict(kw, q8=q)
            # arch["fp8_q8_only"]: under per-tensor scales the forward GEMM and the weight gradient both multiply the e4m3 bytes,
            # the bf16 output would be written and never read (8-column form of the kernel: bf16 rows, W % 8 == 0)
            if (self.fp8_q8_only and self.fp8_wgrad and self._f8_tensor_mode and fp8_for in self.P.w8t and rows is None
                    and x.dtype == torch.bfloat16 and y.shape[1] % 8 == 0 and y.shape[1] <= 1536 and q.stride(0) % 8 == 0):
                y = None
        K.layernorm_fwd(x, self.P.p(name + ".weight"), self.P.p(name + ".bias"), eps, y, mean, rstd, rows=rows, M=M, **kw, **kw_cls)
        return a8

    def _ln_bwd(self, dy, x, name, tag, dx, dx_bf16=None, res1=None, res2=None, rows=None, M=None, fp8_for=None,
                cls_x=None, cls_res1=None, cls_dx=None):
        """fp8_for: name of the weight whose input-gradient GEMM consumes dx_bf16; when that GEMM runs on e4m3 operands the
        LayerNorm backward also emits the e4m3 copy (returned, to be handed to _lin_bwd as dy8).  cls_*: the fp32 CLS rows of the
        hybrid stream (input, incoming stream gradient, outgoing stream gradient)."""
        tr = self.requires_grad[name + ".weight"]
        d8, kw = None, {}
        if cls_x is not None or cls_res1 is not None or cls_dx is not None:
            nc = (cls_x if cls_x is not None else cls_dx if cls_dx is not None else cls_res1).shape[0]
            kw = dict(cls_period=(x.shape[0] if M is None else M) // nc, cls_x=cls_x, cls_res1=cls_res1, cls_dx=cls_dx)
        if (fp8_for is not None and fp8_for in self.P.w8t and rows is None and dx_bf16 is not None and dy.dtype == torch.bfloat16
                and not (res2 is not None and res1 is None)):
            q, sa, kw8 = self._q8(dx_bf16.shape[0] if M is None else M, dx_bf16.shape[1], "dy." + fp8_for)
            d8, kw = (q, sa), dict(kw, q8=q, **kw8)
        K.layernorm_bwd(dy, x, self.buf[tag + ".mean"], self.buf[tag + ".rstd"], self.P.p(name + ".weight"), dx,
                        dx_bf16=dx_bf16, res1=res1, res2=res2, dgamma=self.P.g(name + ".weight") if tr else None,
                        dbeta=self.P.g(name + ".bias") if tr else None, rows=rows, M=M, **kw)
        return d8

    # ------------------------------------------------------------------ generic pre-LN block and tower (text, sort head, v1 ViT)
    # `rows` (int32 token rows): a block whose output the model reads at those R rows only, and into whose other output rows no
    # gradient enters.  LayerNorm 1 and the qkv projection stay dense (keys / values of every token); the attention output
    # (attn_fwd: a query-restricted kernel writing the used rows of `att`), the output projection, the residual, LayerNorm 2 and the
    # MLP are computed for the R used rows; backward: dQ for those rows, dK / dV -- and through them the gradient of every input
    # row -- dense.
    def _block_fwd(self, pre, nm, x_in, x_out, tag, heads, act, eps, attn_fwd, rows=None, drop_path=None, mtag=None, redo=False):
        """attn_fwd(qkv, att, lse): the attention call.  tag None: forward-only (lse None, no act'(x) side output; x_out may be x_in).
        -> x_out, or with `rows` the block output at those rows, packed [R, Wd] fp32 (x_out is not used).
        drop_path (dense training blocks only): (scale_attn [B], scale_mlp [B], rows per sample) -- stochastic depth: each branch's
        projection, bias included, goes to an fp32 scratch and tvts_drop_path_rows forms residual + scale[sample] * branch.
        mtag: the tag of the MLP pair h / a where it is not the block's own (_rc_tags); redo: the backward's second evaluation --
        stops behind fc1, the block's output is the kept stream."""
        assert drop_path is None or (rows is None and tag is not None)
        mtag = mtag or tag
        assert (mtag == tag and not redo) or (rows is None and tag is not None)
        w, f32 = self._w, torch.float32
        M, Wd = x_in.shape
        R = M if rows is None else rows.numel()
        ln1 = w(tag, ".ln1", "ln", (M, Wd))
        self._ln(x_in, pre + nm["ln1"], eps, ln1, tag and tag + ".ln1")
        qkv = w(tag, ".qkv", "qkv", (M, 3 * Wd))
        self._lin(ln1, pre + nm["qkv_w"], pre + nm["qkv_b"], qkv, M)
        att = w(tag, ".att", "att", (M, Wd))
        attn_fwd(qkv, att, self._f(tag + ".lse", (M, heads)) if tag else None)
        res = x_in
        if rows is not None:
            att_r, res = w(tag, ".att_r", "att_r", (R, Wd)), w(tag, ".x_r", "x_r", (R, Wd), f32)
            K.rows_move("gather", rows, full_bf16=att, packed_bf16=att_r)   # (row gathers of R x Wd elements)
            K.rows_move("gather", rows, full_f32=x_in, packed_f32=res)
            att, x_out = att_r, w(tag, ".xo_r", "xoc", (R, Wd), f32)
        mid = w(tag, ".mid", "s", (R, Wd), f32)
        if drop_path is None:
            self._lin(att, pre + nm["o_w"], pre + nm["o_b"], mid, R, residual=res)
        else:
            y = self._f("dp.y", (R, Wd))
            self._lin(att, pre + nm["o_w"], pre + nm["o_b"], y, R)
            K.drop_path_rows(y, drop_path[0], drop_path[2], residual=res, out=mid)
        ln2 = w(tag, ".ln2", "ln" if rows is None else "lnc", (R, Wd))
        self._ln(mid, pre + nm["ln2"], eps, ln2, tag and tag + ".ln2")
        h = self._b(mtag + ".h", (R, 4 * Wd)) if tag else None
        a = w(mtag, ".a", "h", (R, 4 * Wd))
        self._lin(ln2, pre + nm["fc_w"], pre + nm["fc_b"], a, R, act=act, preact=h)
        if redo:
            return None
        if drop_path is None:
            self._lin(a, pre + nm["pj_w"], pre + nm["pj_b"], x_out, R, residual=mid)
        else:
            self._lin(a, pre + nm["pj_w"], pre + nm["pj_b"], y, R)
            K.drop_path_rows(y, drop_path[1], drop_path[2], residual=mid, out=x_out)
        return x_out

    def _block_bwd(self, pre, nm, x_in, dx, dxb, dx_in, dxb_in, tag, scr, heads, act, attn_bwd, rows=None, drop_path=None, mtag=None):
        """dx / dxb: fp32 / bf16 gradient of the block output (with `rows`: at those R rows, packed); attn_bwd(qkv, datt, att, lse,
        delta, dqkv): the attention call.  Writes the gradient of every input row to dx_in / dxb_in.
        drop_path: as _block_fwd -- the gradient entering a branch is scale[sample] * (gradient of the sum), formed from the fp32
        gradient as the bf16 operand of _lin_bwd; the residual path keeps the unscaled gradient."""
        assert drop_path is None or rows is None
        B_, mtag = self.buf, mtag or tag
        M, Wd = x_in.shape
        R, r = (M, "") if rows is None else (rows.numel(), "_r")
        dh, dln_r = self._b(scr + ".dh" + r, (R, 4 * Wd)), self._b(scr + ".dln" + r, (R, Wd))
        if drop_path is not None:
            dxb = self._b(scr + ".dpb", (R, Wd))
            K.drop_path_rows(dx, drop_path[1], drop_path[2], out_bf16=dxb)
        self._lin_bwd(dxb, B_[mtag + ".a"], pre + nm["pj_w"], pre + nm["pj_b"], dh, R, gate_h=B_[mtag + ".h"], gate_act=act)
        self._lin_bwd(dh, B_[tag + ".ln2"], pre + nm["fc_w"], pre + nm["fc_b"], dln_r, R)
        dmid, dmidb = self._f(scr + ".dmid" + r, (R, Wd)), self._b(scr + ".dmidb" + r, (R, Wd))
        self._ln_bwd(dln_r, B_[tag + ".mid"], pre + nm["ln2"], tag + ".ln2", dmid, dx_bf16=dmidb, res1=dx)
        datt = self._b(scr + ".datt" + r, (R, Wd))
        if drop_path is not None:
            dmidb = self._b(scr + ".dpb", (R, Wd))  # (the MLP branch's operand is consumed: same stream, nothing deferred)
            K.drop_path_rows(dmid, drop_path[0], drop_path[2], out_bf16=dmidb)
        self._lin_bwd(dmidb, B_[tag + ".att" + r], pre + nm["o_w"], pre + nm["o_b"], datt, R)
        if rows is not None:
            datt_r, datt = datt, self._b(scr + ".datt", (M, Wd))  # token-row indexed like the attention output; only the R rows are read
            K.rows_move("scatter", rows, full_bf16=datt, packed_bf16=datt_r)
        dqkv = self._b(scr + ".dqkv", (M, 3 * Wd))
        delta = self._f(scr + ".delta", (M, heads))
        attn_bwd(B_[tag + ".qkv"], datt, B_[tag + ".att"], B_[tag + ".lse"], delta, dqkv)
        dln = self._b(scr + ".dln", (M, Wd))  # (the dense block: dln_r again)
        self._lin_bwd(dqkv, B_[tag + ".ln1"], pre + nm["qkv_w"], pre + nm["qkv_b"], dln, M)
        # the residual path, + dmid: inside the LayerNorm backward, or at the used rows behind it (fp32 sum, bf16 copy refreshed
        # for those rows)
        self._ln_bwd(dln, x_in, pre + nm["ln1"], tag + ".ln1", dx_in, dx_bf16=dxb_in, res1=dmid if rows is None else None)
        if rows is not None:
            K.rows_move("scatter_add", rows, full_f32=dx_in, full_bf16=dxb_in, packed_f32=dmid)

    def _blocks_fwd(self, pre, nm, x, tag, depth, heads, act, eps, attn, rows=None, attn_rows=None, drop_path=None, recompute="none"):
        """x through the blocks pre + "0." ... of a pre-LN tower -> the stream behind the last block -- or, with `rows`, that
        block's output at those rows (packed; attn_rows: its attention call), for the caller's final LayerNorm and head.
        tag: block l keeps its tensors as tag + "l" + name and writes the stream tag + ".x<l + 1>"; None: forward-only, in place.
        drop_path: (scale table fp32 [2 * depth, B], rows per sample) of a stochastic-depth step, row 2 l for the attention branch of
        block l and 2 l + 1 for its MLP branch (tvts_drop_path_table); None: no stochastic depth.
        recompute (per CALL: the video towers pass the engine's mode, the text towers and the sort head nothing): "mlp" / "block" keep
        the blocks' tensors in the shared slot of _rc_tags; _blocks_bwd evaluates them again."""
        assert recompute == "none" or (tag is not None and rows is None)
        if tag is not None:
            self._rc_fwd[tag] = recompute
        for l in range(depth):
            used = rows if l == depth - 1 else None
            xo = None if used is not None else self._f(f"{tag}.x{l + 1}", x.shape) if tag else x
            tg, tm = self._rc_tags(tag, l, recompute) if tag else (None, None)
            x = self._block_fwd(f"{pre}{l}.", nm, x, xo, tg, heads, act, eps, attn if used is None else attn_rows,
                                rows=used, drop_path=self._dp_of(drop_path, l), mtag=tm)
            if recompute != "none":
                self._rc_held[tm] = l
        return x

    @staticmethod
    def _dp_of(drop_path, l):
        """block l's share of a tower's drop_path argument"""
        return None if drop_path is None else (drop_path[0][2 * l], drop_path[0][2 * l + 1], drop_path[1])

    @staticmethod
    def _ab(depth, l):
        """The gradient stream of a tower of `depth` blocks ping-pongs between two buffers, "A" and "B": what enters the last block
        from behind is in A; -> the one that block l writes the gradient of its input to."""
        return "B" if (depth - l) % 2 == 1 else "A"

    def _head_ln_bwd(self, dy, name, tag, ln_tag, depth, rows, packed):
        """The backward of a tower's final LayerNorm, which read the last block's output at `rows` -> dx, dxb for _blocks_bwd:
        packed [R, Wd] when that block ran on those rows only, over every row (zero off `rows`) otherwise."""
        if packed:
            xo = self.buf[f"{tag}{depth - 1}.xo_r"]
            dx, dxb = self._f(tag + ".dx_r", xo.shape), self._b(tag + ".dxb_r", xo.shape)
            self._ln_bwd(dy, xo, name, ln_tag, dx, dx_bf16=dxb)
        else:
            x = self.buf[f"{tag}.x{depth}"]
            dx, dxb = self._f(tag + ".dxA", x.shape, zero=True), self._b(tag + ".dxbA", x.shape, zero=True)
            self._ln_bwd(dy, x, name, ln_tag, dx, dx_bf16=dxb, rows=rows)
        return dx, dxb

    def _blocks_bwd(self, pre, nm, tag, depth, dx, dxb, heads, act, attn_bwd, rows=None, attn_bwd_rows=None, after=None,
                    drop_path=None, redo=None):
        """The backward of _blocks_fwd (drop_path: the forward's).  dx / dxb: fp32 / bf16 gradient of what it returned -> the fp32 gradient of its input x.
        The blocks' input gradients alternate between tag + ".dxA|B" / ".dxbA|B" (_ab); after(l): called behind block l.
        redo: (eps, the forward's attention call) of a tower that may have run under a recomputation mode (_blocks_fwd): a block whose
        tensors the shared slot no longer holds is evaluated again from its kept input ("block": up to fc1; "mlp": fc1 alone)
        before its backward -- every launch of this stream that read the slot is queued in front of it."""
        mode = self._rc_fwd.get(tag, "none")
        assert mode == "none" or (redo is not None and rows is None)
        for l in reversed(range(depth)):
            x_in, nx, used = self.buf[f"{tag}.x{l}"], self._ab(depth, l), rows if l == depth - 1 else None
            tg, tm = self._rc_tags(tag, l, mode)
            if mode != "none" and self._rc_held.get(tm) != l:
                if mode == "block":
                    self._block_fwd(f"{pre}{l}.", nm, x_in, None, tg, heads, act, redo[0], redo[1], drop_path=self._dp_of(drop_path, l),
                                    mtag=tm, redo=True)
                else:
                    self._lin(self.buf[tg + ".ln2"], f"{pre}{l}." + nm["fc_w"], f"{pre}{l}." + nm["fc_b"], self._b(tm + ".a", (x_in.shape[0], 4 * x_in.shape[1])),
                              x_in.shape[0], act=act, preact=self._b(tm + ".h", (x_in.shape[0], 4 * x_in.shape[1])))
                self._rc_held[tm] = l
                self.recompute_count += 1
            dxi, dxbi = self._f(f"{tag}.dx{nx}", x_in.shape), self._b(f"{tag}.dxb{nx}", x_in.shape)
            self._block_bwd(f"{pre}{l}.", nm, x_in, dx, dxb, dxi, dxbi, tg, tag + ".s", heads, act,
                            attn_bwd if used is None else attn_bwd_rows, rows=used, drop_path=self._dp_of(drop_path, l), mtag=tm)
            dx, dxb = dxi, dxbi
            if after is not None:
                after(l)
        return dx

    # ------------------------------------------------------------------ text tower
    @staticmethod
    def eot_index(eot_rows, L):
        """(None, int32 position of the EOT token inside its caption).  prepare_batch hands the positions over with the batch (made on
        the host, so that their lifetime is the batch's -- and that of a hipGraph captured over it); this form derives them from
        the rows for callers that drive text_forward by hand."""
        pos = (eot_rows - torch.arange(eot_rows.numel(), device=eot_rows.device, dtype=torch.int32) * L).contiguous()
        return None, pos

    def text_forward(self, ids_dev, eot_rows, N, L, eot_index=None, packed=None):
        """eot_index: Engine.eot_index(eot_rows, L) kept by the caller (prepare_batch); made here when absent (eager use only).
        packed: the batch of prepare_batch under arch["text_packed"] (its seq_start, M, max_len) -- ids_dev is then int32 [M], every
        caption cut behind its EOT token, eot_rows = seq_start[1:] - 1, and the tower runs over those M rows.  M is whatever the
        captions add up to, odd and prime included: the GEMMs of the text blocks take any row count and any contraction length (their
        tile tails are masked), so the packed buffers carry no padding rows."""
        if packed is not None:
            ht, ss, ml = self.arch["text_heads"], packed["seq_start"], packed["max_len"]
            return self._text_tower(
                lambda x: K.text_embed_packed(ids_dev, ss, self.P.p("text_token_embedding.weight"),
                                              self.P.p("text_positional_embedding"), x, N=N),
                lambda qkv, att, lse: K.attn_fwd_packed(qkv, ss, att, N=N, heads=ht, max_len=ml, lse2=lse),
                lambda qkv, att, lse: K.attn_fwd_packed(qkv, ss, att, N=N, heads=ht, max_len=ml, last_only=True, lse2=lse),
                eot_rows, N, packed["M"], "txt")
        t, self._text_eot = self._text_padded(ids_dev, eot_rows, N, L, eot_index, "txt")  # (the backward takes the positions from here)
        return t

    def _text_padded(self, ids_dev, eot_rows, N, L, eot_index, tag):
        """the text tower over N captions padded to L rows each -> (embeddings, the eot_index used)"""
        ht, hd = self.arch["text_heads"], self.dh_text
        if eot_index is None and self.text_used_rows_only:
            eot_index = self.eot_index(eot_rows, L)
        pos = None if eot_index is None else eot_index[1]
        t = self._text_tower(
            lambda x: K.text_embed(ids_dev, self.P.p("text_token_embedding.weight"), self.P.p("text_positional_embedding"), x, N=N, L=L),
            lambda qkv, att, lse: K.attn_fwd("full", qkv, att, lse, B=N, heads=ht, S=L, causal=True, head_dim=hd),
            lambda qkv, att, lse: K.attn_fwd_rowq(qkv, pos, att, lse, B=N, heads=ht, S=L, head_dim=hd), eot_rows, N, N * L, tag)
        return t, eot_index

    def _text_tower(self, embed, attn, attn_last, eot_rows, N, M, tag=None):
        """The CLIP text tower over the M token rows of N captions -> [N, E] fp32 caption embeddings.  embed(x): the embedding
        kernel; attn / attn_last(qkv, att, lse): the attention call of a block / of the last block, whose only queries are the rows
        eot_rows; tag: "txt" in the training step, None forward-only (one stream buffer, updated in place)."""
        a, w = self.arch, self._w
        Wt = a["text_width"]
        x = w(tag, ".x0", "x", (M, Wt), torch.float32)
        embed(x)
        # the model reads the last block's output at the EOT token of every caption only (CLIP/clip/model.py:343-354)
        packed = self.text_used_rows_only
        x = self._blocks_fwd("text_model.resblocks.", _TEXT_NAMES, x, tag, a["text_layers"], a["text_heads"], a["act"], 1e-5, attn,
                             eot_rows if packed else None, attn_last)
        lnf = w(tag, ".lnf", "lnpc", (N, Wt), torch.float32)
        self._ln(x, "text_ln_final", 1e-5, lnf, tag and tag + ".lnf", rows=None if packed else eot_rows)
        t = w(tag, ".t", "temb", (N, a["embed"]), torch.float32)
        K.gemm_small(lnf, self.P.p("text_projection"), t, M=N, N=a["embed"], K=Wt, sa=(Wt, 1), sb=(a["embed"], 1))
        return t

    def text_backward(self, dt, ids_dev, eot_rows, N, L, tok_sort=None, packed=None):
        """packed: as text_forward (the same batch); tok_sort is then the plan over the packed ids and packed["pos_sort"] the
        position plan of tvts_text_embed_bwd_packed."""
        a = self.arch
        Wt, E = a["text_width"], a["embed"]
        lnf = self.buf["txt.lnf"]
        if self.requires_grad["text_projection"]:  # dproj[Wt,E] += lnf^T dt
            K.gemm_small(lnf, dt, self.P.g("text_projection"), M=Wt, N=E, K=N, sa=(1, Wt), sb=(E, 1), accumulate=True)
        dlnf = self._f("txt.dlnf", (N, Wt))
        K.gemm_small(dt, self.P.p("text_projection"), dlnf, M=N, N=Wt, K=E, sa=(E, 1), sb=(1, E))
        used = self.text_used_rows_only  # the gradient of the last block's output exists at the EOT rows only: [N, Wt]
        dx, dxb = self._head_ln_bwd(dlnf, "text_ln_final", "txt", "txt.lnf", a["text_layers"], eot_rows, used)
        ht, hd = a["text_heads"], self.dh_text
        if packed is not None:
            ss, ml = packed["seq_start"], packed["max_len"]
            attn_bwd = lambda qkv, *t: K.attn_bwd_packed(qkv, ss, *t, N=N, heads=ht, max_len=ml)  # noqa: E731
            attn_bwd_last = lambda qkv, *t: K.attn_bwd_packed(qkv, ss, *t, N=N, heads=ht, max_len=ml, last_only=True)  # noqa: E731
        else:
            pos = self._text_eot[1] if used else None  # the forward's tensor (the batch's when it came through prepare_batch)
            attn_bwd = lambda qkv, *t: K.attn_bwd("full", qkv, *t, B=N, heads=ht, S=L, causal=True, head_dim=hd)  # noqa: E731
            attn_bwd_last = lambda qkv, *t: K.attn_bwd_rowq(qkv, pos, *t, B=N, heads=ht, S=L, head_dim=hd)  # noqa: E731
        dx = self._blocks_bwd("text_model.resblocks.", _TEXT_NAMES, "txt", a["text_layers"], dx, dxb, ht, a["act"], attn_bwd,
                              eot_rows if used else None, attn_bwd_last)
        if self.requires_grad["text_token_embedding.weight"] or self.requires_grad["text_positional_embedding"]:
            demb, dpos = self.P.g("text_token_embedding.weight"), self.P.g("text_positional_embedding")
            if packed is not None:
                K.text_embed_bwd_packed(dx, ids_dev, ss, demb, dpos, N=N, tok_sort=tok_sort, pos_sort=packed["pos_sort"])
            else:
                K.text_embed_bwd(dx, ids_dev, demb, dpos, N=N, L=L, tok_sort=tok_sort)

    # ------------------------------------------------------------------ video tower
    def _attn_q8(self, M, W, name, T, n, persistent=False, consumer=None):
        """the divided-attention kernels write the per-tensor e4m3 copy of their result themselves (tensor mode, fused geometries;
        arch["fp8_attn_copies"] = False keeps the quantiser pass: same bytes, tests/test_model_gpu.py::test_fp8_wgrad_path)"""
        if not (self.fp8_wgrad and self._f8_tensor_mode and self.arch.get("fp8_attn_copies", True)) or n + 1 > 112 or T + 1 > 32:
            return {}, None
        q, sc, kw = self._q8(M, W, name, persistent=persistent)
        out = dict(q8out=q, q8_scale=sc, q8_amax=kw["amax"])
        # arch["fp8_q8_only"]: the e4m3 bytes are the kernels' only output for the patch rows -- every consumer of the attention
        # output (projection forward / weight gradient) and of the attention input gradient (qkv input / weight / bias gradient)
        # multiplies the e4m3 copy; the CLS rows, which the CLS-row delta, the hybrid stream's fix-up GEMM and the merge / finalize
        # kernels touch, keep both forms
        if self.fp8_q8_only and consumer is not None and self.requires_grad[consumer]:
            out["q8_only"] = True
        return out, (q, sc)

    def _st_attention_fwd(self, qkv, att, lse, mode, B, T, n, q8_for=None):
        """lse None: forward-only (no log-sum-exp is stored; full-frame SPACE calls take their own fused kernel, attention.hip)"""
        h, S = self.arch["heads"], 1 + T * n
        ws = self._w(None if lse is None else "vit", ".clsws", "clsws", (B * h * max(T, -(-n // 28)) * (self.dh + 2),), torch.float32)
        kw8 = {}
        if lse is not None and q8_for is not None and q8_for in self.P.w8:  # (forward-only: per token, the projection quantises)
            kw8, nxt = self._attn_q8(B * S, att.shape[1], "x." + q8_for, T, n, persistent=True, consumer=q8_for)
            if nxt is not None:
                self._x8_ready[q8_for] = nxt
        K.attn_fwd_divided(mode, qkv, att, lse, ws, B=B, heads=h, S=S, T=T, n=n, head_dim=self.dh, **kw8)

    def _st_attention_bwd(self, qkv, att, datt, lse, dqkv, mode, B, T, n, scr, q8_for=None):
        h, S = self.arch["heads"], 1 + T * n
        M = B * S
        kw8 = {}
        if q8_for is not None and q8_for in self.P.w8t:
            kw8, nxt = self._attn_q8(M, dqkv.shape[1], "dy." + q8_for, T, n, consumer=q8_for if q8_for in self._x8 else None)
            if nxt is not None:
                self._dy8_ready[q8_for] = nxt
        delta = self._f(scr + ".delta", (M, h))
        hd = self.dh
        # one partial of the CLS token's dK / dV / dQ per block of the fused kernels, added in order (no atomics)
        cls_acc = self._f(scr + ".clsacc", (B, h, max(T, -(-n // 28)), 3, hd))
        K.attn_bwd(mode, qkv, datt, att, lse, delta, dqkv, B=B, heads=h, S=S, T=T, n=n, cls_acc=cls_acc, head_dim=hd, **kw8)

    def _vit_embed(self, video, keep_dev, B, T, vid_rows, crop, resize, tag, gather=None):
        """patch gather (fp32 clips, uint8 frames or, with gather = dict(desc, tables), the packed ragged uint8 clips) -> conv GEMM -> token assembly -> ln_pre: (the residual stream x [B * S, W],
        the fp32 CLS rows [B, W] of the hybrid stream or None).  Forward-only (tag None) the fp32 temporaries live in the roles of
        the first block's LayerNorm, MLP and qkv buffers (free until then)."""
        a, w = self.arch, self._w
        W, p, n = a["width"], a["patch"], keep_dev.shape[1]
        M, Mp = B * (1 + T * n), B * T * n
        cols = w(tag, ".im2col", "ln", (Mp, self.P.conv_kpad))
        if gather is not None:
            K.patch_gather_u8_ragged(video, gather["desc"], gather["tables"], keep_dev, cols, B=B, T=T, n=n, img=a["image"], patch=p)
        elif video.dtype == torch.uint8:
            K.patch_gather_u8(video, keep_dev, cols, B=B, T=T, n=n, img=a["image"], patch=p, crop=crop, resize=resize)
        else:
            K.patch_gather(video, keep_dev, cols, B=B, T=T, n=n, img=a["image"], patch=p)
        pe = w(tag, ".patch", "h", (Mp, W), torch.float32)
        K.gemm_nt(cols, self.P.w_conv(), pe, M=Mp)
        tok = w(tag, ".tok", "qkv", (M, W), torch.float32)
        K.vit_assemble(pe, self.P.p("video_model.class_embedding"), self.P.p("video_model.positional_embedding"),
                       self.P.p("video_model.temporal_embedding"), keep_dev, tok, B=B, T=T, n=n)
        x = w(tag, ".x0", "x", (M, W), torch.bfloat16 if self.bf16_residual else torch.float32)  # the residual stream: bf16 or fp32
        self._ln(tok, "video_model.ln_pre", 1e-5, x, tag and tag + ".lnpre")
        xc = None
        if self.cls32:  # the hybrid stream's CLS rows start as ln_pre's fp32 output on those rows
            xc = w(tag, ".xc0", "xc", (B, W), torch.float32)
            self._ln(tok, "video_model.ln_pre", 1e-5, xc, tag and tag + ".lnpre_c", rows=vid_rows)
        return x, xc

    def _vit_block_head(self, pre, x, xc, tg, B, T, n):
        """What every row of a space-time block goes through in both passes, up to the space attention's input:
        ln_3 -> time qkv -> time attention -> t_res -> ln_1 -> space qkv.  -> qkv_s"""
        a, w = self.arch, self._w
        W, M, fo = a["width"], x.shape[0], tg is None
        ln3 = w(tg, ".ln3", "ln", (M, W))
        a8 = self._ln(x, pre + "ln_3", 1e-5, ln3, tg and tg + ".ln3", fp8_for=pre + "timeattn.qkv.weight", cls_x=xc)
        qkv_t = w(tg, ".qkv_t", "qkv", (M, 3 * W))
        self._lin(ln3, pre + "timeattn.qkv.weight", pre + "timeattn.qkv.bias", qkv_t, M, a8=a8, fwd_only=fo)
        att_t, lse_t = w(tg, ".att_t", "att", (M, W)), (self._f(tg + ".lse_t", (M, a["heads"])) if tg else None)
        self._st_attention_fwd(qkv_t, att_t, lse_t, "time", B, T, n, q8_for=pre + "timeattn.proj.weight")
        # the time residual only feeds ln_1 (the space branch restarts from x, video_encoder_ViT_B_16.py:121): bf16
        t_res = w(tg, ".t_res", "tres", (M, W))
        self._lin(att_t, pre + "timeattn.proj.weight", pre + "timeattn.proj.bias", t_res, M, residual=x, fwd_only=fo)
        ln1 = w(tg, ".ln1", "ln", (M, W))
        a8 = self._ln(t_res, pre + "ln_1", 1e-5, ln1, tg and tg + ".ln1", fp8_for=pre + "attn.qkv.weight")
        qkv_s = w(tg, ".qkv_s", "qkv", (M, 3 * W))
        self._lin(ln1, pre + "attn.qkv.weight", pre + "attn.qkv.bias", qkv_s, M, a8=a8, fwd_only=fo)
        return qkv_s

    def _vit_block(self, l, x, xc, tag, B, T, n, recompute="none", redo=False):
        """space-time block l on every row: (x, xc) -> the next (x, xc); forward-only (tag None) in place.
        recompute: the training step's mode -- the block's tensors go where _rc_tags says; redo: the backward's second evaluation,
        which stops behind fc1 (the block's output is the kept stream)."""
        a, w = self.arch, self._w
        pre = f"video_model.transformer.resblocks.{l}."
        tg, tm = self._rc_tags(tag, l, recompute, parity=bool(self.wgrad_stream)) if tag else (None, None)
        W, M, S, fo = a["width"], x.shape[0], 1 + T * n, tag is None
        qkv_s = self._vit_block_head(pre, x, xc, tg, B, T, n)
        att_s, lse_s = w(tg, ".att_s", "att", (M, W)), (self._f(tg + ".lse_s", (M, a["heads"])) if tg else None)
        self._st_attention_fwd(qkv_s, att_s, lse_s, "space", B, T, n, q8_for=pre + "attn.proj.weight")
        s_res = w(tg, ".s_res", "s", (M, W), x.dtype)  # residual from the block INPUT x (video_encoder_ViT_B_16.py:121)
        self._lin(att_s, pre + "attn.proj.weight", pre + "attn.proj.bias", s_res, M, residual=x, fwd_only=fo)
        s_res_c = None
        if xc is not None:
            s_res_c = w(tg, ".s_res_c", "sc", (B, W), torch.float32)
            self._cls_lin(att_s, S, pre + "attn.proj.weight", pre + "attn.proj.bias", xc, s_res_c, fwd_only=fo)
        ln2 = w(tg, ".ln2", "ln", (M, W))
        a8 = self._ln(s_res, pre + "ln_2", 1e-5, ln2, tg and tg + ".ln2", fp8_for=pre + "mlp.c_fc.weight", cls_x=s_res_c)
        h, act = (self._b(tm + ".h", (M, 4 * W)) if tg else None), w(tm, ".a", "h", (M, 4 * W))
        self._lin(ln2, pre + "mlp.c_fc.weight", pre + "mlp.c_fc.bias", act, M, act=a["act"], preact=h, a8=a8,
                  q8_for=pre + "mlp.c_proj.weight", fwd_only=fo)
        if recompute != "none":
            self._rc_held[tm] = l
        if redo:
            return None, None
        xo = self._b(f"{tag}.x{l + 1}", (M, W), x.dtype) if tag else x  # (forward-only: x is dead)
        self._lin(act, pre + "mlp.c_proj.weight", pre + "mlp.c_proj.bias", xo, M, residual=s_res, fwd_only=fo)
        if xc is not None:
            xcn = self._f(f"{tag}.xc{l + 1}", (B, W)) if tag else xc
            self._cls_lin(act, S, pre + "mlp.c_proj.weight", pre + "mlp.c_proj.bias", s_res_c, xcn, fwd_only=fo)
            xc = xcn
        return xo, xc

    def video_forward(self, video, keep_dev, B, T, vid_rows=None):
        a = self.arch
        W, E = a["width"], a["embed"]
        n = keep_dev.shape[1]
        S = 1 + T * n
        M = B * S
        lowres, cls = self.bf16_residual, self.cls32
        if vid_rows is None:
            vid_rows = (torch.arange(B, device=self.dev) * S).to(torch.int32)
        x, xc = self._vit_embed(video, keep_dev, B, T, vid_rows, self.ctx.get("crop"), self.ctx.get("resize"), "vit",
                                   gather=self.ctx.get("gather"))
        rc = self._rc_fwd["vit"] = self.recompute
        for l in range(a["layers"]):
            x, xc = self._vit_block(l, x, xc, "vit", B, T, n, recompute=rc)
        out = self._f("vit.out", (M, E))
        if not self.pooled_tail:  # B models: ln_post on every token, all S projected rows feed the sort head
            lnp = self._b("vit.lnpost", (M, W))
            self._ln(x, "video_model.ln_post", 1e-5, lnp, "vit.lnpost", cls_x=xc)
            K.gemm_nt(lnp, self.P.wt("video_model.proj"), out, M=M)  # x @ proj, proj stored [W,E]
            return out, None
        # H/14 (video_encoder_ViT_H_14.py:472-484): pooled = ln_post(CLS) @ proj in fp32; the patch tokens are projected
        # WITHOUT ln_post (row 0 of each clip is computed too but never read: sort_assemble takes rows 1..S-1)
        if lowres:
            xb = self.buf["vit.xlast_b"] = x  # the stream is bf16 already
        else:
            xb = self._b("vit.xlast_b", (M, W))
            K.cast_f32_bf16(x, xb)
        K.gemm_nt(xb, self.P.wt("video_model.proj"), out, M=M)
        lnc = self._f("vit.lnpost_cls", (B, W))
        if cls:  # ln_post on the exact CLS rows of the hybrid stream
            self.buf["vit.xcls32"] = xc
            self._ln(xc, "video_model.ln_post", 1e-5, lnc, "vit.lnpost")
        elif lowres:  # ln_post on the B CLS rows in fp32: an fp32 copy of those rows (plumbing on [B, W])
            xc, xcb = self._f("vit.xcls32", (B, W)), self._b("vit.xcls16", (B, W))
            K.rows_move("gather", vid_rows, full_bf16=x, packed_f32=xc, packed_bf16=xcb)
            self._ln(xc, "video_model.ln_post", 1e-5, lnc, "vit.lnpost")
        else:
            self._ln(x, "video_model.ln_post", 1e-5, lnc, "vit.lnpost", rows=vid_rows)
        pooled = self._f("vit.pooled", (B, E))
        K.gemm_small(lnc, self.P.p("video_model.proj"), pooled, M=B, N=E, K=W, sa=(W, 1), sb=(E, 1))
        return out, pooled

    def _vit_tail_bwd(self, dout_b, d_pooled, B, M):
        """The backward of video_forward's two tails (all tokens / pooled + patches) -> dx, dxb: the fp32 / bf16 gradient of the
        last block's output (dx None where only the bf16 one is kept), dxc: its fp32 CLS rows [B, W] in the hybrid stream, dxb8:
        the e4m3 copy of dxb when ln_post's backward wrote one."""
        a, B_, rg = self.arch, self.buf, self.requires_grad
        W, E = a["width"], a["embed"]
        lowp, cls = self.bf16_grad_stream, self.cls32
        dxc = None
        dxb = self._b("vit.dxbA", (M, W))
        dx = None if (lowp and not self.pooled_tail) else self._f("vit.dxA", (M, W))
        if not self.pooled_tail:
            dln = self._b("vit.s.dln", (M, W))
            if rg["video_model.proj"]:  # dproj[W,E] += lnpost^T dout
                K.gemm_tn(B_["vit.lnpost"], dout_b, self.P.g("video_model.proj"), M=M, accumulate=True)
            K.gemm_nt(dout_b, self.P.w("video_model.proj"), dln, M=M)
            if cls:
                dxc = self._f("vit.dxcA", (B, W))
            dxb8 = self._ln_bwd(dln, B_[f"vit.x{a['layers']}"], "video_model.ln_post", "vit.lnpost", dx, dx_bf16=dxb,
                                fp8_for=f"video_model.transformer.resblocks.{a['layers'] - 1}.mlp.c_proj.weight",
                                cls_x=B_[f"vit.xc{a['layers']}"] if cls else None, cls_dx=dxc)
            return dx, dxb, dxc, dxb8
        # patch-token branch (no LN): dproj += x^T dout, dx = dout proj^T (CLS rows of dout are zero)
        if dout_b is not None:
            if rg["video_model.proj"]:
                K.gemm_tn(B_["vit.xlast_b"], dout_b, self.P.g("video_model.proj"), M=M, accumulate=True)
            K.gemm_nt(dout_b, self.P.w("video_model.proj"), dx, M=M)
        else:
            K.zero_(dx)
        # pooled branch, fp32: dproj += lnc^T d_pooled, d_lnc = d_pooled proj^T, ln_post backward on the CLS rows only
        lnc = B_["vit.lnpost_cls"]
        if rg["video_model.proj"]:
            K.gemm_small(lnc, d_pooled, self.P.g("video_model.proj"), M=W, N=E, K=B, sa=(1, W), sb=(E, 1), accumulate=True)
        dlnc = self._f("vit.s.dlnc", (B, W))
        K.gemm_small(d_pooled, self.P.p("video_model.proj"), dlnc, M=B, N=W, K=E, sa=(E, 1), sb=(1, E))
        if self.bf16_residual:  # ln_post backward on the fp32 copy of the CLS rows, added into those rows of dx
            # (hybrid stream: those rows of dx are zero -- no gradient enters the CLS rows through the patch-token branch -- so
            # the LayerNorm's result IS the fp32 CLS chain's first value)
            dc = self._f("vit.dxcA" if cls else "vit.s.dxcls", (B, W))
            self._ln_bwd(dlnc, B_["vit.xcls32"], "video_model.ln_post", "vit.lnpost", dc)
            K.rows_move("scatter_add", self.ctx["vid_rows"], full_f32=dx, packed_f32=dc)
            dxc = dc if cls else None
        else:
            self._ln_bwd(dlnc, B_[f"vit.x{a['layers']}"], "video_model.ln_post", "vit.lnpost", dx, res1=dx,
                         rows=self.ctx["vid_rows"])
        K.cast_f32_bf16(dx, dxb)
        return dx, dxb, dxc, None

    def _vit_block_bwd(self, l, dx, dxb, dxc, dxb8, B, T, n, par, wg, join):
        """Space-time block l backward, the mirror of _vit_block: the gradient of its output (dx, dxb, dxc, dxb8 as _vit_tail_bwd
        returns them) -> the same four for its input.  wg: what every weight gradient's _lin_bwd is told (side, defer); par: suffix
        of the buffers those weight gradients read late; join(): called once all six are issued, before the block's input
        gradient is written."""
        a, B_ = self.arch, self.buf
        pre = f"video_model.transformer.resblocks.{l}."
        tg, tm = self._rc_tags("vit", l, self._rc_fwd.get("vit", "none"), parity=bool(self.wgrad_stream))
        M, W = dxb.shape
        # the residual-stream gradient in bf16 (self.bf16_grad_stream, see __init__): measured alone +1.4 % (the three LayerNorm
        # backwards of a block move 3.2 instead of 4.6 GB) at 2.4x the error of the embedding-side gradients, which sit behind
        # ln_pre's cancellation (5.8 % instead of 2.4 % rel-L2; profiles/r03_bf16_streams_ab.txt)
        lowp = self.bf16_grad_stream
        cls = self.cls32   # hybrid stream: the CLS rows of the gradient chain in fp32 side arrays dxc / dsrc [B, W]
        dln, datt = self._b("vit.s.dln", (M, W)), self._b("vit.s.datt", (M, W))
        dsr = None if lowp else self._f("vit.s.dsres", (M, W))
        dh = self._b("vit.s.dh" + par, (M, 4 * W))
        dsrb = self._b("vit.s.dsresb" + par, (M, W))
        dtrb = self._b("vit.s.dtresb" + par, (M, W))
        dqkv = self._b("vit.s.dqkv" + par, (M, 3 * W))
        dqkv_t = self._b("vit.s.dqkv_t" + par, (M, 3 * W)) if (wg["side"] or wg["defer"] is not None) else dqkv
        # (e4m3 input gradients: the LayerNorm backward that produces an output gradient also writes its e4m3 copy, d*8)
        self._lin_bwd(dxb, B_[tm + ".a"], pre + "mlp.c_proj.weight", pre + "mlp.c_proj.bias", dh, M, dy8=dxb8,
                      q8_for=pre + "mlp.c_fc.weight", gate_h=B_[tm + ".h"], gate_act=a["act"], **wg)
        self._lin_bwd(dh, B_[tg + ".ln2"], pre + "mlp.c_fc.weight", pre + "mlp.c_fc.bias", dln, M, **wg)
        dsrc = self._f("vit.s.dsrc", (B, W)) if cls else None
        dsrb8 = self._ln_bwd(dln, B_[tg + ".s_res"], pre + "ln_2", tg + ".ln2", dsr, dx_bf16=dsrb, res1=dxb if lowp else dx,
                             fp8_for=pre + "attn.proj.weight", cls_x=B_[tg + ".s_res_c"] if cls else None,
                             cls_res1=dxc, cls_dx=dsrc)
        # spatial attention branch
        self._lin_bwd(dsrb, B_[tg + ".att_s"], pre + "attn.proj.weight", pre + "attn.proj.bias", datt, M, dy8=dsrb8, **wg)
        self._st_attention_bwd(B_[tg + ".qkv_s"], B_[tg + ".att_s"], datt, B_[tg + ".lse_s"], dqkv, "space", B, T, n, "vit.s",
                               q8_for=pre + "attn.qkv.weight")
        self._lin_bwd(dqkv, B_[tg + ".ln1"], pre + "attn.qkv.weight", pre + "attn.qkv.bias", dln, M, **wg)
        # the time-residual gradient is a side branch (t_res only feeds ln_1): it lives in bf16 only -- as the operand of
        # the timeattn.proj GEMMs and as the bf16 residual term of the ln_3 backward
        dtrb8 = self._ln_bwd(dln, B_[tg + ".t_res"], pre + "ln_1", tg + ".ln1", None, dx_bf16=dtrb,
                             fp8_for=pre + "timeattn.proj.weight")
        # temporal attention branch
        self._lin_bwd(dtrb, B_[tg + ".att_t"], pre + "timeattn.proj.weight", pre + "timeattn.proj.bias", datt, M, dy8=dtrb8, **wg)
        self._st_attention_bwd(B_[tg + ".qkv_t"], B_[tg + ".att_t"], datt, B_[tg + ".lse_t"], dqkv_t, "time", B, T, n, "vit.s",
                               q8_for=pre + "timeattn.qkv.weight")
        self._lin_bwd(dqkv_t, B_[tg + ".ln3"], pre + "timeattn.qkv.weight", pre + "timeattn.qkv.bias", dln, M, **wg)
        join()
        nx = self._ab(a["layers"], l)
        dxbi = self._b("vit.dxb" + nx, (M, W))
        dxi = None if lowp else self._f("vit.dx" + nx, (M, W))
        # x feeds ln_3, the time residual and the space residual
        dxci = self._f("vit.dxc" + nx, (B, W)) if cls else None
        dxb8 = self._ln_bwd(dln, B_[f"vit.x{l}"], pre + "ln_3", tg + ".ln3", dxi, dx_bf16=dxbi, res1=dsrb if lowp else dsr, res2=dtrb,
                            fp8_for=f"video_model.transformer.resblocks.{l - 1}.mlp.c_proj.weight" if l > 0 else None,
                            cls_x=B_[f"vit.xc{l}"] if cls else None, cls_res1=dsrc, cls_dx=dxci)
        return dxi, dxbi, dxci, dxb8

    def _vit_redo(self, l, B, T, n):
        """Under a recomputation mode, in front of block l's backward: evaluate the block again unless its slot still holds it (the
        forward's last writer).  "block": its training forward from the kept x<l> / xc<l>, up to fc1; "mlp": fc1 from the kept ln2.
        The slot's earlier readers are queued in front of this on the current stream -- the grouped weight gradients of block l + 1
        are launched inside that block's backward (join), and the side stream's readers of this parity's slot (block l + 2) were
        joined there as well (video_backward)."""
        mode = self._rc_fwd.get("vit", "none")
        if mode == "none":
            return
        tg, tm = self._rc_tags("vit", l, mode, parity=bool(self.wgrad_stream))
        if self._rc_held.get(tm) == l:
            return
        B_, a = self.buf, self.arch
        if mode == "block":
            self._vit_block(l, B_[f"vit.x{l}"], B_[f"vit.xc{l}"] if self.cls32 else None, "vit", B, T, n, recompute=mode, redo=True)
        else:
            pre, x = f"video_model.transformer.resblocks.{l}.", B_[f"vit.x{l}"]
            M, W = x.shape
            self._lin(B_[tg + ".ln2"], pre + "mlp.c_fc.weight", pre + "mlp.c_fc.bias", self._b(tm + ".a", (M, 4 * W)), M, act=a["act"],
                      preact=self._b(tm + ".h", (M, 4 * W)))
            self._rc_held[tm] = l
        self.recompute_count += 1

    def _vit_embed_bwd(self, dx, keep_dev, B, T):
        """The backward of _vit_embed: ln_pre -> token assembly -> conv weight gradient; the embedding stage's gradients are final."""
        B_ = self.buf
        W, n = self.arch["width"], keep_dev.shape[1]
        M, Mp = B * (1 + T * n), B * T * n
        dtok = self._f("vit.dtok", (M, W))
        self._ln_bwd(dx, B_["vit.tok"], "video_model.ln_pre", "vit.lnpre", dtok)
        dpatch = self._b("vit.dpatch", (Mp, W))
        K.vit_assemble_bwd(dtok, keep_dev, dpatch, self.P.g("video_model.class_embedding"),
                           self.P.g("video_model.positional_embedding"), self.P.g("video_model.temporal_embedding"),
                           B=B, T=T, n=n)
        if self.requires_grad["video_model.conv1.weight"]:
            if self.P.conv_pad is None:
                K.gemm_tn(dpatch, B_["vit.im2col"], self.P.g2d("video_model.conv1.weight"), M=Mp, accumulate=True)
            else:  # K padded to 64: wgrad into a [W, Kpad] scratch, the 588 real columns are folded into the gradient
                scr = self._f("vit.s.dconv", (W, self.P.conv_kpad))
                K.gemm_tn(dpatch, B_["vit.im2col"], scr, M=Mp, accumulate=False)
                K.add_rows_f32(self.P.g2d("video_model.conv1.weight"), scr)
        self._ready("video_model.class_embedding", "video_model.positional_embedding", "video_model.proj",
                    "video_model.temporal_embedding", "video_model.conv1.", "video_model.ln_pre.")
        self._ready("video_model.ln_post.")

    def video_backward(self, dout_b, keep_dev, B, T, d_pooled=None):
        """dout_b: bf16 [B*S, E] grad of the projected tokens (B models: CLS rows carry the embedding grad; H/14: None
        when there is no sorting loss); d_pooled: fp32 [B, E] grad of the pooled embedding (H/14 only)."""
        n = keep_dev.shape[1]
        M = B * (1 + T * n)
        self.recompute_count = 0
        dx, dxb, dxc, dxb8 = self._vit_tail_bwd(dout_b, d_pooled, B, M)
        # the weight gradients of the blocks on the side stream: the output gradients they read (dh, dsrb, dqkv of the space and of
        # the time branch, dtrb, and the block's own dxb) then live in buffers of the layer's parity, and the chain joins the side
        # stream's work of layer l + 1 before layer l overwrites the first of them (its ln_3 backward writes the dxb that layer
        # l + 1 read) -- the side stream may lag one layer behind, never two
        # (not with e4m3 weight gradients in tensor mode: those never take the side branch of _lin_bwd)
        side = self._wgrad_side(M) and not (self.fp8_wgrad and self._f8_tensor_mode)
        grouped = self._tn_grouped_on(M)
        side_done = {}
        cur = torch.cuda.current_stream(self.dev)
        if side:
            self._side()  # the stream exists before anything records on it or joins it (all weights frozen: no launch creates it)
        for l in reversed(range(self.arch["layers"])):
            defer = [] if grouped else None

            def join(l=l, defer=defer):
                if grouped:  # the block's six weight gradients (+ bias gradients) in one launch, their partials in one reduce launch:
                    self._tn_group_run(l, defer)  # every output gradient they read is still intact (dqkv of the two branches apart)
                if side:
                    side_done[l] = torch.cuda.Event()
                    side_done[l].record(self._wg_stream)
                    if l + 1 in side_done:  # layer l + 1's weight gradients are final: its dxb may be overwritten, its range may travel
                        cur.wait_event(side_done.pop(l + 1))
                        self._ready(f"video_model.transformer.resblocks.{l + 1}.")

            self._vit_redo(l, B, T, n)
            dx, dxb, dxc, dxb8 = self._vit_block_bwd(l, dx, dxb, dxc, dxb8, B, T, n, str(l % 2) if side else "",
                                                     dict(side=side, defer=defer), join)
            if not side:
                self._ready(f"video_model.transformer.resblocks.{l}.")
        if side:
            cur.wait_stream(self._wg_stream)
            self._ready("video_model.transformer.resblocks.0.")
        self._vit_embed_bwd(dxb if self.bf16_grad_stream else dx, keep_dev, B, T)

    # ------------------------------------------------------------------ sort head
    # SortTransformer.forward_features normalises and classifies x[:, x_len:] only (v2/model/sort_transformer.py:131-141): of the last
    # block's [B, Sv + NT, E] output the NT transcript rows of every sample are read, the Sv video rows never are, and no gradient
    # enters them.  So the LAST block runs on those R = B * NT rows (_block_fwd with rows): same loss, same gradient for every
    # parameter and every input row as the dense evaluation (tests/test_model_gpu.py::test_sort_head_used_rows_only);
    # arch["sort_used_rows_only"] = False evaluates the block densely like the reference does.
    def sort_forward(self, out, text_before, B, S, NT):
        a = self.arch
        E, hs, depth = self.sort_width, a["sort_heads"], a["sort_depth"]
        off = 1 if self.pooled_tail else 0  # H/14 hands the sort head the patch tokens without CLS
        Sv = S - off
        So = Sv + NT
        xs = self._f("srt.x0", (B * So, E))
        K.sort_assemble(out, text_before, self.P.p("pred_model.type_embed").view(2, E), xs, B=B, S=S, off=off, Sv=Sv, NT=NT)
        rows, packed = self.ctx["sort_rows"], self.sort_used_rows_only and NT <= 16
        x = self._blocks_fwd(
            "pred_model.blocks.", _SORT_NAMES, xs, "srt", depth, hs, "gelu", 1e-6,
            lambda qkv, att, lse: K.attn_fwd("full", qkv, att, lse, B=B, heads=hs, S=So, causal=False, head_dim=E // hs),
            rows if packed else None,
            lambda qkv, att, lse: K.attn_fwd_tail(qkv, att, lse, B=B, heads=hs, S=So, nq=NT, head_dim=E // hs))
        nf = self._f("srt.nf", (B * NT, E))
        self._ln(x, "pred_model.norm", 1e-6, nf, "srt.norm", rows=None if packed else rows)
        pred = self._f("srt.pred", (B * NT, a["n_trans"]))
        self._head_lin(nf, "pred_model.head.weight", "pred_model.head.bias", pred, B * NT)
        return pred

    def sort_backward(self, dpred, B, S, NT):
        """-> fp32 grad of the sort-head input xs [B*So, E]."""
        a, B_ = self.arch, self.buf
        E, hs, depth = self.sort_width, a["sort_heads"], a["sort_depth"]
        So = S - (1 if self.pooled_tail else 0) + NT
        R = B * NT
        dnf = self._f("srt.dnf", (R, E))
        self._head_lin_bwd(dpred, B_["srt.nf"], "pred_model.head.weight", "pred_model.head.bias", dnf, R)
        rows, packed = self.ctx["sort_rows"], self.sort_used_rows_only and NT <= 16  # (gradient at the transcript rows only: [R, E])
        dx, dxb = self._head_ln_bwd(dnf, "pred_model.norm", "srt", "srt.norm", depth, rows, packed)

        def attn_bwd_rows(qkv, datt, att, lse, delta, dqkv):
            K.zero_cols_bf16(dqkv, E)  # dQ of the rows that are no queries (dK / dV are written for every row)
            K.attn_bwd_tail(qkv, datt, att, lse, delta, dqkv, B=B, heads=hs, S=So, nq=NT, head_dim=E // hs)
        return self._blocks_bwd(
            "pred_model.blocks.", _SORT_NAMES, "srt", depth, dx, dxb, hs, "gelu",
            lambda qkv, *t: K.attn_bwd("full", qkv, *t, B=B, heads=hs, S=So, causal=False, head_dim=E // hs),
            rows if packed else None, attn_bwd_rows)

    # ------------------------------------------------------------------ whole model
    def _clip_to_device(self, video: torch.Tensor) -> torch.Tensor:
        """The clip tensor (the one large input: 925 MB of fp32 at 192 pairs) goes host -> device on a COPY STREAM of the engine:
        on the compute stream the copy would queue behind the previous step's kernels and run in front of this step's -- 20 ms
        (pinned) to 46 ms (pageable) of a 140 ms step with nothing else running (tools/bench_fed.py).  On its own stream it travels
        while the previous step computes; the compute stream waits for it by event, the allocator is told who uses the block."""
        if video.is_cuda or not torch.cuda.is_available():
            return video.to(self.dev)
        cs = getattr(self, "_copy_stream", None)
        if cs is None:
            cs = self._copy_stream = torch.cuda.Stream(device=self.dev)
        cur = torch.cuda.current_stream(self.dev)
        if torch.cuda.is_current_stream_capturing():
            return video.to(self.dev)
        with torch.cuda.stream(cs):
            d = video.to(self.dev, non_blocking=True)
        cur.wait_stream(cs)
        d.record_stream(cur)
        return d

    def _packed_to_device(self, clips, plan):
        """source clips of a resize plan -> ONE uint8 device buffer with clip b at plan["offsets"][b].  A tensor [B, T, Hs, Ws, 3] is
        that buffer already; a list is packed into a page-locked staging buffer (a ring of STAGE_SLOTS, each guarded by the event of
        its last copy, as _stage_small).  Either way ONE asynchronous copy on the engine's copy stream (_clip_to_device)."""
        if torch.is_tensor(clips):
            return self._clip_to_device(clips.contiguous().view(-1))
        total = plan["nbytes"]
        ring = getattr(self, "_clip_ring", None)
        if ring is None:
            ring = self._clip_ring = dict(i=0, slots=[None] * self.STAGE_SLOTS)
        i = ring["i"] = (ring["i"] + 1) % self.STAGE_SLOTS
        slot = ring["slots"][i]
        if slot is None or slot[0].numel() < total:
            slot = ring["slots"][i] = [torch.empty(total, dtype=torch.uint8, pin_memory=True), None]
        if slot[1] is not None:
            slot[1].synchronize()
        from .data_loader.v1_input import pack_clips
        dev = self._clip_to_device(pack_clips(clips, plan["offsets"].tolist(), slot[0])[:total])
        if not torch.cuda.is_current_stream_capturing():
            slot[1] = torch.cuda.Event()
            slot[1].record(self._copy_stream)
        return dev

    def _ragged_batch(self, data: dict):
        """the HOST half of a ragged uint8 batch (DESIGN.md 8j "v2 ragged"): data["video"] a list of B uint8 clips [T_b, Hs_b, Ws_b, 3]
        as decoded, each resized (data["resize"]: video_transform.Resize's size, absent = none) and cropped (data["crop"] [B, 2] (top,
        left) in RESIZED coordinates, absent = centre) on its own; a clip of T_b < T frames (T = data["num_frames"], default max T_b)
        is followed by the reference's zero frames behind Normalize (v2/base/base_dataset.py:116-130) -> (clips, plan of
        hip.gather_plan, B, T).  ValueError by name for a clip that is not uint8 [*, *, *, 3], a clip without frames or longer than
        T, T beyond the temporal embedding, a resized side below img, a crop outside the frame.  Nothing here touches the device."""
        a, clips = self.arch, list(data["video"])
        if not clips:
            raise ValueError("video: an empty list of clips")
        for b, c in enumerate(clips):
            if not torch.is_tensor(c) or c.dtype != torch.uint8 or c.dim() != 4 or c.shape[-1] != 3:
                raise ValueError(f"video: clip {b} of a list must be a uint8 tensor [T, Hs, Ws, 3], got "
                                 + (f"{c.dtype} {tuple(c.shape)}" if torch.is_tensor(c) else type(c).__name__))
            if c.shape[0] < 1:
                raise ValueError(f"video: clip {b} has no frames")
        B = len(clips)
        T = int(data["num_frames"]) if data.get("num_frames") is not None else max(int(c.shape[0]) for c in clips)
        for b, c in enumerate(clips):
            if int(c.shape[0]) > T:
                raise ValueError(f"video: clip {b} has {int(c.shape[0])} frames, more than the batch's num_frames of {T}")
        if T > a["num_frames"]:
            raise ValueError(f"clips of {T} frames, the temporal embedding has {a['num_frames']} rows")
        crop = data.get("crop")
        if crop is not None:
            crop = torch.as_tensor(crop).detach().to("cpu", torch.int64)
            if tuple(crop.shape) != (B, 2):
                raise ValueError(f"crop {tuple(crop.shape)}: expected [{B}, 2] (top, left)")
            crop = crop.tolist()
        plan = K.gather_plan([(int(c.shape[1]), int(c.shape[2])) for c in clips], [int(c.shape[0]) for c in clips], crop,
                             size=None if data.get("resize") is None else int(data["resize"]), img=a["image"], T=T)
        return clips, plan, B, T

    def prepare_batch(self, data: dict):
        """Host-side (plumbing): dtype/device normalisation of the reference batch dict."""
        a = self.arch
        video = data["video"]
        crop = resize = crop_cpu = plan = None
        if isinstance(video, (list, tuple)):
            # ragged uint8 wire format: the clips at the decoder's sizes and lengths in ONE packed upload; Resize, crop, / 255,
            # Normalize and the zero frames of short clips happen inside the patch gather (tvts_patch_gather_u8_ragged)
            clips, plan, B, T = self._ragged_batch(data)
            video = self._packed_to_device(clips, plan)
        elif video.dtype == torch.uint8:
            # uint8 wire format: [B, T, H0, W0, 3] frames as decoded + resized; crop / 255 / normalise
            # happen inside the patch gather.  data["crop"]: [B, 2] (top, left) of a random crop, absent = centre crop.
            if video.dim() == 4:
                video = video.unsqueeze(1)
            assert video.dim() == 5 and video.shape[-1] == 3, "uint8 video must be [B, T, H, W, 3]"
            video = self._clip_to_device(video).contiguous()
            if data.get("crop") is not None:
                crop_cpu = data["crop"].detach().to("cpu", torch.int32).contiguous()
            if data.get("resize") is not None:  # the frames are the decoder's pictures: Resize(size) happens inside the gather
                from .data_loader.transforms import resize_tables
                resize = resize_tables(video.shape[2], video.shape[3], int(data["resize"]), self.dev)
        else:
            if video.dim() == 4:
                video = video.unsqueeze(1)
            video = self._clip_to_device(video).to(torch.float32).contiguous()
        if plan is None:
            B, T = video.shape[:2]
        # the reference fails on these with an indexing / broadcasting error (temporal_embedding[:T], nn.Embedding, pos[keep_ind]); the
        # kernels would read or write past the tables instead, so the batch is checked where it enters
        if T > a["num_frames"]:
            raise ValueError(f"clips of {T} frames, the temporal embedding has {a['num_frames']} rows")
        ids = data["text"]
        ids_cpu = ids.detach().to("cpu", torch.int64)
        if ids_cpu.numel() == 0 or ids_cpu.shape[0] % B:
            raise ValueError(f"text: {tuple(ids_cpu.shape)} token rows for {B} clips (expected n_trans * B rows, clip-major)")
        if int(ids_cpu.min()) < 0 or int(ids_cpu.max()) >= a["vocab"] or ids_cpu.shape[1] > a["context"]:
            raise IndexError(f"token ids must lie in [0, {a['vocab']}) and captions within the context of {a['context']}")
        eot = ids_cpu.argmax(dim=-1)
        L = int(eot.max()) + 1
        N = ids_cpu.shape[0]
        NT = N // B
        pk = K.pack_captions(ids_cpu, a["context"]) if self.text_packed else None  # (captions stay in batch order: rows i * B + b)
        # every small index tensor of the batch is made on the HOST and travels in one asynchronous copy (_stage_small): no copy of
        # this function is ordered behind the compute stream's running step, so the host prepares batch t + 1 while step t computes
        if pk is None:
            small = {"eot_rows": (torch.arange(N) * L + eot).to(torch.int32), "eot_pos": eot.to(torch.int32),
                     "ids": ids_cpu[:, :L].to(torch.int32).contiguous()}
            # rows sorted by token id: the token-embedding gradient is then an ordered sum per id instead of a scatter of atomics
            small["tok_order"], small["tok_seg"] = K.token_sort(ids_cpu[:, :L])
        else:  # the packed descriptors instead of the rectangle's: ids [M], seq_start, the EOT rows and the two sort plans
            small = {k: pk[k] for k in ("eot_rows", "ids", "seq_start", "tok_order", "tok_seg", "pos_order", "pos_seg")}
        keep = None
        if "keep_ind" not in data:
            # device-drawn tube mask: data["mask_seed"] + the global number of the batch's first sample
            # reproduce the draw whatever the batch split; the reference draws it in the dataset worker
            # (YTTemporal_dataset.py:207-213) and ships it with the batch
            if "mask_seed" not in data:
                raise KeyError("batch dict needs 'keep_ind' or 'mask_seed' (+ optional 'sample_offset')")
            keep = K.tube_mask(int(data["mask_seed"]), int(data.get("sample_offset", 0)), B, patches_per_frame(a),
                               n_keep(a), device=self.dev)
        else:
            kc = data["keep_ind"]
            if kc.dim() != 2 or kc.shape[0] not in (1, B):
                raise ValueError(f"keep_ind {tuple(kc.shape)}: expected [B, n_keep] (or [1, n_keep] for the whole batch)")
            if kc.numel() and (int(kc.min()) < 0 or int(kc.max()) >= patches_per_frame(a)):
                raise IndexError(f"keep_ind must index the {patches_per_frame(a)} patches of a frame")
            if kc.shape[0] == 1 and B > 1:  # one tube mask for the whole batch (the downstream scripts pass arange(n)[None])
                kc = kc.expand(B, -1)
            if kc.is_cuda:
                keep = kc.to(torch.int32).contiguous()
            else:
                small["keep"] = kc.to(torch.int32).contiguous()
        n = (keep if keep is not None else small["keep"]).shape[1]
        S = 1 + T * n
        Sv = S - 1 if self.pooled_tail else S
        So = Sv + NT
        small["sort_rows"] = (torch.arange(B)[:, None] * So + Sv + torch.arange(NT)[None, :]).reshape(-1).to(torch.int32)
        small["vid_rows"] = (torch.arange(B) * S).to(torch.int32)
        if crop_cpu is not None:
            small["crop"] = crop_cpu
        if plan is not None:
            small["ga_desc"], small["ga_tables"] = torch.from_numpy(plan["desc"]), torch.from_numpy(plan["tables"])
        if "label" in data and NT != 1:
            small["labels"] = data["label"].detach().reshape(-1).to("cpu", torch.int32)
        d = self._stage_small(small)
        if keep is None:
            keep = d["keep"]
        pb = dict(video=video, crop=d.get("crop", crop), resize=resize, ids=d["ids"], tok_sort=(d["tok_order"], d["tok_seg"]),
                  eot_rows=d["eot_rows"], eot_index=(None, d["eot_pos"]) if pk is None else None, keep=keep, B=B, T=T, N=N, NT=NT, L=L,
                  n=n, S=S, sort_rows=d["sort_rows"], vid_rows=d["vid_rows"], labels=d.get("labels"))
        if pk is not None:
            pb.update(M=int(pk["ids"].numel()), seq_start=d["seq_start"], max_len=pk["max_len"], pos_sort=(d["pos_order"], d["pos_seg"]))
        if plan is not None:
            pb["gather"] = dict(desc=d["ga_desc"], tables=d["ga_tables"])
        return pb

    STAGE_SLOTS = 4

    def _stage_small(self, small: dict) -> dict:
        """{name: small host int tensor} -> {name: device tensor}: packed into ONE page-locked staging buffer (a ring of STAGE_SLOTS, each
        guarded by the event of its last copy) and moved by ONE asynchronous copy on the engine's copy stream; the compute stream
        waits for it by event.  (One pageable .to(device) per tensor is a synchronous copy queued behind the running step: the host
        would wait for the previous step to finish before it could even start preparing the next one.)"""
        offs, total = {}, 0
        for k, t in small.items():
            offs[k] = total
            total += (t.numel() * t.element_size() + 15) // 16 * 16
        total = max(total, 16)
        if not torch.cuda.is_available() or self.dev.type != "cuda":
            return {k: t.to(self.dev) for k, t in small.items()}
        ring = getattr(self, "_stage_ring", None)
        if ring is None:
            ring = self._stage_ring = dict(i=0, slots=[None] * self.STAGE_SLOTS)
        i = ring["i"] = (ring["i"] + 1) % self.STAGE_SLOTS
        slot = ring["slots"][i]
        if slot is None or slot[0].numel() < total:
            slot = ring["slots"][i] = [torch.empty(max(total, 1 << 16), dtype=torch.uint8, pin_memory=True), None]
        if slot[1] is not None:
            slot[1].synchronize()  # the copy that last read this staging buffer (STAGE_SLOTS batches ago: long done)
        host = slot[0]
        for k, t in small.items():
            nb = t.numel() * t.element_size()
            if nb:
                host[offs[k]:offs[k] + nb].view(t.dtype).copy_(t.reshape(-1))
        cs = getattr(self, "_copy_stream", None)
        if cs is None:
            cs = self._copy_stream = torch.cuda.Stream(device=self.dev)
        cur = torch.cuda.current_stream(self.dev)
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            devbuf = host[:total].to(self.dev)
        else:
            with torch.cuda.stream(cs):
                devbuf = torch.empty(total, dtype=torch.uint8, device=self.dev)
                devbuf.copy_(host[:total], non_blocking=True)
                slot[1] = torch.cuda.Event()
                slot[1].record(cs)
            cur.wait_stream(cs)
            devbuf.record_stream(cur)
        out = {}
        for k, t in small.items():
            nb = t.numel() * t.element_size()
            out[k] = devbuf[offs[k]:offs[k] + nb].view(t.dtype).view(t.shape)
        return out

    def forward(self, pb: dict, sort_head: bool = True):
        """-> (text_emb [B,E], video_emb [B,E], pred [B*NT, n_trans] | None); all fp32 workspace tensors.
        sort_head=False (the embedding pass of the micro-batched step): the same launches up to the two embeddings,
        hence their bits; the sort head is left out and pred is None."""
        a = self.arch
        self.ctx = pb
        self._tick += 1  # (workspace: a buffer whose shape changes from here on belongs to a new step, see _b)
        B, T, N, NT, L, S, E = pb["B"], pb["T"], pb["N"], pb["NT"], pb["L"], pb["S"], a["embed"]
        text_emb = self._f("mdl.text_emb", (B, E))
        text_before = self._f("mdl.text_before", (B, NT, E))
        with self._text_lane():  # (the text tower beside the ViT when self.text_side, in line otherwise)
            t = self.text_forward(pb["ids"], pb["eot_rows"], N, L, eot_index=pb.get("eot_index"),
                                  packed=pb if pb.get("seq_start") is not None else None)
            K.text_mean(t, text_emb, text_before, NT=NT, B=B)
        out, pooled = self.video_forward(pb["video"], pb["keep"], B, T, vid_rows=pb["vid_rows"])
        if pooled is None:
            video_emb = self._f("mdl.video_emb", (B, E))
            K.rows_gather(out, pb["vid_rows"], video_emb)
        else:
            video_emb = pooled
        self._text_join()
        if self.embeds_ready is not None:  # the embedding all-gather starts here and travels under the sort head's forward
            self.embeds_ready(text_emb, video_emb)
        pred = self.sort_forward(out, text_before, B, S, NT) if (NT != 1 and self.has_sort_head and sort_head) else None
        return text_emb, video_emb, pred

    class _TextLane:
        """`with` block whose launches go to the text tower's stream (forked from the current stream's position) and use the side
        scratch lane; a no-op when the text tower runs in line"""

        def __init__(self, eng):
            self.eng = eng

        def __enter__(self):
            e = self.eng
            if not e.text_side:
                return
            if e._txt_stream is None:
                e._txt_stream = torch.cuda.Stream(device=e.dev)
            cur = torch.cuda.current_stream(e.dev)
            e._txt_stream.wait_stream(cur)
            self.sc, self.ln = torch.cuda.stream(e._txt_stream), K.lane(1)
            self.sc.__enter__()
            self.ln.__enter__()
            e._txt_open = True

        def __exit__(self, *exc):
            if self.eng.text_side:
                self.ln.__exit__(*exc)
                self.sc.__exit__(*exc)

    def _text_lane(self):
        return Engine._TextLane(self)

    def _text_join(self):
        """the current stream waits for what the text lane has queued"""
        if self.text_side and getattr(self, "_txt_open", False):
            torch.cuda.current_stream(self.dev).wait_stream(self._txt_stream)
            self._txt_open = False

    def backward(self, d_text, d_video, d_pred):
        """Accumulates parameter gradients into the flat grad buffer (+=).  d_* are fp32 GPU tensors (or None)."""
        a, pb = self.arch, self.ctx
        B, T, N, NT, L, S, E = pb["B"], pb["T"], pb["N"], pb["NT"], pb["L"], pb["S"], a["embed"]
        # the text tower first: it shares nothing with the video / sort-head backward (the sort head sees DETACHED caption
        # embeddings, model_dist..B_16.py:69), and its gradient range (token embedding included) is the largest single
        # all-reduce of the step -- issued here it travels under the whole video backward instead of after it
        # ... which holds while the text tower runs IN LINE.  On its own stream (text_side) its backward finishes some 150 kernels after
        # the fork, and an all-reduce issued from that lane would sit at the head of the single collective stream until then with every
        # ViT range queued behind it: with an exchange step attached (world > 1 / range-wise optimizer) the text range is handed over
        # at the join instead, from the main stream, behind the ViT ranges.
        text_ready_at_join = False
        if d_text is not None:
            dt = self._f("mdl.dt", (N, E))
            with self._text_lane():  # beside the sort head's and the ViT's backward when self.text_side; joined at the end
                K.text_mean_bwd(d_text, dt, NT=NT, B=B)
                self.text_backward(dt, pb["ids"], pb["eot_rows"], N, L, tok_sort=pb.get("tok_sort"),
                                   packed=pb if pb.get("seq_start") is not None else None)
                if self.text_side and (self.grad_ready is not None or self.param_ready is not None):
                    text_ready_at_join = True
                else:
                    self._ready("text_")
        dout = self._b("mdl.dout", (B * S, E))
        off = 1 if self.pooled_tail else 0
        dv_cls = None if self.pooled_tail else d_video  # B models: the embedding IS the CLS row of the projected tokens
        if d_pred is not None:
            dxs = self.sort_backward(d_pred, B, S, NT)
            K.sort_assemble_bwd(dxs, dv_cls, dout, self.P.g("pred_model.type_embed").view(2, E), B=B, S=S, off=off,
                                Sv=S - off, NT=NT)
            self._ready("pred_model.")
        elif not self.pooled_tail:
            K.sort_assemble_bwd(None, dv_cls, dout, None, B=B, S=S, off=0, Sv=S, NT=NT)
        else:
            dout = None
        self.video_backward(dout, pb["keep"], B, T, d_pooled=d_video if self.pooled_tail else None)
        self._text_join()
        if text_ready_at_join:
            self._ready("text_")

    # ------------------------------------------------------------------ forward-only encoders (feature extraction, zero-shot)
    # The two passes of the forward.  There is ONE forward wiring (_ln, _lin, _st_attention_fwd, _block_fwd, _blocks_fwd,
    # _text_tower, _vit_embed, _vit_block_head, _vit_block); the training step and the encoders below both run it, and the `tag`
    # argument is all that tells them apart:
    #   tag = a name   every buffer is the named tensor tag + name of self.buf (_b), one per layer, kept for the backward; the
    #                  tensors only a backward reads are produced: LayerNorm mean / rstd, the attention log-sum-exp, the act'(x)
    #                  side output of c_fc;
    #   tag = None     every buffer is an encoder workspace (_ib) keyed by ROLE, in a namespace of its own (self._inf), reused by
    #                  every layer (peak ~ one layer) with the residual stream updated in place; the backward-only tensors are
    #                  neither allocated nor written (lse2 = None: SPACE calls at full frames take their own fused kernel).
    # Same entry points, weights, epilogue options and epsilons either way.  What the encoders add of their own: the last ViT
    # block runs its second half for the CLS rows only.  Nothing of the training step's workspace is read, written or resized by an
    # encoder call.
    # e4m3 architectures (fp8 / fp8_dgrad / fp8_wgrad): the blocks' six linear layers multiply the e4m3 weight copies of ParamStore.w8
    # in the PER-TOKEN regime -- activation rows under their own scale, from the LayerNorm in front of qkv / c_fc or from one
    # quantiser pass -- which has no state: no calibration, and on an fp8_wgrad model also after _f8_tensor_mode has come on; the
    # scale table (_f8_scale, _f8_amax, _f8_ids) and the backward's operand bookkeeping (_x8, _x8_ready, _x8_only) are neither read
    # nor written.  The e4m3 bytes and row scales are the encoder workspaces "q8.<width>" / "q8.row_scale" (_q8 with name None).
    # The last block's CLS tail multiplies the e4m3 copies of attn.proj and mlp.c_proj as well (tvts_rows_linear_fp8 over the B
    # quantised CLS rows).  The text tower is never quantised: encode_text* run what they run on a bf16 architecture.
    def _inf_check(self):
        a = self.arch
        if a.get("family") == "v1":
            raise NotImplementedError("the forward-only encoders are built for the v2 models")

    def _cls_tail_lin(self, a_c, wname, bname, res_c, out_c):
        """a residual-adding projection of the last block on the B CLS rows a_c (bf16, possibly a strided row view) -> out_c fp32:
        on the weight's e4m3 copy where the architecture has one (the rows quantised per token like every other row of the layer,
        tvts_quant_fp8_rows over the strided view), on the bf16 shadow otherwise"""
        bias = self.P.p(bname)
        if wname in self.P.w8:
            w8, ws, _ = self.P.w8[wname]
            q, rs, kw = self._q8(a_c.shape[0], a_c.shape[1], None)
            K.quantize_fp8_rows(a_c, q=q, **kw)
            K.rows_linear_fp8(q, rs, w8, ws, out_c, bias=bias, residual=res_c)
            return
        K.rows_linear(a_c, self.P.w(wname), out_c, bias=bias, residual=res_c)

    def encode_video(self, video, keep_dev, B, T, crop=None, resize=None, gather=None):
        """-> [B, E] fp32 video embeddings (an encoder workspace: the next encoder call overwrites it).  video: fp32 [B, T, 3, H, W]
        or uint8 [B, T, H0, W0, 3] on the device, or with gather = dict(desc, tables) (device copies of a hip.gather_plan) the packed
        ragged uint8 clips; keep_dev: int32 [B, n] kept patches per frame."""
        self._inf_check()
        a, f32 = self.arch, torch.float32
        W, E, h = a["width"], a["embed"], a["heads"]
        n = keep_dev.shape[1]
        S = 1 + T * n
        M = B * S
        vid_rows = self._row_starts("vid_rows", B, S)
        x, xc = self._vit_embed(video, keep_dev, B, T, vid_rows, crop, resize, None, gather=gather)
        for l in range(a["layers"] - 1):
            x, xc = self._vit_block(l, x, xc, None, B, T, n)
        # the last block for the CLS rows: the time branch and the space qkv run on every row (they make the keys and values of
        # the CLS query); the CLS query attends all S keys (MODE_CLS), everything after it runs on B rows in fp32
        pre = f"video_model.transformer.resblocks.{a['layers'] - 1}."
        qkv = self._vit_block_head(pre, x, xc, None, B, T, n)
        att = self._ib("att", (M, W))
        K.attn_fwd("cls", qkv, att, None, B=B, heads=h, S=S, T=T, n=n, head_dim=self.dh)
        if xc is not None:
            x_c = xc
        else:
            x_c = self._ib("xg", (B, W), f32)
            K.rows_move("gather", vid_rows, full_f32=x if x.dtype == f32 else None,
                        full_bf16=x if x.dtype == torch.bfloat16 else None, packed_f32=x_c)
        att_c = att.view(B, S * W)[:, :W]
        s_c = self._ib("sc", (B, W), f32)
        self._cls_tail_lin(att_c, pre + "attn.proj.weight", pre + "attn.proj.bias", x_c, s_c)
        ln_c = self._ib("lnc", (B, W))
        a8 = self._ln(s_c, pre + "ln_2", 1e-5, ln_c, None, fp8_for=pre + "mlp.c_fc.weight")
        h_c = self._ib("hc", (B, 4 * W))
        self._lin(ln_c, pre + "mlp.c_fc.weight", pre + "mlp.c_fc.bias", h_c, B, act=a["act"], a8=a8, fwd_only=True)
        xo_c = self._ib("xoc", (B, W), f32)
        self._cls_tail_lin(h_c, pre + "mlp.c_proj.weight", pre + "mlp.c_proj.bias", s_c, xo_c)
        emb = self._ib("vemb", (B, E), f32)
        if not self.pooled_tail:  # B models: ln_post, then x @ proj of the CLS rows (the embedding is the CLS row of the tokens)
            lnp = self._ib("lnc", (B, W))
            self._ln(xo_c, "video_model.ln_post", 1e-5, lnp, None)
            K.gemm_nt(lnp, self.P.wt("video_model.proj"), emb, M=B)
            return emb
        lnc = self._ib("lnpc", (B, W), f32)  # H/14: pooled = ln_post(CLS) @ proj in fp32
        self._ln(xo_c, "video_model.ln_post", 1e-5, lnc, None)
        K.gemm_small(lnc, self.P.p("video_model.proj"), emb, M=B, N=E, K=W, sa=(W, 1), sb=(E, 1))
        return emb

    def encode_text(self, ids_dev, eot_rows, N, L, eot_index=None):
        """-> [N, E] fp32 caption embeddings, the bits of text_forward (an encoder workspace).  eot_index as in text_forward."""
        self._inf_check()
        return self._text_padded(ids_dev, eot_rows, N, L, eot_index, None)[0]

    def encode_text_packed(self, ids_packed, seq_start, N, max_len):
        """encode_text over PACKED captions -> [N, E] fp32 (an encoder workspace).  ids_packed: int32 [M] on the device, every caption
        cut behind its own EOT token (rows behind it cannot reach the EOT row: causal mask); seq_start: int32 [N + 1], caption i owns
        rows seq_start[i] .. seq_start[i + 1] - 1 and is read at its last one; max_len >= the longest caption.  M = sum L_i rows go
        through the LayerNorms and GEMMs instead of N * max L_i; pack captions of similar length next to each other.
        The ids must be validated by the caller (TVTSv2Base.encode_text does): the embedding kernel leaves a row whose token id is
        outside the vocabulary, or whose position is past the context, unwritten, and stale workspace contents would run through the tower."""
        self._inf_check()
        ht = self.arch["text_heads"]
        if self.dh_text != 64:
            raise NotImplementedError("the packed attention kernels are built for head dim 64")
        eot_rows = self._ib("eot_rows", (N,), torch.int32)
        torch.sub(seq_start[1:], 1, out=eot_rows)
        return self._text_tower(
            lambda x: K.text_embed_packed(ids_packed, seq_start, self.P.p("text_token_embedding.weight"),
                                          self.P.p("text_positional_embedding"), x, N=N),
            lambda qkv, att, lse: K.attn_fwd_packed(qkv, seq_start, att, N=N, heads=ht, max_len=max_len),
            lambda qkv, att, lse: K.attn_fwd_packed(qkv, seq_start, att, N=N, heads=ht, max_len=max_len, last_only=True),
            eot_rows, N, ids_packed.numel())


class LossHead:
    """sim_matrix + NormSoftmaxLoss (+ sorting CE) forward AND backward on the GPU, fp32.

    model/model_dist_TVTSv2_ViT_B_16.py:119-127, model/loss.py:13-25, trainer/trainer.py:484-496."""

    def __init__(self, device, temperature=0.05):
        self.dev, self.temp = device, temperature
        self.buf: Dict[str, torch.Tensor] = {}

    def _f(self, name, shape, zero=False):
        t = self.buf.get(name)
        shape = tuple(int(s) for s in shape)
        if t is None or tuple(t.shape) != shape:
            t = self.buf[name] = torch.zeros(shape, dtype=torch.float32, device=self.dev)
        elif zero:
            K.zero_(t)
        return t

    def sim(self, a, b, eps=1e-8):
        G, E = a.shape
        an, bn = self._f("an", (G, E)), self._f("bn", (b.shape[0], E))
        ai, bi = self._f("ai", (G,)), self._f("bi", (b.shape[0],))
        K.l2norm_rows(a, an, ai, eps)
        K.l2norm_rows(b, bn, bi, eps)
        return an, bn, ai, bi

    def contrastive(self, video_all, text_all, need_grad=True):
        """-> (loss1 scalar tensor, d_video_all, d_text_all).  Rows of the similarity are videos (trainer.py:484)."""
        G, E = video_all.shape
        vn, tn, vi, ti = self.sim(video_all, text_all)
        x = self._f("x", (G, G))
        K.gemm_small(vn, tn, x, M=G, N=G, K=E, sa=(E, 1), sb=(1, E), alpha=1.0 / self.temp)
        lse = self._f("lse", (2 * G,))
        loss = self._f("loss1", (1,), zero=True)
        dx = self._f("dx", (G, G)) if need_grad else None
        K.infonce(x, lse, dx, loss)
        if not need_grad:
            return loss, None, None
        dvn, dtn = self._f("dvn", (G, E)), self._f("dtn", (G, E))
        K.gemm_small(dx, tn, dvn, M=G, N=E, K=G, sa=(G, 1), sb=(E, 1), alpha=1.0 / self.temp)
        K.gemm_small(dx, vn, dtn, M=G, N=E, K=G, sa=(1, G), sb=(E, 1), alpha=1.0 / self.temp)
        dv, dt = self._f("dv", (G, E)), self._f("dt", (G, E))
        K.l2norm_rows_bwd(dvn, vn, vi, dv)
        K.l2norm_rows_bwd(dtn, tn, ti, dt)
        return loss, dv, dt

    def sorting(self, pred, labels_i32, need_grad=True, scale=2.0, add=False):
        """2 * CrossEntropy (trainer.py:487-492) -> (loss2, dpred).  scale / add (the micro-batched step): the kernel means over the
        rows it is given, so chunk k of n passes scale 2 / n, and add=True keeps the value the earlier chunks left in loss2 -- the
        kernel adds to it, the n shares sum to the full batch's 2 * CE in chunk order."""
        loss = self._f("loss2", (1,), zero=not add)
        dp = self._f("dpred", pred.shape) if need_grad else None
        K.cross_entropy(pred, labels_i32, scale, dp, loss)
        return loss, dp
