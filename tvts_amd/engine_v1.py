"""Step engine of the v1 TVTS model over the same HIP kernels as the v2 engine.

What differs from TVTSv2 (reference paths under v1/):
  video tower   Conv3d TUBELET patch embedding (2 frames x 16 x 16 -> one token) as gather + MFMA GEMM over the kept patches
                only, a tube mask PER TUBE, JOINT space-time attention over all kept tokens of the clip (one FULL attention
                site per block instead of the divided time / space pair), pre-LN blocks with erf-GELU, final norm on every
                token, vid_proj on the CLS token           model/video_encoder.py:78-217, model/model_dist_TVTS.py:143-147
  text tower    Hugging Face DistilBERT: learned word + position embeddings -> LayerNorm, POST-LN blocks (separate q / k / v /
                out projections, erf-GELU FFN, eps 1e-12), padded keys masked, [CLS] row -> ReLU -> Linear
                                                            model/model_dist_TVTS.py:34,65-68,131-141
  sort head     the same SortTransformer, fed the un-projected normed ViT tokens (width 768) and the [CLS] text rows
                                                            model/model_dist_TVTS.py:99-116
Dropout: the reference puts the text tower in training mode (model_dist_TVTS.py:33-34 ``self.text_model.train()``), so every
pretraining step runs DistilBERT's dropouts (transformers modeling_distilbert: ``Embeddings.dropout`` behind the embedding
LayerNorm, ``attention_dropout`` on the softmax probabilities, ``FFN.dropout`` behind lin2; all p = 0.1, config defaults).  Built
here with a COUNTER-BASED generator (splitmix64 of seed + site + element index, tvts_attn_*_len_drop / tvts_dropout_rows): the
attention mask lives inside the attention kernels (probabilities are never materialised), the backward regenerates every mask from
(seed, site), the seed sits in device memory and is advanced by a device op at the start of every training forward (graph replays
draw new masks).  ``engine.training = False`` (the module's eval mode: validation, feature extraction) or
``arch["text_dropout"] = 0`` switch it off.
"""
from __future__ import annotations

import torch

from . import hip as K
from .engine import Engine, ParamStore, _SORT_NAMES

_VIT_NAMES = dict(ln1="norm1", qkv_w="attn.qkv.weight", qkv_b="attn.qkv.bias", o_w="attn.proj.weight", o_b="attn.proj.bias",
                  ln2="norm2", fc_w="mlp.fc1.weight", fc_b="mlp.fc1.bias", pj_w="mlp.fc2.weight", pj_b="mlp.fc2.bias")


class EngineV1(Engine):
    def __init__(self, store: ParamStore):
        super().__init__(store)
        assert self.arch.get("family") == "v1"
        if self.dh_text != 64:
            raise NotImplementedError("the masked FULL attention kernels are used at head dim 64 here")
        self.training = True                                   # the nn.Module wrapper mirrors its own .training flag here
        self.text_drop_p = float(self.arch.get("text_dropout", 0.1))
        # seed of the step's dropout masks (int64 device scalar = the bits of an unsigned 64-bit counter)
        # every data-parallel rank draws its own masks, as the reference's ranks do (each seeds its own generator): the rank is mixed
        # into the seed with an odd 64-bit constant.  The seed is trainer state: Trainer_TVTS saves it with the checkpoint.
        from .dist import world
        self._drop_rank = world()[1]  # the rank whose offset the seed carries (adopt_rank: a process group created afterwards)
        seed = (int(self.arch.get("dropout_seed", 0x1234ABCD)) + self._drop_rank * self.DROP_RANK_STRIDE) & ((1 << 64) - 1)
        self.drop_seed = torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64, device=self.dev)
        self._drop_active = 0.0

    DROP_STEP_STRIDE = 0x51ED270B7F4A7C15  # added to the seed (mod 2^64) once per training forward
    DROP_RANK_STRIDE = 0x9E3779B97F4A7C15  # ... and once per rank below this one

    @classmethod
    def _rank_offset(cls, rank):
        return (rank * cls.DROP_RANK_STRIDE) & ((1 << 64) - 1)

    def drop_seed_base(self) -> int:
        """the rank-independent part of the seed (configured seed + step advances, unsigned 64-bit): what a checkpoint stores --
        rank 0 writes the file, every rank reads it"""
        return ((int(self.drop_seed.item()) & ((1 << 64) - 1)) - self._rank_offset(self._drop_rank)) & ((1 << 64) - 1)

    def set_drop_seed_base(self, base: int):
        """resume: this rank's seed = stored base + this rank's offset (mod 2^64), so that every rank continues ITS OWN mask
        sequence -- loading rank 0's seed verbatim would give all ranks the same masks"""
        from .dist import world
        self._drop_rank = world()[1]
        seed = ((int(base) & ((1 << 64) - 1)) + self._rank_offset(self._drop_rank)) & ((1 << 64) - 1)
        self.drop_seed.fill_(seed - (1 << 64) if seed >= (1 << 63) else seed)

    def adopt_rank(self):
        """The seed carries the offset of the rank this process had when the engine was built.  A process group that was created
        AFTERWARDS gives the process another rank: move the seed to that rank's sequence (same base), or every rank would draw
        rank 0's masks.  Nothing happens, and nothing is read back, when the rank is the one the seed already carries."""
        from .dist import world
        if world()[1] != self._drop_rank:
            self.set_drop_seed_base(self.drop_seed_base())

    def _advance_drop_seed(self):
        """new masks for this step (a device op: a captured graph advances the seed on every replay)"""
        self._drop_active = self.text_drop_p if self.training else 0.0
        if self._drop_active > 0.0:
            self.drop_seed.add_(self.DROP_STEP_STRIDE)

    # ------------------------------------------------------------------ DistilBERT text tower
    # One wiring for both passes, like the v2 towers (Engine._w): with a `tag` the buffers are the step's named tensors, which the
    # backward reads; with tag None they are encoder workspaces, no log-sum-exp and no pre-activation is written, and there is NO
    # dropout whatever _drop_active says.
    # arch["text_unpadded"] (DESIGN.md 8b "v1"): the same wiring over M = sum(len_i) rows, captions in batch order.  `pk` is the batch's
    # device descriptor (seq_start, max_len; hip.pack_captions(lens=...)); with it the sequence-aware calls -- embedding, attention,
    # dropout, embedding backward, the [CLS] row starts -- are the packed entry points, L is the PADDED step's L (the longest caption:
    # the counter rule of the dropout masks) and every GEMM, LayerNorm and cast is the same call with M rows.
    def _txt_drop(self, x, pk, N, L, **kw):
        if pk is None:
            K.dropout_rows(x, **kw)
        else:
            K.dropout_rows_packed(x, pk["seq_start"], N=N, L_pad=L, **kw)

    def _pln_fwd(self, pre, x, xb, x_out, xb_out, tag, M, N, L, kv_len, layer=0, rows=None, pk=None):
        """one POST-LN DistilBERT block over N captions of L rows: x (fp32) / xb (bf16 copy) -> x_out / xb_out.
        rows (forward-only): the [CLS] row of every caption, for a last block whose output is read there only -- keys / values
        from every row, one query per caption (tvts_attn_fwd_first), everything behind the attention on N rows: x_out is [N, Wt]."""
        a, P, w, f32 = self.arch, self.P, self._w, torch.float32
        dp = self._drop_active if tag else 0.0
        Wt, h, Ff = a["text_width"], a["text_heads"], a["text_ffn"]
        R = M if rows is None else N
        qkv = w(tag, ".qkv", "qkv", (M, 3 * Wt))
        for i, lin in enumerate(("q_lin", "k_lin", "v_lin")):  # three projections into the packed [M, 3 Wt] buffer
            w_, b_ = P.w(pre + f"attention.{lin}.weight"), P.p(pre + f"attention.{lin}.bias")
            if rows is not None and i == 0 and pk is not None:  # ... of packed captions: no row stride, the N rows are moved
                xq, q_r = self._ib("xq_r", (N, Wt)), self._ib("q_r", (N, Wt))
                K.rows_move("gather", rows, full_bf16=xb, packed_bf16=xq)
                K.gemm_nt(xq, w_, q_r, M=N, bias=b_)
                K.rows_move("scatter", rows, full_bf16=qkv[:, :Wt], packed_bf16=q_r)
            elif rows is not None and i == 0:  # the one query of every caption: its [CLS] row (row stride L of the operand and of qkv)
                K.gemm_nt(xb.view(N, L * Wt)[:, :Wt], w_, qkv.view(N, L * 3 * Wt)[:, :Wt], M=N, bias=b_)
            else:
                K.gemm_nt(xb, w_, qkv[:, i * Wt:(i + 1) * Wt], M=M, bias=b_)
        att, lse = w(tag, ".att", "att", (M, Wt)), (self._f(tag + ".lse", (M, h)) if tag else None)
        res = x
        if rows is not None:
            assert tag is None, "the backward of the DistilBERT block is dense"
            if pk is not None:
                K.attn_fwd_packed_first(qkv, pk["seq_start"], att, N=N, heads=h, max_len=pk["max_len"])
            else:
                K.attn_fwd_first(qkv, kv_len, att, None, B=N, heads=h, S=L, head_dim=self.dh_text)
            att_r, res = self._ib("att_r", (N, Wt)), self._ib("x_r", (N, Wt), f32)
            K.rows_move("gather", rows, full_bf16=att, packed_bf16=att_r)
            K.rows_move("gather", rows, full_f32=x, packed_f32=res)
            att = att_r
        elif pk is not None:  # (p = 0: the kernels without generator work)
            K.attn_fwd_packed_bidir(qkv, pk["seq_start"], att, lse, N=N, heads=h, max_len=pk["max_len"], L_pad=L, p=dp,
                                    seed=self.drop_seed, site=1 + 2 * layer)
        elif dp > 0.0:  # weights = dropout(softmax(scores)) inside the kernel
            K.attn_fwd_len_drop(qkv, kv_len, att, lse, B=N, heads=h, S=L, p=dp, seed=self.drop_seed, site=1 + 2 * layer, head_dim=self.dh_text)
        else:
            K.attn_fwd_len(qkv, kv_len, att, lse, B=N, heads=h, S=L, head_dim=self.dh_text)
        pre1 = w(tag, ".pre1", "s", (R, Wt), f32)
        self._lin(att, pre + "attention.out_lin.weight", pre + "attention.out_lin.bias", pre1, R, residual=res)
        x1, x1b = w(tag, ".x1", "x1", (R, Wt), f32), w(tag, ".x1b", "lnc", (R, Wt))
        self._ln(pre1, pre + "sa_layer_norm", 1e-12, x1, tag and tag + ".ln_sa")
        K.cast_f32_bf16(x1, x1b)
        hpre, hact = (self._b(tag + ".h", (R, Ff)) if tag else None), w(tag, ".a", "h", (R, Ff))
        self._lin(x1b, pre + "ffn.lin1.weight", pre + "ffn.lin1.bias", hact, R, act="gelu", preact=hpre)
        pre2 = w(tag, ".pre2", "s", (R, Wt), f32)  # (forward-only pre1 is dead here: x1 carries the residual)
        if dp > 0.0:  # pre2 = dropout(lin2(.)) + x1
            y2 = self._f("txt.s.y2", (R, Wt))
            self._lin(hact, pre + "ffn.lin2.weight", pre + "ffn.lin2.bias", y2, R)
            self._txt_drop(y2, pk, N, L, p=dp, seed=self.drop_seed, site=2 + 2 * layer, residual=x1, out=pre2)
        else:
            self._lin(hact, pre + "ffn.lin2.weight", pre + "ffn.lin2.bias", pre2, R, residual=x1)
        self._ln(pre2, pre + "output_layer_norm", 1e-12, x_out, tag and tag + ".ln_out")
        if xb_out is not None:
            K.cast_f32_bf16(x_out, xb_out)

    def _pln_bwd(self, pre, xb_in, dx_out, dx_in, tag, M, N, L, kv_len, layer=0, pk=None):
        """dx_out: fp32 grad wrt the block output; writes the fp32 grad wrt the block input into dx_in."""
        a, P, B_ = self.arch, self.P, self.buf
        dp = self._drop_active
        Wt, h, Ff = a["text_width"], a["text_heads"], a["text_ffn"]
        # output_layer_norm: y = LN(pre2), pre2 = lin2(gelu(lin1(x1))) + x1
        dpre2, dpre2b = self._f("txt.s.dpre2", (M, Wt)), self._b("txt.s.dpre2b", (M, Wt))
        self._ln_bwd(dx_out, B_[tag + ".pre2"], pre + "output_layer_norm", tag + ".ln_out", dpre2, dx_bf16=dpre2b)
        dh = self._b("txt.s.dh", (M, Ff))
        dy2b = dpre2b
        if dp > 0.0:  # gradient of lin2's output: the forward's mask again (the residual path keeps the unmasked dpre2)
            dy2b = self._b("txt.s.dy2b", (M, Wt))
            self._txt_drop(dpre2, pk, N, L, p=dp, seed=self.drop_seed, site=2 + 2 * layer, out_bf16=dy2b)
        self._lin_bwd(dy2b, B_[tag + ".a"], pre + "ffn.lin2.weight", pre + "ffn.lin2.bias", dh, M, gate_h=B_[tag + ".h"], gate_act="gelu")
        dx1 = self._f("txt.s.dx1", (M, Wt))  # = dpre2 (residual) + lin1 dgrad, fused as the GEMM's fp32 residual epilogue
        self._lin_bwd(dh, B_[tag + ".x1b"], pre + "ffn.lin1.weight", pre + "ffn.lin1.bias", dx1, M, residual=dpre2)
        # sa_layer_norm: x1 = LN(pre1), pre1 = out_lin(att) + x
        dpre1, dpre1b = self._f("txt.s.dpre1", (M, Wt)), self._b("txt.s.dpre1b", (M, Wt))
        self._ln_bwd(dx1, B_[tag + ".pre1"], pre + "sa_layer_norm", tag + ".ln_sa", dpre1, dx_bf16=dpre1b)
        datt = self._b("txt.s.datt", (M, Wt))
        self._lin_bwd(dpre1b, B_[tag + ".att"], pre + "attention.out_lin.weight", pre + "attention.out_lin.bias", datt, M)
        dqkv, delta = self._b("txt.s.dqkv", (M, 3 * Wt)), self._f("txt.s.delta", (M, h))
        if pk is not None:  # (every row of every caption is written in all three thirds: no zeroing)
            K.attn_bwd_packed_bidir(B_[tag + ".qkv"], pk["seq_start"], datt, B_[tag + ".att"], B_[tag + ".lse"], delta, dqkv, N=N, heads=h,
                                    max_len=pk["max_len"], L_pad=L, p=dp, seed=self.drop_seed, site=1 + 2 * layer)
        elif dp > 0.0:
            K.attn_bwd_len_drop(B_[tag + ".qkv"], kv_len, datt, B_[tag + ".att"], B_[tag + ".lse"], delta, dqkv, B=N, heads=h, S=L,
                                p=dp, seed=self.drop_seed, site=1 + 2 * layer, head_dim=self.dh_text)
        else:
            K.attn_bwd_len(B_[tag + ".qkv"], kv_len, datt, B_[tag + ".att"], B_[tag + ".lse"], delta, dqkv, B=N, heads=h, S=L,
                           head_dim=self.dh_text)
        # dx = dpre1 (residual) + dq Wq + dk Wk + dv Wv: a chain of fp32-residual epilogues over two ping-pong buffers
        acc, tmp = dpre1, self._f("txt.s.dacc", (M, Wt))
        for i, lin in enumerate(("q_lin", "k_lin", "v_lin")):
            dst = dx_in if i == 2 else (tmp if acc is dpre1 else dpre1)
            self._lin_bwd(dqkv[:, i * Wt:(i + 1) * Wt], xb_in, pre + f"attention.{lin}.weight", pre + f"attention.{lin}.bias", dst, M,
                          residual=acc)
            acc = dst

    def _text_tower_v1(self, ids, kv_len, cls_rows, N, L, tag, pk=None):
        """DistilBERT over N right-padded captions of L rows -> (before [N, Wt] fp32 = the last hidden state at [CLS],
        [N, E] = txt_proj(relu(before))).  tag "txt": the training step -- every block dense, every stream kept; None: forward-only
        -- one stream x / xb updated in place, the last block for the [CLS] rows.
        pk: the descriptor of PACKED captions -- ids is then int32 [M], cls_rows = seq_start[:-1], no buffer carries a padding row."""
        a, P, w, f32 = self.arch, self.P, self._w, torch.float32
        Wt, M, E, nl = a["text_width"], (N * L if pk is None else pk["M"]), a["embed"], a["text_layers"]
        dp = self._drop_active if tag else 0.0
        emb = w(tag, ".emb", "s", (M, Wt), f32)
        if pk is not None:
            K.text_embed_packed(ids, pk["seq_start"], P.p("text_model.embeddings.word_embeddings.weight"),
                                P.p("text_model.embeddings.position_embeddings.weight"), emb, N=N)
        else:
            K.text_embed(ids, P.p("text_model.embeddings.word_embeddings.weight"),
                         P.p("text_model.embeddings.position_embeddings.weight"), emb, N=N, L=L)
        x, xb = w(tag, ".x0", "x", (M, Wt), f32), w(tag, ".x0b", "ln", (M, Wt))
        if dp > 0.0:  # Embeddings: dropout(LayerNorm(word + position))
            xln = self._f(tag + ".xln", (M, Wt))
            self._ln(emb, "text_model.embeddings.LayerNorm", 1e-12, xln, tag + ".ln_emb")
            self._txt_drop(xln, pk, N, L, p=dp, seed=self.drop_seed, site=0, out=x, out_bf16=xb)
        else:
            self._ln(emb, "text_model.embeddings.LayerNorm", 1e-12, x, tag and tag + ".ln_emb")
            K.cast_f32_bf16(x, xb)
        packed = tag is None  # forward-only the last block runs for the rows the model reads; the step's backward is dense
        for l in range(nl - packed):
            xo, xbo = w(tag, f".x{l + 1}", "x", (M, Wt), f32), w(tag, f".x{l + 1}b", "ln", (M, Wt))
            self._pln_fwd(f"text_model.transformer.layer.{l}.", x, xb, xo, xbo, tag and f"{tag}{l}", M, N, L, kv_len, layer=l, pk=pk)
            x, xb = xo, xbo
        before = w(tag, ".before", "tbefore", (N, Wt), f32)
        if packed:
            self._pln_fwd(f"text_model.transformer.layer.{nl - 1}.", x, xb, before, None, None, M, N, L, kv_len, layer=nl - 1, rows=cls_rows,
                          pk=pk)
        else:
            K.rows_gather(x, cls_rows, before)
        act = w(tag, ".relu", "trelu", (N, Wt), f32)
        K.relu(before, act)
        t = w(tag, ".t", "temb", (N, E), f32)
        self._head_lin(act, "txt_proj.1.weight", "txt_proj.1.bias", t, N)
        return before, t

    def text_forward_v1(self, ids, kv_len, cls_rows, N, L, pk=None):
        """the training step's text tower (new dropout masks per call in training mode) -> (text_before, text_emb) as _text_tower_v1"""
        self._advance_drop_seed()
        return self._text_tower_v1(ids, kv_len, cls_rows, N, L, "txt", pk=pk)

    def text_backward_v1(self, dt, ids, kv_len, cls_rows, N, L, tok_sort=None, pk=None):
        a, P, B_ = self.arch, self.P, self.buf
        Wt, M = a["text_width"], (N * L if pk is None else pk["M"])
        dact = self._f("txt.dact", (N, Wt))
        self._head_lin_bwd(dt, B_["txt.relu"], "txt_proj.1.weight", "txt_proj.1.bias", dact, N)
        dbefore = self._f("txt.dbefore", (N, Wt))
        K.relu(B_["txt.before"], dbefore, dy=dact)
        dx = self._f("txt.dxA", (M, Wt), zero=True)
        K.rows_gather(dbefore, cls_rows, dx, scatter_add=True)  # only the [CLS] rows of the last hidden state are consumed
        for l in reversed(range(a["text_layers"])):
            dxi = self._f("txt.dx" + self._ab(a["text_layers"], l), (M, Wt))
            self._pln_bwd(f"text_model.transformer.layer.{l}.", B_[f"txt.x{l}b"], dx, dxi, f"txt{l}", M, N, L, kv_len, layer=l, pk=pk)
            dx = dxi
        if self._drop_active > 0.0:  # through the embedding dropout
            ddrop = self._f("txt.s.ddrop", (M, Wt))
            self._txt_drop(dx, pk, N, L, p=self._drop_active, seed=self.drop_seed, site=0, out=ddrop)
            dx = ddrop
        demb = self._f("txt.demb", (M, Wt))
        self._ln_bwd(dx, B_["txt.emb"], "text_model.embeddings.LayerNorm", "txt.ln_emb", demb)
        if pk is not None:
            K.text_embed_bwd_packed(demb, ids, pk["seq_start"], P.g("text_model.embeddings.word_embeddings.weight"),
                                    P.g("text_model.embeddings.position_embeddings.weight"), N=N, tok_sort=tok_sort, pos_sort=pk["pos_sort"])
        else:
            K.text_embed_bwd(demb, ids, P.g("text_model.embeddings.word_embeddings.weight"),
                             P.g("text_model.embeddings.position_embeddings.weight"), N=N, L=L, tok_sort=tok_sort)

    # ------------------------------------------------------------------ tubelet ViT with joint attention
    def _vit_embed_v1(self, video, keep, B, tubes, tag, crop=None, channel_major=False, mix=None, aug=None, view=None):
        """tubelet gather over the kept patches (fp32 clips, channel-major ones, or uint8 frames with their crop) -> patch GEMM ->
        token assembly: the tokens [B * S, W] fp32 in front of the first block.  mix: the device table of hip.mix_table() -- Mixup /
        CutMix applied inside the gather (channel-major fp32 clips and uint8 frames: the layouts the fine-tuning step takes).
        aug: the device table of hip.aug_table() for B samples -- random-resized crop, flip and random erasing inside the gather, uint8
        source frames [Bs, T, H0, W0, 3] only (every sample names its source clip; crop is not used), the mix applied behind it.
        view: the device table of hip.view_table() for B samples -- the test views of ssv2.py:132-164 (a strided run of frames of a source
        clip, cropped at an offset) formed inside the gather, uint8 source clips [Bs, Tsrc, H0, W0, 3] only; no crop, mix or aug with it"""
        a, P, w = self.arch, self.P, self._w
        W, p, tb, n = a["width"], a["patch"], a["tubelet"], keep.shape[2]
        M, Mp = B * (1 + tubes * n), B * tubes * n
        cols = w(tag, ".im2col", "im2col", (Mp, P.conv_k))
        if view is not None:
            if video.dtype != torch.uint8 or crop is not None or mix is not None or aug is not None:
                raise ValueError("a view table needs uint8 source clips [Bs, Tsrc, H0, W0, 3] and takes no crop, mix or aug beside it")
            K.patch_gather_tube_u8_view(video, keep, cols, view, B=B, tubes=tubes, tubelet=tb, n=n, img=a["image"], patch=p)
        elif aug is not None:
            if video.dtype != torch.uint8:
                raise ValueError("an augmentation table needs uint8 frames [Bs, T, H0, W0, 3] (fp32 clips are augmented by their producer)")
            K.patch_gather_tube_u8_aug(video, keep, cols, aug, mix, B=B, tubes=tubes, tubelet=tb, n=n, img=a["image"], patch=p)
        elif mix is not None:
            if video.dtype == torch.uint8:
                K.patch_gather_tube_u8_mix(video, keep, cols, mix, B=B, tubes=tubes, tubelet=tb, n=n, img=a["image"], patch=p, crop=crop)
            elif channel_major:
                K.patch_gather_tube_mix(video, keep, cols, mix, B=B, tubes=tubes, tubelet=tb, n=n, img=a["image"], patch=p)
            else:
                raise ValueError("a mix table needs channel-major fp32 clips [B, 3, T, H, W] or uint8 frames (no kernel for [B, T, 3, H, W])")
        elif video.dtype == torch.uint8:
            K.patch_gather_tube_u8(video, keep, cols, B=B, tubes=tubes, tubelet=tb, n=n, img=a["image"], patch=p, crop=crop)
        else:
            K.patch_gather_tube(video, keep, cols, B=B, tubes=tubes, tubelet=tb, n=n, img=a["image"], patch=p,
                                channel_major=channel_major)
        pe = w(tag, ".patch", "patch", (Mp, W), torch.float32)
        K.gemm_nt(cols, P.w_conv(), pe, M=Mp, bias=P.p("video_model.patch_embed.proj.bias"))
        tok = w(tag, ".x0", "x", (M, W), torch.float32)
        K.vit_assemble(pe, P.p("video_model.cls_token").view(W), P.p("video_model.pos_embed").view(-1, W),
                       P.p("video_model.temporal_embed").view(-1, W), keep, tok, B=B, T=tubes, n=n)
        return tok

    def video_forward_v1(self, video, keep, B, tubes, cls_rows, crop=None, resize=None):
        """-> (tokens [B*S, W] fp32 after the final norm, video_emb [B, E]).  video: fp32 [B, T, 3, img, img]; uint8 [B, T, H0, W0, 3]
        with crop (int32 [B, 2] on the device, None = centre); or, with resize (the device plan of prepare_batch: desc, tables,
        tmp_rows), the packed uint8 source clips -- Pillow's Resize and the crop run first (tvts_resize_crop_u8) into a workspace of
        [B, T, img, img, 3], which the uint8 gather then reads whole (its centre crop of an img x img frame is the identity)."""
        a = self.arch
        W, E, hv = a["width"], a["embed"], a["heads"]
        S = 1 + tubes * keep.shape[2]
        if resize is not None:
            T, img = tubes * a["tubelet"], a["image"]
            frames = self._b("vit.u8frames", (B, T, img, img, 3), torch.uint8)
            tmp = self._b("vit.u8rows", (B * T * resize["tmp_rows"] * img * 3,), torch.uint8)
            K.resize_crop_u8(video, resize["desc"], resize["tables"], tmp, frames, B=B, T=T, img=img, tmp_rows=resize["tmp_rows"])
            video, crop = frames, None
        tok = self._vit_embed_v1(video, keep, B, tubes, "vit", crop)
        x = self._blocks_fwd("video_model.blocks.", _VIT_NAMES, tok, "vit", a["layers"], hv, "gelu", 1e-6,
                             lambda qkv, att, lse: K.attn_fwd("full", qkv, att, lse, B=B, heads=hv, S=S, causal=False, head_dim=W // hv),
                             recompute=self.recompute)
        out = self._f("vit.out", (B * S, W))
        self._ln(x, "video_model.norm", 1e-6, out, "vit.norm")
        cls = self._f("vit.cls", (B, W))
        K.rows_gather(out, cls_rows, cls)
        emb = self._f("mdl.video_emb", (B, E))
        self._head_lin(cls, "vid_proj.0.weight", "vid_proj.0.bias", emb, B)
        return out, emb

    def video_backward_v1(self, dout_b, keep, B, tubes):
        """dout_b: bf16 [B*S, W] grad of the normed tokens (sort head + the CLS rows' share from vid_proj)"""
        a, P, B_ = self.arch, self.P, self.buf
        W = a["width"]
        n = keep.shape[2]
        S = 1 + tubes * n
        M, Mp = B * S, B * tubes * n
        dx, dxb = self._f("vit.dxA", (M, W)), self._b("vit.dxbA", (M, W))
        self._ln_bwd(dout_b, B_[f"vit.x{a['layers']}"], "video_model.norm", "vit.norm", dx, dx_bf16=dxb)
        hv = a["heads"]
        self.recompute_count = 0
        dx = self._blocks_bwd("video_model.blocks.", _VIT_NAMES, "vit", a["layers"], dx, dxb, hv, "gelu",
                              lambda qkv, *t: K.attn_bwd("full", qkv, *t, B=B, heads=hv, S=S, causal=False, head_dim=W // hv),
                              after=lambda l: self._ready(f"video_model.blocks.{l}."),
                              redo=(1e-6, lambda qkv, att, lse: K.attn_fwd("full", qkv, att, lse, B=B, heads=hv, S=S, causal=False,
                                                                           head_dim=W // hv)))
        dpatch = self._b("vit.dpatch", (Mp, W))
        K.vit_assemble_bwd(dx, keep, dpatch, P.g("video_model.cls_token").view(W), P.g("video_model.pos_embed").view(-1, W),
                           P.g("video_model.temporal_embed").view(-1, W), B=B, T=tubes, n=n)
        K.gemm_tn(dpatch, B_["vit.im2col"], P.g2d("video_model.patch_embed.proj.weight"), M=Mp, accumulate=True,
                  colsum=P.g("video_model.patch_embed.proj.bias"))
        self._ready("video_model.cls_token", "video_model.pos_embed", "video_model.temporal_embed", "video_model.patch_embed.")
        self._ready("video_model.norm.")

    # ------------------------------------------------------------------ action-recognition fine-tuning (v1/downstream)
    # The downstream class with num_classes > 0 as run_class_finetuning.py trains it: every patch kept, timm DropPath on both
    # branches of every block (video_encoder.py:65,71-72,138), `norm` at the CLS rows, `head`.  The blocks are the training step's
    # own wiring (_blocks_fwd / _blocks_bwd) with its drop_path hook; the last block runs dense.
    # Seed rule: every finetune_forward advances drop_seed once, by a device op (DROP_STEP_STRIDE, per-rank offsets as for the text
    # dropout), then draws the step's table from it -- branch s of block l is site FT_SITE_BASE + 2 l (+ 1).  The backward re-reads
    # the table the forward left.  The forward-only encoders never touch the seed.
    FT_SITE_BASE = 1 << 20   # clear of the text tower's dropout sites (0 .. 2 * text_layers)
    drop_path_rate = 0.0     # the downstream class sets its constructor argument here
    drop_path_override = None  # fp32 device [2 * depth, B]: used instead of the drawn table (replaying a reference run's masks)

    def _ft_table(self, B):
        """the step's scale table [2 * depth, B] (None: no stochastic depth in this step)"""
        depth = self.arch["layers"]
        if self.drop_path_override is not None:
            t = self.drop_path_override
            assert t.dtype == torch.float32 and tuple(t.shape) == (2 * depth, B) and t.is_cuda and t.is_contiguous()
            return t
        rate = float(self.drop_path_rate)
        if rate <= 0.0:
            return None
        ent = self.buf.get(("ft.dp_rates", rate))
        if ent is None:  # video_encoder.py:138, each block's rate for both of its branches
            dpr = [torch.linspace(0, rate, depth)[l].item() for l in range(depth)]
            ent = self.buf[("ft.dp_rates", rate)] = torch.tensor([r for r in dpr for _ in (0, 1)], dtype=torch.float32, device=self.dev)
        table = self._f("ft.dp_table", (2 * depth, B))
        K.drop_path_table(self.drop_seed, ent, table, site_base=self.FT_SITE_BASE)
        return table

    def finetune_forward(self, video, B, tubes, channel_major=True, crop=None, mix=None, aug=None):
        """-> logits [B, C] fp32 (a named tensor of the step).  video on the device: fp32 [B, 3, T, H, W] (channel_major, the
        downstream layout), fp32 [B, T, 3, H, W], or uint8 [B, T, H0, W0, 3] with crop int32 [B, 2] (None: centre).  mix: the
        device table of hip.mix_table(), Mixup / CutMix inside the gather (engine_for_finetuning.py:58-59).  aug: the device table of
        hip.aug_table() for B samples over uint8 source frames [Bs, T, H0, W0, 3] (ssv2.py:186-227 inside the gather)."""
        a = self.arch
        W, hv, C, depth = a["width"], a["heads"], a["head_classes"], a["layers"]
        ppf = (a["image"] // a["patch"]) ** 2
        S = 1 + tubes * ppf
        self._tick += 1
        self.drop_seed.add_(self.DROP_STEP_STRIDE)
        table = self._ft_table(B)
        keep = self.buf.get(("ft.keep", B, tubes))
        if keep is None:
            keep = self.buf[("ft.keep", B, tubes)] = torch.arange(ppf, dtype=torch.int32, device=self.dev).repeat(B, tubes, 1).contiguous()
            self.buf[("ft.cls_rows", B, S)] = (torch.arange(B, device=self.dev) * S).to(torch.int32)
        cls_rows = self.buf[("ft.cls_rows", B, S)]
        tok = self._vit_embed_v1(video, keep, B, tubes, "ft", crop, channel_major, mix, aug)
        dp = None if table is None else (table, S)
        x = self._blocks_fwd("video_model.blocks.", _VIT_NAMES, tok, "ft", depth, hv, "gelu", 1e-6,
                             lambda qkv, att, lse: K.attn_fwd("full", qkv, att, lse, B=B, heads=hv, S=S, causal=False, head_dim=W // hv),
                             drop_path=dp, recompute=self.recompute)
        feat = self._f("ft.feat", (B, W))
        self._ln(x, "video_model.norm", 1e-6, feat, "ft.norm", rows=cls_rows)
        logits = self._f("ft.logits", (B, C))
        self._head_lin(feat, "head.weight", "head.bias", logits, B)
        self.ft_ctx = dict(B=B, tubes=tubes, S=S, keep=keep, cls_rows=cls_rows, drop_path=dp)
        return logits

    def finetune_backward(self, dlogits, trainable="all"):
        """dlogits fp32 [B, C] -> the gradients, ACCUMULATED into the store.  trainable "head": linear probing
        (run_class_linear.py:342-346), nothing behind the head runs."""
        if trainable not in ("all", "head"):
            raise ValueError("trainable: 'all' or 'head'")
        a, c, P, B_ = self.arch, self.ft_ctx, self.P, self.buf
        B, S, tubes, W, hv, depth = c["B"], c["S"], c["tubes"], a["width"], a["heads"], a["layers"]
        self.recompute_count = 0  # (trainable "head": the backward never reaches the blocks, nothing is evaluated again)
        dfeat = self._f("ft.dfeat", (B, W))
        self._head_lin_bwd(dlogits, B_["ft.feat"], "head.weight", "head.bias", dfeat, B)
        self._ready("head.")
        if trainable == "head":
            return
        dx, dxb = self._head_ln_bwd(dfeat, "video_model.norm", "ft", "ft.norm", depth, c["cls_rows"], False)
        dx = self._blocks_bwd("video_model.blocks.", _VIT_NAMES, "ft", depth, dx, dxb, hv, "gelu",
                              lambda qkv, *t: K.attn_bwd("full", qkv, *t, B=B, heads=hv, S=S, causal=False, head_dim=W // hv),
                              after=lambda l: self._ready(f"video_model.blocks.{l}."), drop_path=c["drop_path"],
                              redo=(1e-6, lambda qkv, att, lse: K.attn_fwd("full", qkv, att, lse, B=B, heads=hv, S=S, causal=False,
                                                                           head_dim=W // hv)))
        n = c["keep"].shape[2]
        Mp = B * tubes * n
        dpatch = self._b("ft.dpatch", (Mp, W))
        K.vit_assemble_bwd(dx, c["keep"], dpatch, P.g("video_model.cls_token").view(W), P.g("video_model.pos_embed").view(-1, W),
                           P.g("video_model.temporal_embed").view(-1, W), B=B, T=tubes, n=n)
        K.gemm_tn(dpatch, B_["ft.im2col"], P.g2d("video_model.patch_embed.proj.weight"), M=Mp, accumulate=True,
                  colsum=P.g("video_model.patch_embed.proj.bias"))
        self._ready("video_model.cls_token", "video_model.pos_embed", "video_model.temporal_embed", "video_model.patch_embed.")
        self._ready("video_model.norm.")

    # ------------------------------------------------------------------ whole model
    # uint8 wire formats of the pretraining step: the transform chain of v1/video_transforms/videoaug.py:8-22 behind
    # the decoder runs on the device -- Resize (Pillow's 8-bit bilinear resample, tvts_resize_crop_u8) and the crop at the head of
    # video_forward_v1, ClipToTensor and Normalize inside tvts_patch_gather_tube_u8.
    def _u8_batch(self, data: dict):
        """the HOST half of a uint8 batch: None for fp32 clips, else dict(B, T, clips, crop, plan) --
          no data["resize"]   clips uint8 [B, T, H0, W0, 3], already resized (or cropped: H0 = W0 = img); crop int32 [B, 2] (top, left)
                              from data["crop"], None = the centre crop; plan None
          data["resize"]      clips = a tensor [B, T, Hs, Ws, 3] or a list of B tensors [T, Hs_b, Ws_b, 3] at the decoder's sizes;
                              data["crop"] in RESIZED coordinates (None: centre); plan = hip.resize_plan(...), crop None (the plan has it)
        ValueError by name for: uint8 that is not [..., 3]; a clip with fewer frames than the batch's T (the reference zero-pads short
        clips BEHIND Normalize, v1/base/base_dataset.py:121-123, which uint8 frames cannot express); a (resized) side below img; a crop
        outside the (resized) frame.  Nothing here touches the device."""
        a, video = self.arch, data["video"]
        img = a["image"]
        ragged = isinstance(video, (list, tuple))
        if not ragged and video.dtype != torch.uint8:
            return None
        clips = list(video) if ragged else video
        if ragged and (not clips or any(not torch.is_tensor(c) or c.dtype != torch.uint8 for c in clips)):
            raise ValueError("video: a list of clips must hold uint8 tensors [T, Hs, Ws, 3]")
        for b, c in enumerate(clips if ragged else [video]):
            if c.dim() != (4 if ragged else 5) or c.shape[-1] != 3:
                raise ValueError(f"uint8 video must be [B, T, H, W, 3] (or a list of [T, H, W, 3] clips), got {tuple(c.shape)}"
                                 + (f" for clip {b}" if ragged else ""))
        B = len(clips) if ragged else int(video.shape[0])
        T = max(int(c.shape[0]) for c in clips) if ragged else int(video.shape[1])
        for b in range(B if ragged else 0):
            if int(clips[b].shape[0]) != T:
                raise ValueError(f"clip {b} has {int(clips[b].shape[0])} frames, the batch has clips of {T}: short clips are zero-padded "
                                 "behind Normalize by the reference, which uint8 frames cannot express (pad them on the host as fp32)")
        if T < a["tubelet"]:
            raise ValueError(f"clips of {T} frames: fewer than one tubelet of {a['tubelet']}")
        crop = data.get("crop")
        if crop is not None:
            crop = torch.as_tensor(crop).detach().to("cpu", torch.int32).contiguous()
            if tuple(crop.shape) != (B, 2):
                raise ValueError(f"crop {tuple(crop.shape)}: expected [{B}, 2] (top, left)")
        if data.get("resize") is None:
            if ragged:
                raise ValueError("a list of clips needs data['resize']: without it the frames are one tensor [B, T, H0, W0, 3]")
            H0, W0 = int(video.shape[2]), int(video.shape[3])
            if H0 < img or W0 < img:
                raise ValueError(f"uint8 frames of {H0} x {W0}: a side below the crop of {img} x {img}")
            if crop is not None and bool(((crop < 0) | (crop[:, :1] > H0 - img) | (crop[:, 1:] > W0 - img)).any()):
                raise ValueError(f"crop outside the frame: needs 0 <= top <= {H0 - img} and 0 <= left <= {W0 - img}")
            return dict(B=B, T=T, clips=video, crop=crop, plan=None)
        sizes = [(int(c.shape[1]), int(c.shape[2])) for c in clips] if ragged else [(int(video.shape[2]), int(video.shape[3]))] * B
        plan = K.resize_plan(sizes, None if crop is None else crop.tolist(), size=int(data["resize"]), img=img, T=T)
        return dict(B=B, T=T, clips=clips, crop=None, plan=plan)

    def _u8_pb(self, u8, d):
        """the prepared batch's share of a uint8 batch (d: the device tensors of _stage_small)"""
        if u8 is None:
            return {}
        out = dict(crop=d.get("crop"))
        if u8["plan"] is not None:
            out["resize"] = dict(desc=d["rs_desc"], tables=d["rs_tables"], tmp_rows=u8["plan"]["tmp_rows"])
        return out

    def prepare_batch(self, data: dict):
        """v1 batch dict (v1/trainer/trainer.py:121-131): text = the tokenizer's {'input_ids', 'attention_mask'} (right-padded),
        video fp32 [B, T, 3, H, W] or one of the uint8 wire formats of _u8_batch, keep_ind int64 [B, n_tubes, n_keep] (one mask per
        tube) or, without it, mask_seed (+ sample_offset): the masks drawn on the device."""
        a = self.arch
        u8 = self._u8_batch(data)  # (host only: the uint8 wire formats below, checked before anything reaches the device)
        if "keep_ind" not in data and "mask_seed" not in data:
            raise KeyError("batch dict needs 'keep_ind' or 'mask_seed' (+ optional 'sample_offset')")
        vsmall = {}  # the small tensors of a uint8 batch: they travel in one staging copy (_stage_small)
        if u8 is None:
            video = self._clip_to_device(data["video"]).to(torch.float32).contiguous()
            B, T = video.shape[:2]
        else:
            B, T = u8["B"], u8["T"]
            video = self._packed_to_device(u8["clips"], u8["plan"]) if u8["plan"] is not None else self._clip_to_device(u8["clips"]).contiguous()
            if u8["crop"] is not None:
                vsmall["crop"] = u8["crop"]
            if u8["plan"] is not None:
                vsmall["rs_desc"], vsmall["rs_tables"] = torch.from_numpy(u8["plan"]["desc"]), torch.from_numpy(u8["plan"]["tables"])
        tubes = T // a["tubelet"]
        from .model.model_dist_TVTS import right_padded, tokenizer_inputs  # (that module imports this one)
        text = {k: data["text"][k].detach().to("cpu", torch.int64) for k in ("input_ids", "attention_mask")}
        assert right_padded(text["attention_mask"]), "attention_mask must be a right-padded prefix mask"
        if self.text_unpadded:  # (the packed descriptors are made on the host and travel in one copy: _prepare_unpadded)
            N, L = text["input_ids"].shape[0], int(text["attention_mask"].sum(-1).max())
        else:
            ids, kv_len, N, L = tokenizer_inputs(text, self.dev)
        NT = N // B
        if "keep_ind" in data:
            keep = data["keep_ind"][:, :tubes].to(torch.int32).contiguous().to(self.dev)
        else:
            # device-drawn tube masks: row (sample_offset + b) * n_temp + t of tvts_tube_mask is tube t of global clip sample_offset + b, so
            # the draw depends on neither the batch split nor the clip length (the reference draws n_temp masks per clip in the dataset
            # worker, v1/base/base_dataset.py:129-140, and ships them with the batch)
            from .arch import n_keep, patches_per_frame
            n_temp = a["num_frames"] // a["tubelet"]
            if tubes > n_temp:
                raise ValueError(f"mask_seed: clips of {tubes} tubes, the model draws {n_temp} masks per clip")
            keep = K.tube_mask(int(data["mask_seed"]), int(data.get("sample_offset", 0)) * n_temp, B * n_temp, patches_per_frame(a),
                               n_keep(a), device=self.dev).view(B, n_temp, -1)[:, :tubes].contiguous()
        n = keep.shape[2]
        S = 1 + tubes * n
        So = S + NT
        if self.text_unpadded:
            return self._prepare_unpadded(text, dict(video=video, keep=keep, B=B, T=T, tubes=tubes, N=N, NT=NT, L=L, n=n, S=S), So, u8, vsmall)
        pb_u8 = self._u8_pb(u8, self._stage_small(vsmall) if vsmall else {})
        return dict(video=video, ids=ids, kv_len=kv_len, **pb_u8,
                    tok_sort=tuple(t.to(self.dev) for t in K.token_sort(text["input_ids"][:, :L])),  # ordered word-embedding gradient sums
                    txt_cls_rows=(torch.arange(N) * L).to(torch.int32).to(self.dev), keep=keep, B=B, T=T, tubes=tubes, N=N, NT=NT, L=L,
                    n=n, S=S, vid_rows=(torch.arange(B) * S).to(torch.int32).to(self.dev),
                    sort_rows=(torch.arange(B)[:, None] * So + S + torch.arange(NT)[None, :]).reshape(-1).to(torch.int32).to(self.dev),
                    sort_rows64=(torch.arange(B)[:, None] * So + S + torch.arange(NT)[None, :]).reshape(-1).to(self.dev))

    MAX_UNPADDED = 80  # the longest caption the packed attention kernels take (tile classes up to 5 x 16 rows)

    def _prepare_unpadded(self, text, pb, So, u8=None, vsmall=None):
        """the text half of prepare_batch under arch["text_unpadded"]: the captions packed by their lengths (hip.pack_captions), every
        descriptor and row table of the batch in ONE staging copy (_stage_small) -- the crop, resize descriptor and tap tables of a
        uint8 batch (vsmall) among them.  pb["L"] stays the longest caption: the L of the padded step, which the dropout masks are
        drawn for."""
        lens = text["attention_mask"].sum(-1)
        if int(lens.max()) > self.MAX_UNPADDED:
            raise ValueError(f"text_unpadded: a caption of {int(lens.max())} tokens, the packed attention kernels take at most "
                             f"{self.MAX_UNPADDED} (the trainer's tokenizer call truncates at 50)")
        if int(lens.min()) < 1:
            raise ValueError("text_unpadded: a caption without tokens")
        B, NT, S = pb["B"], pb["NT"], pb["S"]
        pk = K.pack_captions(text["input_ids"], self.arch["max_pos"], lens=lens)
        small = {k: pk[k] for k in ("ids", "seq_start", "cls_rows", "tok_order", "tok_seg", "pos_order", "pos_seg")}
        small["vid_rows"] = (torch.arange(B) * S).to(torch.int32)
        small["sort_rows"] = (torch.arange(B)[:, None] * So + S + torch.arange(NT)[None, :]).reshape(-1).to(torch.int32)
        small.update(vsmall or {})
        d = self._stage_small(small)
        pb.update(self._u8_pb(u8, d))
        M = int(pk["ids"].numel())
        pb.update(ids=d["ids"], kv_len=None, tok_sort=(d["tok_order"], d["tok_seg"]), txt_cls_rows=d["cls_rows"], vid_rows=d["vid_rows"],
                  sort_rows=d["sort_rows"], sort_rows64=d["sort_rows"].to(torch.int64), M=M, seq_start=d["seq_start"],
                  max_len=pk["max_len"], txt_pk=dict(seq_start=d["seq_start"], max_len=pk["max_len"], M=M,
                                                     pos_sort=(d["pos_order"], d["pos_seg"])))
        return pb

    def forward(self, pb: dict):
        a = self.arch
        self.ctx = pb
        self._tick += 1  # (workspace: a buffer whose shape changes from here on belongs to a new step, see _b)
        B, N, NT, L, S, E = pb["B"], pb["N"], pb["NT"], pb["L"], pb["S"], a["embed"]
        before, t = self.text_forward_v1(pb["ids"], pb["kv_len"], pb["txt_cls_rows"], N, L, pk=pb.get("txt_pk"))
        text_emb = self._f("mdl.text_emb", (B, E))
        tmean_scratch = self._f("mdl.text_before_e", (B, NT, E))
        K.text_mean(t, text_emb, tmean_scratch, NT=NT, B=B)          # mean over the NT captions (model_dist_TVTS.py:104-107)
        text_before = self._f("mdl.text_before", (B, NT, a["text_width"]))
        K.text_mean(before, self._f("mdl.tb_mean", (B, a["text_width"])), text_before, NT=NT, B=B)  # [NT,B,W] -> [B,NT,W] (:99-101)
        out, video_emb = self.video_forward_v1(pb["video"], pb["keep"], B, pb["tubes"], pb["vid_rows"], pb.get("crop"), pb.get("resize"))
        if self.embeds_ready is not None:
            self.embeds_ready(text_emb, video_emb)
        pred = self.sort_forward(out, text_before, B, S, NT) if NT != 1 else None
        return text_emb, video_emb, pred

    def backward(self, d_text, d_video, d_pred):
        a, pb, P = self.arch, self.ctx, self.P
        B, N, NT, L, S, E, W = pb["B"], pb["N"], pb["NT"], pb["L"], pb["S"], a["embed"], a["width"]
        if d_text is not None:
            dt = self._f("mdl.dt", (N, E))
            K.text_mean_bwd(d_text, dt, NT=NT, B=B)
            self.text_backward_v1(dt, pb["ids"], pb["kv_len"], pb["txt_cls_rows"], N, L, tok_sort=pb.get("tok_sort"), pk=pb.get("txt_pk"))
            self._ready("text_model.")
            self._ready("txt_proj.")
        # vid_proj on the CLS token: dW += d_video^T cls, db += colsum, d_cls = d_video W
        dcls = self._f("vit.dcls", (B, W))
        self._head_lin_bwd(d_video, self.buf["vit.cls"], "vid_proj.0.weight", "vid_proj.0.bias", dcls, B)
        self._ready("vid_proj.")
        dout = self._b("mdl.dout", (B * S, W))
        if d_pred is not None:
            dxs = self.sort_backward(d_pred, B, S, NT)
            K.sort_assemble_bwd(dxs, dcls, dout, P.g("pred_model.type_embed").view(2, W), B=B, S=S, off=0, Sv=S, NT=NT)
            self._ready("pred_model.")
        else:
            K.sort_assemble_bwd(None, dcls, dout, None, B=B, S=S, off=0, Sv=S, NT=NT)
        self.video_backward_v1(dout, pb["keep"], B, pb["tubes"])

    # ------------------------------------------------------------------ forward-only encoders (feature extraction, retrieval)
    # The v1 counterparts of Engine.encode_video / encode_text.  They run the training step's own forward wiring -- _vit_embed_v1
    # and Engine._blocks_fwd, _text_tower_v1 over _pln_fwd, _head_lin -- with tag None: every buffer is an encoder workspace (_ib)
    # instead of a named tensor of the step, so nothing of Engine.buf is read, written or resized and a call between two training
    # steps leaves the step alone.  No log-sum-exp, no pre-activations, no LayerNorm statistics are kept, and the LAST block of
    # either tower runs for the rows the model reads: its keys / values come from every row, its one query per sequence is the
    # CLS / [CLS] row (tvts_attn_fwd_first), and everything behind the attention (output projection, residuals, LayerNorms,
    # MLP / FFN) is computed for those B (N) rows only.
    # Seed rule: the text encoder NEVER applies dropout and NEVER advances drop_seed, whatever `training` says -- it is an
    # inference call, and an encoder call between two training steps must not shift the step's mask sequence.
    # (_advance_drop_seed is text_forward_v1's alone, and with tag None _pln_fwd / _text_tower_v1 do not look at _drop_active.)
    # Base-class refusal (_inf_check) stays for encode_text_packed (the causal CLIP pass); the packed DistilBERT pass is encode_text
    # with a descriptor `pk` (TVTS.encode_text(text, packed=True)).
    def encode_video(self, video, keep, B, tubes, crop=None, channel_major=False, project=True, view=None):
        """-> (feat [B, W] fp32 = the normed CLS token, emb [B, E] = vid_proj(feat)).  Both are encoder workspaces: the next
        encoder call overwrites them.  project=False returns emb = None (a store without vid_proj: the downstream class).
        video, on the device: fp32 [B, T, 3, H, W]; fp32 [B, 3, T, H, W] with channel_major (the layout of the v1 downstream
        classes); or uint8 [B, T, H0, W0, 3].  keep: int32 [B, tubes, n].
        crop (uint8 only): int32 [B, 2] (top, left) inside the frame, None = centre crop.  It is an argument of the engine alone:
        TVTS.encode_video and the downstream class always take the centre crop.
        view (uint8 only): the device table of hip.view_table() for B samples over source clips [Bs, Tsrc, H0, W0, 3] -- B test views of
        tubes * tubelet frames each, formed inside the gather (downstream/evaluate_v1.py); None: the path above, launch for launch."""
        a, f32 = self.arch, torch.float32
        W, E, hv = a["width"], a["embed"], a["heads"]
        S = 1 + tubes * keep.shape[2]
        tok = self._vit_embed_v1(video, keep, B, tubes, None, crop, channel_major, view=view)
        x_c = self._blocks_fwd(
            "video_model.blocks.", _VIT_NAMES, tok, None, a["layers"], hv, "gelu", 1e-6,
            lambda qkv, att, lse: K.attn_fwd("full", qkv, att, lse, B=B, heads=hv, S=S, causal=False, head_dim=W // hv),
            rows=self._row_starts("vid_rows", B, S),
            attn_rows=lambda qkv, att, lse: K.attn_fwd_first(qkv, None, att, lse, B=B, heads=hv, S=S, head_dim=W // hv))
        feat = self._ib("vfeat", (B, W), f32)
        self._ln(x_c, "video_model.norm", 1e-6, feat, None)
        if not project:
            return feat, None
        emb = self._ib("vemb", (B, E), f32)
        self._head_lin(feat, "vid_proj.0.weight", "vid_proj.0.bias", emb, B)
        return feat, emb

    def encode_text(self, ids, kv_len, N, L, pk=None):
        """-> (before [N, Wt] fp32 = DistilBERT's last hidden state at [CLS], emb [N, E] = txt_proj(relu(before))); both encoder
        workspaces.  ids int32 [N, L], kv_len int32 [N] (right-padded captions) on the device.  No dropout, drop_seed untouched.
        pk: packed captions instead (ids int32 [M]; dict of seq_start, cls_rows, max_len, M on the device, hip.pack_captions(lens=...))."""
        if pk is not None:
            return self._text_tower_v1(ids, None, pk["cls_rows"], N, L, None, pk=pk)
        return self._text_tower_v1(ids, kv_len, self._row_starts("cls_rows", N, L), N, L, None)
