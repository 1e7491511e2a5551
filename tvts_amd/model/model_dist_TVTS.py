"""Drop-in for v1/model/model_dist_TVTS.py: ``TVTS(args, video_params, text_params, projection_dim=256,
load_checkpoint=None, projection='minimal')`` -- DistilBERT text tower, tubelet ViT-B/16 with joint space-time attention,
ReLU+Linear / Linear projections, transcript-sorting head -- over the HIP step engine (tvts_amd/engine_v1.py).  Same
``forward(data, return_embeds=True) -> (text_embeds, video_embeds, pred_order)``, ``compute_text`` / ``compute_video``,
state-dict names and order, ``sim_matrix`` as an importable free function.

The text tower's dropout (Hugging Face DistilBERT, p = 0.1, active because of ``self.text_model.train()`` at
model_dist_TVTS.py:33-34) follows the module's training flag: ``model.train()`` steps draw counter-based masks
(tvts_amd/engine_v1.py), ``model.eval()`` (validation, compute_text for retrieval) runs without.  The pretrained initialisations (``AutoModel.from_pretrained``, ``./mae_pretrain_vit_base.pth``, :34,49-58) are
replaced by the same classes' random initialisers unless ``load_checkpoint`` names a checkpoint.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..arch import ARCH_V1
from ..engine_v1 import EngineV1
from ._common import TVTSv2Base, sim_matrix  # noqa: F401


def reference_init_v1_(store, seed: int = 0):
    """DistilBERT: N(0, 0.02) weights / embeddings, zero biases, LayerNorm (1, 0) (transformers _init_weights); ViT: trunc-normal
    0.02 Linear weights, zero biases, LayerNorm (1, 0), cls / pos trunc-normal 0.02, temporal zeros, Conv3d default
    (v1/model/video_encoder.py:146-166); projections: nn.Linear default; sort head as in v2."""
    g = torch.Generator().manual_seed(seed)
    for name, shape in store.shapes.items():
        leaf = name.rsplit(".", 1)[-1]
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
        if "norm" in name.lower() and "type_embed" not in name:
            t = torch.ones(shape) if leaf == "weight" else torch.zeros(shape)
        elif name in ("video_model.temporal_embed", "pred_model.type_embed"):
            t = torch.zeros(shape)
        elif name.startswith("text_model.") or name in ("video_model.cls_token", "video_model.pos_embed"):
            t = torch.zeros(shape) if leaf == "bias" else torch.randn(shape, generator=g) * 0.02
        elif name.startswith("video_model.blocks."):
            t = torch.zeros(shape) if leaf == "bias" else (torch.randn(shape, generator=g) * 0.02).clamp_(-0.04, 0.04)
        elif leaf == "bias":
            w_shape = store.shapes[name[:-4] + "weight"]
            t = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(int(np.prod(w_shape[1:])))
        else:
            t = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
        store.p(name).copy_(t.to(store.device))


def right_padded(mask) -> bool:
    """is every row of the [N, L] attention mask a run of ones followed by zeros?"""
    return bool((mask == (torch.arange(mask.shape[1])[None] < mask.sum(-1)[:, None])).all())


def tokenizer_inputs(text, device, validate=False, arch=None):
    """the tokenizer's {'input_ids', 'attention_mask'} (right-padded) -> (ids int32 [N, L] on the device, cut at the longest
    caption; kv_len int32 [N] on the device, the captions' lengths; N; L): the text arguments of EngineV1.text_forward_v1 /
    encode_text.  validate: refuse what the kernels would not survive or would silently misread -- ValueError for shapes and
    masks, IndexError for token ids outside arch's vocabulary and captions longer than its position table."""
    ids = text["input_ids"].detach().to("cpu", torch.int64)
    mask = text["attention_mask"].detach().to("cpu", torch.int64)
    if validate and (ids.dim() != 2 or ids.numel() == 0 or mask.shape != ids.shape):
        raise ValueError(f"text: expected [N, L] input_ids and attention_mask, got {tuple(ids.shape)} / {tuple(mask.shape)}")
    lens = mask.sum(-1)
    if validate and (not right_padded(mask) or int(lens.min()) < 1):
        raise ValueError("attention_mask must be a non-empty right-padded prefix mask")
    N, L = ids.shape[0], int(lens.max())
    if validate and (int(ids.min()) < 0 or int(ids.max()) >= arch["vocab"] or L > arch["max_pos"]):
        raise IndexError(f"token ids must lie in [0, {arch['vocab']}) and captions within the {arch['max_pos']} positions")
    return ids[:, :L].to(torch.int32).contiguous().to(device), lens.to(torch.int32).to(device), N, L


class TVTS(TVTSv2Base):
    ENGINE = EngineV1
    INIT = staticmethod(reference_init_v1_)

    def __init__(self, args, video_params=None, text_params=None, projection_dim=256, load_checkpoint=None,
                 projection="minimal", arch=None, init_seed=0, grad_checkpointing=None):
        video_params = video_params or {}
        text_params = text_params or {"model": "distilbert-base-uncased", "pretrained": True}
        if arch is None:
            if not text_params.get("pretrained", True):
                raise NotImplementedError("Huggingface text models require pretrained init.")  # model_dist_TVTS.py:31-32
            if not text_params.get("model", "distilbert-base-uncased").startswith("distilbert"):
                raise NotImplementedError("only the distilbert-base-uncased text tower of the shipped configs is built")
            if video_params.get("arch_config", "base_patch16_224") != "base_patch16_224" or projection != "minimal":
                raise NotImplementedError
            arch = dict(ARCH_V1, num_frames=video_params.get("num_frames", 16), embed=projection_dim)
        self.video_params, self.text_params = video_params, text_params
        super().__init__(args, load_checkpoint=load_checkpoint, arch=arch, init_seed=init_seed, grad_checkpointing=grad_checkpointing)

    def forward(self, data, return_embeds=True):
        self.engine.training = self.training  # dropout of the text tower in training mode only
        return super().forward(data, return_embeds)

    # pieces the reference exposes (model_dist_TVTS.py:131-147)
    def compute_text(self, text_data):
        self._fresh_shadows()
        eng = self.engine
        eng.training = self.training
        ids, kv_len, N, L = tokenizer_inputs(text_data, self.store.device)
        before, t = eng.text_forward_v1(ids, kv_len, (torch.arange(N) * L).to(torch.int32).to(self.store.device), N, L)
        return before.clone(), t.clone()

    def compute_video(self, video_data, keep_ind):
        self._fresh_shadows()
        a = self.arch
        v = video_data.to(self.store.device, torch.float32).contiguous()
        B, T = v.shape[:2]
        tubes = T // a["tubelet"]
        keep = keep_ind[:, :tubes].to(torch.int32).contiguous().to(self.store.device)
        S = 1 + tubes * keep.shape[2]
        out, emb = self.engine.video_forward_v1(v, keep, B, tubes, (torch.arange(B) * S).to(torch.int32).to(self.store.device))
        return out.view(B, S, -1).clone(), emb.clone()

    # forward-only encoders (feature extraction, retrieval): EngineV1.encode_video / encode_text -- no per-layer activations, the
    # last block of either tower for the rows the model reads, never any dropout (whatever .training says) and no advance of
    # the training step's mask seed
    @torch.no_grad()
    def encode_video(self, video, keep_ind=None, project=True):
        """-> [B, E] video embeddings, or with project=False the normed CLS feature [B, W] (compute_video's tokens[:, 0]).
        video: fp32 [B, T, 3, H, W] or uint8 [B, T, H0, W0, 3] frames (centre crop, / 255, ImageNet Normalize on the device);
        keep_ind: kept patches per tube [tubes, n] (every clip) or [B, tubes, n], None = every patch of every tube."""
        self._fresh_shadows()
        feat, emb = _encode_video_v1(self.engine, video, keep_ind, channel_major=False, project=project)
        return (emb if project else feat).clone()

    @torch.no_grad()
    def encode_text(self, text_dict, packed=False):
        """-> [N, E] caption embeddings (compute_text's second output in eval mode) from the tokenizer's
        {'input_ids', 'attention_mask'} (right-padded).  packed: the tower over sum(len_i) token rows instead of N * max(len_i)
        (captions of at most 80 tokens, bidirectional packed attention); the default gives the padded pass, bit for bit."""
        self._fresh_shadows()
        if not packed:
            _, t = self.engine.encode_text(*tokenizer_inputs(text_dict, self.store.device, validate=True, arch=self.arch))
            return t.clone()
        from .. import hip as K
        eng = self.engine
        longest = int(text_dict["attention_mask"].sum(-1).max())
        if longest > eng.MAX_UNPADDED:
            raise ValueError(f"encode_text(packed=True): a caption of {longest} tokens, the packed attention kernels take at most "
                             f"{eng.MAX_UNPADDED}")
        _, _, N, L = tokenizer_inputs(text_dict, "cpu", validate=True, arch=self.arch)  # (the checks; the rectangle stays on the host)
        pk = K.pack_captions(text_dict["input_ids"].detach().to("cpu", torch.int64), self.arch["max_pos"],
                             lens=text_dict["attention_mask"].detach().to("cpu", torch.int64).sum(-1))
        d = eng._stage_small({k: pk[k] for k in ("ids", "seq_start", "cls_rows")})
        _, t = eng.encode_text(d["ids"], None, N, L, pk=dict(seq_start=d["seq_start"], cls_rows=d["cls_rows"], max_len=pk["max_len"],
                                                             M=int(pk["ids"].numel())))
        return t.clone()


def _encode_video_v1(engine, video, keep_ind, channel_major, project):
    """the argument checks of the v1 video encoders (TVTS.encode_video, downstream VisionTransformer) in front of
    EngineV1.encode_video; mirrors TVTSv2Base.encode_video.  channel_major: fp32 clips arrive as [B, 3, T, H, W]."""
    a, dev = engine.arch, engine.dev
    if video.dim() != 5:
        raise ValueError(f"video: expected a 5-D clip batch, got {tuple(video.shape)}")
    if video.dtype == torch.uint8:
        if video.shape[-1] != 3 or video.shape[2] < a["image"] or video.shape[3] < a["image"]:
            raise ValueError(f"uint8 video must be [B, T, H, W, 3] with H, W >= {a['image']}, got {tuple(video.shape)}")
        v = video.to(dev).contiguous()
        T, channel_major = v.shape[1], False
    else:
        want = (3, None, a["image"], a["image"]) if channel_major else (None, 3, a["image"], a["image"])
        if any(w is not None and w != s for w, s in zip(want, video.shape[1:])):
            raise ValueError(f"video must be fp32 {'[B, 3, T, H, W]' if channel_major else '[B, T, 3, H, W]'} with H = W = "
                             f"{a['image']} (or uint8 [B, T, H0, W0, 3]), got {tuple(video.shape)}")
        v = video.to(dev, torch.float32).contiguous()
        T = v.shape[2] if channel_major else v.shape[1]
    B, tb = v.shape[0], a["tubelet"]
    if T == 0 or T % tb:
        raise ValueError(f"clips of {T} frames: not a multiple of the tubelet size {tb}")
    if T > a["num_frames"]:
        raise ValueError(f"clips of {T} frames, the temporal embedding has {a['num_frames'] // tb} rows of {tb} frames")
    tubes, ppf = T // tb, (a["image"] // a["patch"]) ** 2
    kc = torch.arange(ppf).view(1, 1, ppf).expand(1, tubes, ppf) if keep_ind is None else keep_ind
    if kc.dim() == 2:
        kc = kc.unsqueeze(0)
    if kc.dim() != 3 or kc.shape[0] not in (1, B) or kc.shape[1] != tubes or kc.shape[2] == 0:
        raise ValueError(f"keep_ind {tuple(kc.shape)}: expected [{tubes}, n_keep] or [{B}, {tubes}, n_keep]")
    if int(kc.min()) < 0 or int(kc.max()) >= ppf:
        raise IndexError(f"keep_ind must index the {ppf} patches of a frame")
    keep = kc.expand(B, -1, -1).to(dev, torch.int32).contiguous()
    return engine.encode_video(v, keep, B, tubes, channel_major=channel_major, project=project)
