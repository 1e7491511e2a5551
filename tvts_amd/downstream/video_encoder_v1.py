"""Drop-in for v1/downstream/video_encoder_zero.py and v1/downstream/video_encoder.py: ``VisionTransformer(img_size=224,
patch_size=16, ..., num_frames=16, tubelet_size=2)`` -- the pretrain video tower without mask (Conv3d tubelet embedding, joint
space-time attention, pre-LN blocks), read at the normed CLS token (video_encoder_zero.py:176-207), plus ``head`` when
``num_classes > 0`` (video_encoder.py:204-208) -- over the forward-only encoder of the HIP engine (EngineV1.encode_video).

Same constructor keywords, same state-dict keys in the same order (``cls_token, pos_embed, temporal_embed, patch_embed.proj.*,
blocks.i.*, norm.*[, head.*]``), so ``model.load_state_dict(state_dict, strict=False)`` works as v1/downstream/run_class_zero.py
uses it (:336-340); ``VisionTransformer.from_pretrain(checkpoint, ...)`` applies the script's ``module.video_model.`` key filter.
The parameter store holds the video tower and the head only (no DistilBERT, no sorting head).  ``forward`` / ``forward_features``
are inference calls in every module mode: they run under ``no_grad``, parameters have ``requires_grad=False`` (there is no autograd
graph; the hand-written backward writes into the store's flat gradient buffer), dropout rates are accepted and have no effect, and
``drop_path_rate`` has no effect on them either.  Training this class -- action-recognition fine-tuning and linear probing -- is
``tvts_amd.downstream.finetune_v1.FinetuneStep``, which reads ``drop_path_rate``, ``grad_views()`` and ``set_trainable()`` here.
"""
from __future__ import annotations

import functools

import torch
import torch.nn as nn

from .. import hip as K
from ..arch import ARCH_V1, recompute_mode
from ..engine import ParamStore
from ..engine_v1 import EngineV1
from ..model._common import _require_gpu
from ..model.model_dist_TVTS import _encode_video_v1, reference_init_v1_

_PREFIX = "video_model."


def _norm_eps(norm_layer):
    """the eps of the reference's norm_layer argument: None = partial(nn.LayerNorm, eps=1e-6) (video_encoder_zero.py:122)"""
    if norm_layer is None:
        return 1e-6
    if isinstance(norm_layer, functools.partial) and norm_layer.func is nn.LayerNorm and not norm_layer.args:
        return float(norm_layer.keywords.get("eps", 1e-5))
    if norm_layer is nn.LayerNorm:
        return 1e-5
    raise NotImplementedError("norm_layer: only nn.LayerNorm is built")


class VisionTransformer(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=0, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.,
                 qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., norm_layer=None, num_frames=16,
                 tubelet_size=2, representation_size=None, device_index=0, init_seed=0, grad_checkpointing=False):
        super().__init__()
        if not qkv_bias:
            raise NotImplementedError("qkv_bias=False is not built (every shipped v1 checkpoint has the bias)")
        if representation_size:
            raise NotImplementedError("representation_size (the pre_logits layer) is not built")
        if embed_dim % num_heads or embed_dim // num_heads != 64:
            raise NotImplementedError(f"the v1 encoder's attention kernels are used at head dim 64, not {embed_dim}/{num_heads}")
        if in_chans != 3 or float(mlp_ratio) != 4.0:
            raise NotImplementedError("in_chans = 3 and mlp_ratio = 4 are what is built")
        if qk_scale is not None and abs(float(qk_scale) - 64 ** -0.5) > 1e-12:
            raise NotImplementedError("qk_scale other than head_dim ** -0.5 is not built")
        if _norm_eps(norm_layer) != 1e-6:
            raise NotImplementedError("LayerNorm eps other than 1e-6 is not built")
        img_size = img_size[0] if isinstance(img_size, (tuple, list)) else img_size
        patch_size = patch_size[0] if isinstance(patch_size, (tuple, list)) else patch_size
        if img_size % patch_size or patch_size % 8 or tubelet_size < 1 or num_frames < tubelet_size or num_classes < 0:
            raise ValueError("img_size must be a multiple of patch_size, patch_size of 8, num_frames >= tubelet_size >= 1")
        self.num_classes = int(num_classes)
        self.num_features = self.embed_dim = int(embed_dim)
        self.tubelet_size = int(tubelet_size)
        self.patches_per_frame = (img_size // patch_size) ** 2
        self.arch = dict(ARCH_V1, name="v1_video", image=int(img_size), patch=int(patch_size), tubelet=int(tubelet_size),
                         width=int(embed_dim), heads=int(num_heads), layers=int(depth), num_frames=int(num_frames),
                         towers="video", head_classes=self.num_classes, sort_head=False,
                         recompute=recompute_mode(grad_checkpointing))  # (FinetuneStep's backward; a bool or a mode string)
        dev = _require_gpu(device_index)
        self.store = ParamStore(self.arch, dev)
        self.engine = EngineV1(self.store)
        self.engine.training = False
        self.drop_path_rate = float(drop_path_rate)  # stochastic depth of FinetuneStep (video_encoder.py:138); forward ignores it
        self.engine.drop_path_rate = self.drop_path_rate
        reference_init_v1_(self.store, init_seed)
        for name in self.store.shapes:  # the reference's names: the tower's without the pretrain model's prefix
            parts = (name[len(_PREFIX):] if name.startswith(_PREFIX) else name).split(".")
            mod = self
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, nn.Module())
                mod = mod._modules[p]
            mod.register_parameter(parts[-1], nn.Parameter(self.store.p(name), requires_grad=False))
        self._versions = None
        self.eval()

    @staticmethod
    def pretrain_state_dict(checkpoint):
        """the video tower's entries of a pretrain checkpoint ({'state_dict': ...} or the state dict itself) under this class's
        names: the key filter of v1/downstream/run_class_zero.py:336-338"""
        sd = checkpoint["state_dict"] if "state_dict" in checkpoint else checkpoint
        return {k.replace("module.video_model.", ""): v for k, v in sd.items() if "module.video_model." in k}

    @classmethod
    def from_pretrain(cls, checkpoint, **kwargs):
        """a model with the video tower of a pretrain checkpoint loaded the way the script does (strict=False: `head.*` keeps its
        initialisation); checkpoint: a path, {'state_dict': ...} or a state dict with `module.video_model.` keys"""
        if isinstance(checkpoint, (str, bytes)) or hasattr(checkpoint, "__fspath__"):
            checkpoint = torch.load(checkpoint, map_location="cpu", weights_only=False)
        model = cls(**kwargs)
        sd = cls.pretrain_state_dict(checkpoint)
        if not sd:
            raise KeyError("the checkpoint has no `module.video_model.` entries")
        model.load_state_dict(sd, strict=False)
        return model

    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    # ---- what finetune_v1 needs: names, gradient views, the trainable map, the shadow bookkeeping
    @staticmethod
    def store_name(name: str) -> str:
        """the parameter store's name of the parameter `name` of this module"""
        return name if name.startswith("head.") else _PREFIX + name

    def grad_views(self):
        """{parameter name: view of the store's flat fp32 gradient buffer}, in named_parameters() order"""
        return {n: self.store.g(self.store_name(n)) for n, _ in self.named_parameters()}

    def set_trainable(self, trainable: str = "all"):
        """the engine's requires_grad map: "all" -- every parameter; "head" -- linear probing, head.* only
        (run_class_linear.py:342-346).  -> {parameter name: bool}"""
        if trainable not in ("all", "head"):
            raise ValueError("trainable: 'all' or 'head'")
        if self.num_classes == 0:
            raise ValueError("a model without head (num_classes = 0) has nothing to fine-tune")
        out = {}
        for n, _ in self.named_parameters():
            out[n] = self.engine.requires_grad[self.store_name(n)] = trainable == "all" or n.startswith("head.")
        return out

    def set_grad_checkpointing(self, enable=True):
        """activation recomputation in FinetuneStep's backward: True -- "block" (every block is evaluated again from its kept input,
        drop-path table and all, instead of keeping what it saves), False -- "none", or a mode string ("none" / "mlp" / "block").
        Same logits, loss, gradient norm and update, bit for bit.  May be called between steps; workspaces only grow."""
        self.engine.set_recompute(recompute_mode(enable))

    def mark_shadows_fresh(self):
        """the fused optimizer rewrote the bf16 shadows together with the parameters"""
        self._versions = tuple(p._version for p in self.parameters())

    def _fresh_shadows(self):
        """re-derive the bf16 weight shadows iff some parameter changed since the last refresh (load_state_dict copies in place)"""
        vers = tuple(p._version for p in self.parameters())
        if vers != self._versions:
            self.store.refresh_shadows()
            self._versions = vers

    @torch.no_grad()
    def forward_features(self, x):
        """x: fp32 [B, 3, T, H, W] (the reference's layout) or uint8 frames [B, T, H0, W0, 3] (centre crop + normalisation on the
        device) -> [B, embed_dim] = norm(blocks(tokens))[:, 0]"""
        self._fresh_shadows()
        feat, _ = _encode_video_v1(self.engine, x, None, channel_major=True, project=False)
        return feat.clone()

    def _head(self, feat):
        if self.num_classes == 0:
            return feat
        B, W, C = feat.shape[0], self.embed_dim, self.num_classes
        logits = torch.empty(B, C, dtype=torch.float32, device=feat.device)
        K.gemm_small(feat, self.store.p("head.weight"), logits, M=B, N=C, K=W, sa=(W, 1), sb=(1, W), bias=self.store.p("head.bias"))
        return logits

    @torch.no_grad()
    def forward(self, x):
        return self._head(self.forward_features(x))

    @torch.no_grad()
    def forward_views(self, frames, view_i, T):
        """forward() over test views cut from uint8 SOURCE clips on the device (v1/downstream/ssv2.py:132-164): frames uint8
        [Bs, Tsrc, H0, W0, 3], view_i integer [B, 8] = (src, t0, tstep, top, left, 0, 0, 0) on the host (hip.view_table checks it), T the
        frames per view.  Sample b is frames[src, t0::tstep][:T, top:top + img, left:left + img], normalised inside the gather: the
        result is forward() on those B uint8 clips, bit for bit, from one upload of the source clips.  -> [B, num_classes] (or the
        features [B, embed_dim] without a head).  tvts_amd.downstream.evaluate_v1.final_test(views=...) is the caller."""
        a, dev = self.arch, self.engine.dev
        if frames.dim() != 5 or frames.dtype != torch.uint8 or frames.shape[-1] != 3:
            raise ValueError(f"frames: uint8 source clips [Bs, Tsrc, H0, W0, 3], got {frames.dtype} {tuple(frames.shape)}")
        tb = a["tubelet"]
        if T < 1 or T % tb or T > a["num_frames"]:
            raise ValueError(f"views of {T} frames: need a multiple of {tb}, at most {a['num_frames']}")
        v = frames.to(dev).contiguous()
        table = K.view_table(view_i, Bs=v.shape[0], Tsrc=v.shape[1], H0=v.shape[2], W0=v.shape[3], T=T, img=a["image"], device=dev)
        B, tubes, ppf = table.shape[0], T // tb, self.patches_per_frame
        keep = torch.arange(ppf, dtype=torch.int32, device=dev).repeat(B, tubes, 1).contiguous()
        self._fresh_shadows()
        feat, _ = self.engine.encode_video(v, keep, B, tubes, project=False, view=table)
        return self._head(feat.clone())
