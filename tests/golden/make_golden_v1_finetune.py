#!/usr/bin/env python3
"""Generate tests/golden/v1_finetune.npz by RUNNING THE REFERENCE's downstream class and optimizer factory (build container only).

/root/reference/v1/downstream/video_encoder.py and optim_factory.py are imported read-only under the import shims of
make_golden_v1_downstream.py (timm is not installed here; optim_factory's timm.optim imports are stubbed with placeholders it
never touches on the adamw path).  The ``DropPath`` stub multiplies by a given per-sample scale table instead of drawing, so that
the run's masks are the ones tests/v1_finetune_ref.draw_table derives from the stored seed.  No reference file is edited or
copied: weights, clips and targets are regenerated from seeds (tests/v1_downstream_synth.py, tests/v1_finetune_ref.py), and only
seeds, names and RESULTS are stored.  optim_factory.get_parameter_groups returns the groups without their names (it prints
them): the names are read from what it prints.

Two steps as engine_for_finetuning.py runs them: SoftTargetCrossEntropy (restated in one line: timm is absent),
clip_grad_norm_, torch.optim.AdamW over the layer-decay groups with lr * lr_scale per group.

    python tests/golden/make_golden_v1_finetune.py
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TVTS_REFERENCE_V1", "/root/reference/v1")
sys.path.insert(0, ROOT)

from tests import v1_downstream_synth as S  # noqa: E402
from tests import v1_finetune_ref as R  # noqa: E402
from tests.golden.make_golden_v1 import _load, _stub, save  # noqa: E402


class TableDropPath(torch.nn.Module):
    """stands in for timm's DropPath: x * scale[sample], the scale rows handed over per forward (attention branch, then MLP)"""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob, self.rows, self.calls = drop_prob, None, 0

    def forward(self, x):
        s = self.rows[self.calls % 2]
        self.calls += 1
        return x * s.to(x.dtype)[:, None, None]


def import_reference():
    _stub("timm"); _stub("timm.models")
    _stub("timm.models.layers", StdConv2dSame=object, DropPath=TableDropPath,
          to_2tuple=lambda x: x if isinstance(x, tuple) else (x, x), trunc_normal_=lambda t, std=1.0: t)
    _stub("timm.optim")
    for mod, cls in (("adafactor", "Adafactor"), ("adahessian", "Adahessian"), ("adamp", "AdamP"), ("lookahead", "Lookahead"),
                     ("nadam", "Nadam"), ("novograd", "NovoGrad"), ("nvnovograd", "NvNovoGrad"), ("radam", "RAdam"),
                     ("rmsprop_tf", "RMSpropTF"), ("sgdp", "SGDP")):
        _stub("timm.optim." + mod, **{cls: object})
    enc = _load("v1_downstream_video_encoder_ft", os.path.join(REF, "downstream/video_encoder.py"))
    fac = _load("v1_downstream_optim_factory", os.path.join(REF, "downstream/optim_factory.py"))
    return enc, fac


def groups_of(fac, model, weight_decay, layer_decay, depth):
    assigner = fac.LayerDecayValueAssigner(list(layer_decay ** (depth + 1 - i) for i in range(depth + 2)))  # run_class_finetuning.py:372-374
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        groups = fac.get_parameter_groups(model, weight_decay, model.no_weight_decay(), assigner.get_layer_id, assigner.get_scale)
    named = json.loads(buf.getvalue().split("Param groups = ", 1)[1])
    assert len(named) == len(groups)
    for (name, ng), g in zip(named.items(), groups):
        assert len(ng["params"]) == len(g["params"]) and ng["lr_scale"] == g["lr_scale"]
        g["name"], g["param_names"] = name, ng["params"]
    return groups


def flat_groups(groups):
    return dict(names=np.array([g["name"] for g in groups]), scales=np.array([g["lr_scale"] for g in groups], dtype=np.float64),
                wds=np.array([g["weight_decay"] for g in groups], dtype=np.float64),
                members=np.array([n for g in groups for n in g["param_names"]]),
                member_group=np.array([i for i, g in enumerate(groups) for _ in g["param_names"]], dtype=np.int32))


def main():
    torch.manual_seed(0)
    enc, fac = import_reference()
    F, kw = R.FX, S.TINY
    B, C, depth = F["B"], F["classes"], kw["depth"]
    model = enc.VisionTransformer(num_classes=C, drop_path_rate=F["drop_path_rate"], **kw).train()
    sd = R.state(kw, F["seed"], C)
    model.load_state_dict(sd, strict=True)
    clip, targets = S.synth_clip(kw, B, F["T"], F["clip_seed"]), R.soft_targets(B, C, F["target_seed"])
    rates = R.site_rates(F["drop_path_rate"], depth)
    tables = [torch.from_numpy(R.draw_table(R.step_seed(F["drop_seed"], k + 1), rates, B)) for k in range(F["steps"])]
    t1 = tables[0][2:]
    assert (t1 == 0).any() and (t1 > 1).any(), "block 1 must hold a dropped and a kept sample: choose another drop_seed"

    groups = groups_of(fac, model, F["weight_decay"], F["layer_decay"], depth)
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.head.parameters():          # run_class_linear.py:342-346
        p.requires_grad_(True)
    head_groups = groups_of(fac, model, F["weight_decay"], F["layer_decay"], depth)
    for p in model.parameters():
        p.requires_grad_(True)
    opt = torch.optim.AdamW([{k: v for k, v in g.items() if k in ("params", "weight_decay", "lr_scale")} for g in groups],
                            lr=F["lr"], betas=(0.9, 0.999), eps=1e-8)           # optim_factory.py:110,129-130
    names = [n for n, _ in model.named_parameters()]
    out = dict(logits=[], loss=[], grad_norm=[], tensor_grad_norms=[])
    clip_grad = None
    for k in range(F["steps"]):
        for g in opt.param_groups:            # engine_for_finetuning.py:48-53 (a constant schedule)
            g["lr"] = F["lr"] * g["lr_scale"]
        for l, blk in enumerate(model.blocks):
            if isinstance(blk.drop_path, TableDropPath):
                blk.drop_path.rows, blk.drop_path.calls = (tables[k][2 * l], tables[k][2 * l + 1]), 0
            else:                             # rate 0: nn.Identity (video_encoder.py:65)
                assert float(tables[k][2 * l:2 * l + 2].min()) == float(tables[k][2 * l:2 * l + 2].max()) == 1.0
        opt.zero_grad()
        logits = model(clip)
        loss = torch.sum(-targets * torch.nn.functional.log_softmax(logits, dim=-1), dim=-1).mean()  # timm SoftTargetCrossEntropy
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        if clip_grad is None:                 # below the first step's norm, so that clipping binds
            clip_grad = round(0.5 * float(torch.cat([g.flatten() for g in grads.values()]).norm()), 3)
        gn = torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad)  # utils.py:366
        if k == 0:
            assert float(gn) > clip_grad
            out["full"] = {n: grads[n] for n in R.FULL_GRADS}
        out["logits"].append(logits.detach().clone())
        out["loss"].append(float(loss))
        out["grad_norm"].append(float(gn))
        out["tensor_grad_norms"].append([float(grads[n].double().norm()) for n in names])
        opt.step()
    after = dict(model.named_parameters())
    # (delta_for_compare: without the key third of attn.qkv.bias, whose gradient is identically zero in exact arithmetic)
    delta = [float(R.delta_for_compare(n, after[n].detach().double() - sd[n].double()).norm()) for n in names]
    ga, gh = flat_groups(groups), flat_groups(head_groups)
    save("v1_finetune", seed=F["seed"], clip_seed=F["clip_seed"], target_seed=F["target_seed"], drop_seed=np.uint64(F["drop_seed"]),
         tables=torch.stack(tables), clip_grad=clip_grad, param_names=np.array(names),
         logits=torch.stack(out["logits"]), loss=np.array(out["loss"]), grad_norm=np.array(out["grad_norm"]),
         tensor_grad_norms=np.array(out["tensor_grad_norms"]), delta_norms=np.array(delta),
         **{"all_" + k: v for k, v in ga.items()}, **{"head_" + k: v for k, v in gh.items()},
         **{"grad." + n: g for n, g in out["full"].items()})


if __name__ == "__main__":
    main()
