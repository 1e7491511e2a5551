"""Fused multi-tensor optimizers over the flat parameter store: ``step()`` is ONE kernel launch over the flat buffers.

``_FlatOptimizer`` holds what all of them share (chunk table, lr / weight_decay device table, step counters, ``_begin`` /
``_begin_guard`` / ``_finish``, ``norm_coef``, the shadow refresh); ``_FlatAdamW`` adds what the two AdamWs share (moments, state views,
checkpoints), ``_TorchRule`` what the two torch rules share (``ema``, the body of ``step(closure, device_step, guard)``).

``FusedHFAdamW`` replaces ``transformers.AdamW(params=optimizer_grouped_parameters)`` built at
v2/train_dist_TVTSv2_ViT_B_16.py:118-125 (defaults betas (0.9, 0.999), eps 1e-6, correct_bias=True).
``FusedTorchAdamW`` is ``torch.optim.AdamW`` (eps 1e-8) for the v1 fine-tuning step (downstream/finetune_v1.py).
``FusedTorchSGD`` is ``torch.optim.SGD`` (momentum, Nesterov) for the v1 linear probe (v1/scripts/linear_ssv2.sh), bit for bit.
All are ``torch.optim.Optimizer``s, so param_groups / state_dict keep the reference checkpoint layout
(AdamW: ``state[p] = {step, exp_avg, exp_avg_sq}``, SGD: ``state[p] = {momentum_buffer}``; views of the flat state buffers).

``FusedTorchAdamW.step(guard=True)`` / ``FusedTorchSGD.step(guard=True)`` are the same launches under the overflow guard
(tvts_adamw_torch / tvts_sgd_torch with ``skipped``): the kernel updates only when ``norm_coef[0]`` is finite, the step counter the
kernels read lives on the device and advances there, ``skipped`` (device int64) counts the calls that did not update, and
``state_dict()`` reports the device's step count.  ``FusedHFAdamW.step(guard=True)`` is the same for the pretraining step
(tvts_adamw_hf_guarded; StepRunner(skip_nonfinite=True)), and with ``norm_coef`` set its launch multiplies the gradient by the clip
coefficient (StepRunner(clip_grad=...)).

Gradient handling follows the reference's pinned torch 1.11 ``zero_grad()`` (grads zeroed, not set to
None): every trainable tensor is updated every step, tensors that received no gradient see g = 0.
"""
from __future__ import annotations

import torch

from . import hip as K
from .engine import CH, ParamStore


class _FlatOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: the 1024-element chunk table (group per chunk, 255 = frozen), the lr / weight_decay device
    table and the host / device step counters.  A subclass sets MAX_GROUPS (the width of its kernel's table), allocates its state
    on the ParamStore (_alloc_state, _init_param), names its per-launch constants (_hyper) and launches its kernel in step()."""
    MAX_GROUPS = 0
    norm_coef = None  # set by the step that clips / guards: device fp32 [norm, clip coefficient] as tvts_grad_sumsq leaves them
    _NORM_OWNER = "StepRunner(clip_grad / skip_nonfinite)"  # who sets norm_coef, for the message of a guarded step without one

    def __init__(self, params, defaults, store: ParamStore, model=None):
        super().__init__(params, defaults)
        self._cls = type(self).__name__
        if len(self.param_groups) > self.MAX_GROUPS:
            raise ValueError(f"the fused kernel supports up to {self.MAX_GROUPS} parameter groups")
        self.store, self.model = store, model
        dev = store.device
        self._alloc_state()
        ptr2name = {store.p(n).data_ptr(): n for n in store.shapes}
        table = torch.full((store.total // CH,), 255, dtype=torch.uint8)
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                name = ptr2name.get(p.data_ptr())
                if name is None:
                    raise ValueError(f"{self._cls} only handles parameters of the flat store")
                o, n = store.off[name], p.numel()
                table[o // CH:(o + n + CH - 1) // CH] = gi
                self._init_param(p, o, n)
        self.chunk_group = table.to(dev)
        self.global_step = 0
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int64, device=dev)  # updates the overflow guard skipped (step(guard=True))
        self._guarded = False  # a guarded step has run since the host last read step_dev: global_step may lag behind it
        self.hyper_dev = torch.zeros(2 * self.MAX_GROUPS, dtype=torch.float32, device=dev)  # lr[MAX_GROUPS] | wd[MAX_GROUPS]
        self._hyper_host = None
        self.grad_scale = 1.0

    def _alloc_state(self):
        """the flat state buffers this optimizer keeps on the store"""
        raise NotImplementedError

    def _init_param(self, p, o, n):
        """state[p] of the parameter at elements [o, o + n) of the flat store"""
        raise NotImplementedError

    def _hyper(self):
        """-> (the per-launch constants ..., lr per group, weight_decay per group), both lists padded to MAX_GROUPS"""
        raise NotImplementedError

    def _lr_wd(self):
        pad = [0.0] * (self.MAX_GROUPS - len(self.param_groups))
        return [float(g["lr"]) for g in self.param_groups] + pad, [float(g["weight_decay"]) for g in self.param_groups] + pad

    def sync_hyper(self):
        """Upload lr / weight_decay of the parameter groups to the device table.  When a captured hipGraph is REPLAYED, call it
        after changing param_groups (an LR schedule) -- the replay then uses the new values without re-capture.  The copy is
        skipped when nothing changed."""
        *_, lr, wd = self._hyper()
        if self._hyper_host != (lr, wd):
            self.hyper_dev.copy_(torch.tensor(lr + wd, dtype=torch.float32), non_blocking=False)
            self._hyper_host = (lr, wd)

    def zero_grad(self, set_to_none: bool = False):
        K.zero_(self.store.grad)

    def _begin(self, device_step: bool):
        """counters of a new optimizer step (once per step, in front of its first launch) -> _hyper()"""
        hp = self._hyper()
        lr, wd = hp[-2:]
        capturing = torch.cuda.is_current_stream_capturing()
        if device_step and not capturing:
            self.sync_hyper()  # (a host -> device copy: not capturable; the caller syncs before capture / replay)
        elif device_step and self._hyper_host != (lr, wd):
            raise RuntimeError(f"{self._cls}: call sync_hyper() (or run one eager device_step) before capturing the step")
        if self._guarded:  # (guarded steps count on the device only: the host counter catches up before it is used again)
            self._adopt_device_step()
        self.global_step += 1
        if device_step:
            self.step_dev.add_(1)
        else:
            self.step_dev.fill_(self.global_step)  # keeps the device counter in step when eager and captured steps mix
        return hp

    def _begin_guard(self):
        """a step under the overflow guard (step(guard=True)) -> _hyper().  The kernels decide on the device whether the step
        counts: the launch itself advances step_dev or skipped, and the host counter is re-read from step_dev when somebody needs it
        (state_dict, the next unguarded step) -- nothing here synchronises."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._cls}: step(guard=True) inside a stream capture is not built")
        if self.norm_coef is None:
            raise RuntimeError(f"{self._cls}: step(guard=True) needs norm_coef (the device norm of tvts_grad_sumsq; {self._NORM_OWNER} sets it)")
        hp = self._hyper()
        self.sync_hyper()
        self._guarded = True
        return hp

    def _adopt_device_step(self):
        """the host counter takes the device's value (a host read): behind guarded steps the device alone knows how many counted"""
        self.global_step = int(self.step_dev.item())
        self._guarded = False

    def _finish(self, device_step: bool, transposed: bool = True):
        """behind the step's last launch: the shadows the kernel does not write"""
        self.store.refresh_shadows(cast=False, transposed=transposed)
        if self.model is not None:
            self.model.mark_shadows_fresh()


class _FlatAdamW(_FlatOptimizer):
    """What the fused AdamWs share: the moments on the ParamStore, the ``state[p]`` views with their step fields, checkpoints."""

    def _alloc_state(self):
        store = self.store
        if store.m is None:
            store.m = torch.zeros_like(store.flat)
        if store.v is None:
            store.v = torch.zeros_like(store.flat)

    def _init_param(self, p, o, n):
        store = self.store
        self.state[p] = dict(step=0, exp_avg=store.m[o:o + n].view(p.shape), exp_avg_sq=store.v[o:o + n].view(p.shape))

    def _hyper(self):
        b1, b2 = self.param_groups[0]["betas"]
        eps = self.param_groups[0]["eps"]
        for g in self.param_groups[1:]:  # one kernel launch covers every group: these three cannot differ per group
            if tuple(g["betas"]) != (b1, b2) or g["eps"] != eps:
                raise ValueError(f"{self._cls} needs the same betas / eps in every parameter group (lr and weight_decay may differ)")
        return (b1, b2, eps, *self._lr_wd())

    def _sync_step_from_device(self):
        """Under hipGraph replay the host counters only advance at capture time: re-read the device counter."""
        st = int(self.step_dev.item())
        if st > self.global_step or self._guarded:
            self.global_step, self._guarded = st, False
        for s in self.state.values():
            s["step"] = self.global_step

    def state_dict(self):
        self._sync_step_from_device()
        return super().state_dict()

    def _finish(self, device_step: bool, transposed: bool = True):
        """the shadows, and the per-parameter step fields"""
        super()._finish(device_step, transposed)
        if not device_step:
            for st in self.state.values():
                st["step"] = self.global_step

    def load_state_dict(self, state_dict):
        """Accepts the HF-AdamW / torch layout: state keyed by the running parameter index."""
        sd_groups, sd_state = state_dict["param_groups"], state_dict["state"]
        for g, sg in zip(self.param_groups, sd_groups):
            for k, v in sg.items():
                if k != "params":
                    g[k] = v
            for p, idx in zip(g["params"], sg["params"]):
                st = sd_state.get(idx)
                if st is None:
                    continue
                self.state[p]["exp_avg"].copy_(st["exp_avg"])
                self.state[p]["exp_avg_sq"].copy_(st["exp_avg_sq"])
                self.state[p]["step"] = int(st["step"])
                self.global_step = max(self.global_step, int(st["step"]))
        self.step_dev.fill_(self.global_step)
        self._guarded = False


class FusedHFAdamW(_FlatAdamW):
    """``transformers.AdamW`` arithmetic for up to 4 parameter groups (the reference uses 4).  The device table is lr[4] | wd[4];
    the kernel reads it only together with the device step counter (captured launches)."""
    MAX_GROUPS = 4

    def __init__(self, params, store: ParamStore, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0,
                 correct_bias=True, model=None):
        if not correct_bias:
            raise NotImplementedError("correct_bias=False is not built")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias), store, model)
        self._ranged = None      # (hyper-parameters, device_step, [chunk ranges done]) between begin_ranges() and step()
        self._opt_stream = None

    def _launch(self, lo: int, hi: int, hp, device_step: bool):
        """the update of the chunks [lo, hi) of the flat buffers + the transposed shadows of the weights inside them"""
        b1, b2, eps, lr4, wd4 = hp
        st = self.store
        s, e = lo * CH, hi * CH
        K.adamw_hf(st.flat[s:e], st.grad[s:e], st.m[s:e], st.v[s:e], st.shadow[s:e], self.chunk_group[lo:hi],
                   lr4, wd4, self.global_step, b1, b2, eps, self.grad_scale, step_dev=self.step_dev if device_step else None,
                   hyper_dev=self.hyper_dev if device_step else None)
        st.refresh_transposed(s, e)

    @torch.no_grad()
    def step(self, closure=None, device_step: bool = False, guard: bool = False):
        """device_step=True keeps the step counter in device memory (hipGraph replay).  After begin_ranges() / step_range() calls
        this finishes the step: the chunks no range has covered yet.  With ``norm_coef`` set (StepRunner(clip_grad=...)) the launch
        is tvts_adamw_hf_guarded, which multiplies every gradient by the clip coefficient norm_coef[1]; guard=True
        (StepRunner(skip_nonfinite=True)) runs it under the overflow guard: the update happens only when norm_coef[0] is finite,
        decided on the device, and a skipped call advances ``skipped`` instead of the device step counter."""
        nch = self.chunk_group.numel()
        st = self.store
        if guard:
            if self._ranged is not None:
                raise RuntimeError(f"{self._cls}: step(guard=True) cannot finish a ranged update (begin_ranges / step_range)")
            hp = self._begin_guard()
            K.adamw_hf_guarded(st.flat, st.grad, st.m, st.v, st.shadow, self.chunk_group, hp[3], hp[4], 0, hp[0], hp[1], hp[2],
                               self.grad_scale, step_dev=self.step_dev, hyper_dev=self.hyper_dev, norm_coef=self.norm_coef,
                               skipped=self.skipped)
            self._finish(True)
        elif self._ranged is None:
            hp = self._begin(device_step)
            dev = dict(step_dev=self.step_dev if device_step else None, hyper_dev=self.hyper_dev if device_step else None)
            if self.norm_coef is not None:
                K.adamw_hf_guarded(st.flat, st.grad, st.m, st.v, st.shadow, self.chunk_group, hp[3], hp[4], self.global_step, hp[0], hp[1],
                                   hp[2], self.grad_scale, norm_coef=self.norm_coef, **dev)
            else:
                K.adamw_hf(st.flat, st.grad, st.m, st.v, st.shadow, self.chunk_group, hp[3], hp[4], self.global_step, hp[0], hp[1], hp[2],
                           self.grad_scale, **dev)
            self._finish(device_step)
        else:
            hp, dstep, done = self._ranged
            self._ranged = None
            cur = torch.cuda.current_stream(self.store.device)
            if self._opt_stream is not None and done:
                cur.wait_stream(self._opt_stream)  # every range launched beside the backward has landed
            pos = 0
            for lo, hi in sorted(done) + [(nch, nch)]:
                if lo > pos:
                    self._launch(pos, lo, hp, dstep)
                pos = max(pos, hi)
            self._finish(device_step, transposed=False)  # what is not per-range: K-padded conv weight, e4m3 copies

    # ---- the update range by range, beside the backward (round 5).  The hand-written backward reports every parameter range whose
    # gradient is final (Engine._ready -> param_ready); its update -- HBM-bound, 30 B per parameter -- then runs on a stream of its
    # own under the remaining backward instead of behind it: the layer's weights are not read again before the next forward.
    # begin_ranges() once per step in front of the backward, step_range(lo, hi) per finished range (elements of the flat buffers,
    # chunk-aligned as Engine.trainable_runs hands them out), step() afterwards for whatever no range covered.
    def begin_ranges(self, device_step: bool = False, guard: bool = False):
        if self.norm_coef is not None or guard:
            # a range's update starts before the last gradient exists: neither the global norm nor the guard's decision is known then
            raise RuntimeError(f"{self._cls}: ranged updates (begin_ranges / step_range) cannot be combined with "
                               f"{'the overflow guard' if guard else 'gradient clipping (norm_coef)'}: the global gradient norm exists "
                               "only behind the whole backward")
        self._ranged = (self._begin(device_step), device_step, [])

    def step_range(self, lo_elem: int, hi_elem: int, wait=None):
        """wait: callable run on the optimizer stream in front of the launch (the range's all-reduce completing)"""
        if self._ranged is None:
            raise RuntimeError("FusedHFAdamW.step_range outside begin_ranges() ... step()")
        hp, dstep, done = self._ranged
        lo, hi = lo_elem // CH, -(-hi_elem // CH)
        if self._opt_stream is None:
            self._opt_stream = torch.cuda.Stream(device=self.store.device)
        self._opt_stream.wait_stream(torch.cuda.current_stream(self.store.device))
        with torch.cuda.stream(self._opt_stream), K.lane(2):
            if wait is not None:
                wait()
            self._launch(lo, hi, hp, dstep)
        done.append((lo, hi))


class _TorchRule:
    """What the two torch rules (the v1 downstream steps) add to _FlatOptimizer: up to 64 parameter groups whose lr / weight_decay
    travel as the device table lr[64] | wd[64], which the kernel always reads (step() uploads it on every call), and the optional
    parts of the launch.  ``norm_coef`` (the base class's; set by FinetuneStep): the device buffer whose second element scales every
    gradient -- the clip coefficient of tvts_grad_sumsq.  ``ema`` (set by FinetuneStep from its ModelEma): (fp32 buffer with the flat store's
    layout, decay) -- the launch then also carries the averaged weights; None: the launch without an average.  A subclass names
    its buffers and its kernel in ``_launch(hp, step, **kw)``; kw is what the two kernels' wrappers have in common."""
    MAX_GROUPS = 64
    ema = None
    _NORM_OWNER = "FinetuneStep"

    @torch.no_grad()
    def step(self, closure=None, device_step: bool = False, guard: bool = False):
        """device_step=True: the step counter the kernel reads lives in device memory (same bits as the host counter).
        guard=True (FinetuneStep(skip_nonfinite=True)): the update happens only when norm_coef[0] is finite, decided on the device;
        a skipped call advances ``skipped`` instead of the device step counter."""
        kw = dict(grad_scale=self.grad_scale, norm_coef=self.norm_coef)
        if self.ema is not None:
            kw.update(ema=self.ema[0], ema_decay=self.ema[1])
        if guard:
            self._launch(self._begin_guard(), 0, step_dev=self.step_dev, skipped=self.skipped, **kw)
        else:
            self.sync_hyper()
            self._launch(self._begin(device_step), self.global_step, step_dev=self.step_dev if device_step else None, **kw)
        self._finish(guard or device_step)


class FusedTorchAdamW(_TorchRule, _FlatAdamW):
    """``torch.optim.AdamW`` arithmetic (decay first, p *= 1 - lr wd; bias corrections bc1 = 1 - b1^t, bc2 = 1 - b2^t;
    p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)) as ONE launch over the flat store (tvts_adamw_torch) -- the 28 layer-decay
    groups of ViT-B (v1 fine-tuning, downstream/finetune_v1.py)."""

    def __init__(self, params, store: ParamStore, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, model=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), store, model)

    def _launch(self, hp, step, **kw):
        st = self.store
        K.adamw_torch(st.flat, st.grad, st.m, st.v, st.shadow, self.chunk_group, self.hyper_dev, step, *hp[:3], **kw)


class FusedTorchSGD(_TorchRule, _FlatOptimizer):
    """``torch.optim.SGD`` (single-tensor form, dampening 0) as ONE launch over the flat store, bit for bit, for up to 64 parameter
    groups: the optimizer optim_factory.create_optimizer builds for ``sgd`` / ``nesterov`` (nesterov=True) and ``momentum``
    (optim_factory.py:121-126) -- v1/scripts/linear_ssv2.sh trains the probe with ``--opt sgd --lr 0.1 --momentum 0.9
    --weight_decay 1e-9``.  Constructor as torch's; refused: dampening != 0, maximize, foreach=True, fused=True, differentiable,
    and nesterov without momentum (torch refuses that too).  lr / weight_decay travel per group in the device table lr[64] |
    wd[64]; momentum / nesterov / dampening are one value per launch and must agree across the groups.  The momentum buffer is
    ``store.m`` (no ``store.v``; with momentum 0 no state at all), ``state[p] = {"momentum_buffer": view of store.m}`` once the
    first update has run, as torch fills it.  The first update (buf = d, the bits of d) is decided for the whole store by the step
    counter: under this project's zero-gradient convention every trainable tensor is updated every step, so torch's per-parameter
    ``buf is None`` is the same rule.  ``norm_coef`` / ``ema`` / ``grad_scale`` as FusedTorchAdamW."""

    def __init__(self, params, store: ParamStore, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *,
                 maximize=False, foreach=None, differentiable=False, fused=None, model=None):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"FusedTorchSGD: lr {lr}, momentum {momentum} and weight_decay {weight_decay} must not be negative")
        for what, bad in (("dampening != 0", dampening != 0), ("maximize=True", bool(maximize)), ("foreach=True", bool(foreach)),
                          ("fused=True", bool(fused)), ("differentiable=True", bool(differentiable))):
            if bad:
                raise NotImplementedError(f"FusedTorchSGD({what}) is not built")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        super().__init__(params, defaults, store, model)
        self._hyper()

    def _alloc_state(self):
        if self.defaults["momentum"] != 0 and self.store.m is None:
            self.store.m = torch.zeros_like(self.store.flat)

    def _init_param(self, p, o, n):
        pass  # (torch.optim.SGD has no state in front of its first update)

    def _buffers(self):
        """state[p] = {"momentum_buffer": view of store.m} for every parameter, as torch holds it behind an update"""
        st = self.store
        if self.defaults["momentum"] == 0 or len(self.state):
            return
        ptr2name = {st.p(n).data_ptr(): n for n in st.shapes}
        for group in self.param_groups:
            for p in group["params"]:
                o = st.off[ptr2name[p.data_ptr()]]
                self.state[p] = dict(momentum_buffer=st.m[o:o + p.numel()].view(p.shape))

    def _hyper(self):
        g0 = self.param_groups[0]
        mu, nes = float(g0["momentum"]), bool(g0["nesterov"])
        for g in self.param_groups:  # one kernel launch covers every group: these cannot differ per group
            if float(g["momentum"]) != mu or bool(g["nesterov"]) != nes:
                raise ValueError(f"{self._cls} needs the same momentum / nesterov in every parameter group (lr and weight_decay may differ)")
            if g["dampening"] != 0 or g["maximize"] or g["foreach"] or g["fused"] or g["differentiable"]:
                raise NotImplementedError(f"{self._cls}: dampening / maximize / foreach / fused / differentiable are not built")
        if (mu != 0) != (self.defaults["momentum"] != 0):
            raise ValueError(f"{self._cls}: momentum cannot be switched on or off after construction (the buffer is allocated there)")
        if nes and mu <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        return (mu, nes, *self._lr_wd())

    def _launch(self, hp, step, **kw):
        """Behind a guarded launch ``state[p]`` is filled by state_dict(), which reads the device counter: whether a first update
        has happened is then the device's knowledge."""
        st = self.store
        K.sgd_torch(st.flat, st.grad, st.m if hp[0] != 0 else None, st.shadow, self.chunk_group, self.hyper_dev, step,
                    momentum=hp[0], nesterov=hp[1], **kw)
        if kw.get("skipped") is None:
            self._buffers()

    def state_dict(self):
        st = int(self.step_dev.item())  # (under hipGraph replay the host counter only advances at capture time)
        if st > self.global_step or self._guarded:
            self.global_step, self._guarded = st, False
        if self.global_step > 0:
            self._buffers()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Accepts torch.optim.SGD's layout, state keyed by the running parameter index.  Buffers present: the next update is not
        a first one; an empty state: it is.  Some parameters with and some without a buffer: ValueError (the first-update rule
        is one decision for the whole store)."""
        sd_groups, sd_state = state_dict["param_groups"], state_dict["state"]
        if len(sd_groups) != len(self.param_groups) or any(len(g["params"]) != len(sg["params"])
                                                           for g, sg in zip(self.param_groups, sd_groups)):
            raise ValueError("loaded state dict has other parameter groups than this optimizer")
        pairs = [(p, sd_state.get(idx)) for g, sg in zip(self.param_groups, sd_groups) for p, idx in zip(g["params"], sg["params"])]
        have = [s is not None and s.get("momentum_buffer") is not None for _, s in pairs]
        if any(have) and not all(have):
            raise ValueError(f"{self._cls}.load_state_dict: {sum(have)} of {len(have)} parameters carry a momentum_buffer; all or none")
        kept = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        for g, sg in zip(self.param_groups, sd_groups):
            for k, v in sg.items():
                if k != "params":
                    g[k] = v
        try:
            mu = self._hyper()[0]
            if any(have) and mu == 0:
                raise ValueError(f"{self._cls}.load_state_dict: momentum buffers for an optimizer with momentum 0")
        except Exception:
            for g, k in zip(self.param_groups, kept):
                g.update(k)
            raise
        if any(have):
            self.state.clear()
            self._buffers()
            for p, s in pairs:
                self.state[p]["momentum_buffer"].copy_(s["momentum_buffer"])
            self.global_step = max(self.global_step, 1)
        else:
            self.state.clear()
            self.global_step = 0
        self.step_dev.fill_(self.global_step)
        self._guarded = False
