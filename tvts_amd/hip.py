"""Thin tensor-level wrappers over the C ABI (include/tvts_hip.h).

PyTorch is used for device memory and the current HIP stream only; every function here launches a
hand-written gfx950 kernel.  Tensors must live on the GPU; a CPU tensor raises (no fallback).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import _lib

GEMM_PROFILE = None  # bench.py: list collecting (kind, flops, start_event, end_event) per MFMA GEMM launch
HBM_PROFILE = None   # bench.py: list collecting (family, algorithmic bytes, start_event, end_event) per HBM-bound launch


class _hbm:
    """Brackets one launch of an HBM-bound kernel family with HIP events on the launch stream while bench.py's instrumented step
    collects them (HBM_PROFILE is a list); free otherwise.  nbytes = the ALGORITHMIC bytes of the launch: every operand and result
    crossing HBM once."""

    def __init__(self, family, nbytes):
        self.family, self.nbytes = family, nbytes

    def __enter__(self):
        if HBM_PROFILE is not None:
            self.e0, self.e1 = Event(), Event()
            self.e0.record()

    def __exit__(self, *exc):
        if HBM_PROFILE is not None and exc[0] is None:
            self.e1.record()
            HBM_PROFILE.append((self.family, float(self.nbytes() if callable(self.nbytes) else self.nbytes), self.e0, self.e1))
        return False


def _nb(*tensors_rows):
    """bytes of (tensor, rows) pairs: rows x row width x element size (None entries are skipped)"""
    return sum(r * t.shape[-1] * t.element_size() for t, r in tensors_rows if t is not None)

ACT = {"none": 0, None: 0, "quick_gelu": 1, "gelu": 2, "add": 3}  # "add": gate slot only (bf16 residual added to the result)
MODE = {"full": 0, "space": 1, "time": 2, "cls": 3}


class HipError(RuntimeError):
    pass


def _chk(rc: int, name: str):
    if rc != 0:
        raise HipError(f"{name} failed with code {rc}")


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise HipError("tvts_amd kernels need GPU tensors (no CPU path)")
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "expected a row-major 2-D tensor"
    return t.stride(0)


# ---- per-call dispatch options.  The C library keeps no state: every alternative kernel path is selected by the `opts` word of
# the call (include/tvts_hip.h, TVTS_GEMM_* / TVTS_TN_* / TVTS_ATTN_*).  Tests and benches that want a whole engine step on an
# alternative path wrap it in `with hip.options(nt_tile=256): ...`; the defaults below are what every call uses otherwise.
# The one product use: `nt_cus` -- the CU reservation of the persistent GEMM grid when world > 1 (tvts_amd/dist.py).
_DEFAULTS = dict(nt_tile=0, nt_cus=0, nt_f32_patch=False, nt_streamk=None, tn_streamk=None, fp8_k32=False, tn_tile=0, tn_splits=0, tn_early_dma=None, tn_a_fast=None,
                 attn_tr=True, attn_shared=True, attn_fused=True, attn_ablate=0)
_OPTS = dict(_DEFAULTS)
if os.environ.get("TVTS_NT_F32_PATCH") == "1":  # A/B switch: the fp32 LDS patch of rounds 1 - 5 for the plain NT forms (same bits)
    _OPTS["nt_f32_patch"] = True


class options:
    """Context manager: dispatch options of every call made inside the block (restored on exit, also on an exception)."""

    def __init__(self, **kw):
        bad = set(kw) - set(_DEFAULTS)
        if bad:
            raise KeyError(f"unknown dispatch option(s) {sorted(bad)}")
        self.kw = kw

    def __enter__(self):
        self.saved = dict(_OPTS)
        _OPTS.update(self.kw)
        return self

    def __exit__(self, *exc):
        _OPTS.clear()
        _OPTS.update(self.saved)
        return False


def set_default(**kw):
    """Process-wide default of a dispatch option (Python side only; dist.py reserves CUs for the RCCL kernels with nt_cus)."""
    bad = set(kw) - set(_DEFAULTS)
    if bad:
        raise KeyError(f"unknown dispatch option(s) {sorted(bad)}")
    _OPTS.update(kw)


def _tile_bits(t):
    # "ring" (/ "ring2" "ring3" "ring4"): the one-block-per-CU ring form of the 128-column NT kernel (/ 128, 192, 256 tile rows), "noring": never take it
    return {0: 0, None: 0, 128: 1, 256: 2, "ring": 1 | 128, "ring2": 1 | 128 | (1 << 16), "ring3": 1 | 128 | (2 << 16), "ring4": 1 | 128 | (3 << 16), "noring": 16384,
            "128noring": 1 | 16384}[t]


def _sk_bits(sk):
    return 0 if sk is None else (32 if sk else 64)  # TVTS_GEMM_STREAMK / TVTS_GEMM_NO_STREAMK


def nt_opts(tile=None, cus=None, fp8_k32=None, streamk=None, side_deriv=False):
    tile = _OPTS["nt_tile"] if tile is None else tile
    cus = _OPTS["nt_cus"] if cus is None else cus
    k32 = _OPTS["fp8_k32"] if fp8_k32 is None else fp8_k32
    streamk = _OPTS["nt_streamk"] if streamk is None else streamk
    return (_tile_bits(tile) | (4 if k32 else 0) | (((int(cus) // 8) & 63) << 8) | _sk_bits(streamk) | ((1 << 20) if side_deriv else 0)
            | ((1 << 22) if _OPTS["nt_f32_patch"] else 0))   # TVTS_GEMM_F32_PATCH


def tn_opts(tile=None, splits=None, early_dma=None, a_fast=None, streamk=None):
    streamk = _OPTS["tn_streamk"] if streamk is None else streamk
    tile = _OPTS["tn_tile"] if tile is None else tile
    splits = _OPTS["tn_splits"] if splits is None else splits
    early_dma = _OPTS["tn_early_dma"] if early_dma is None else early_dma
    a_fast = _OPTS["tn_a_fast"] if a_fast is None else a_fast
    o = _tile_bits(tile) | (int(splits) << 8) | _sk_bits(streamk)
    if early_dma is not None and not early_dma:
        o |= 4
    if a_fast is not None:
        o |= 16 if a_fast else 8
    return o


def attn_opts(tr=None, shared=None, fused=None, ablate=None, q8_only=False):
    tr = _OPTS["attn_tr"] if tr is None else tr
    shared = _OPTS["attn_shared"] if shared is None else shared
    fused = _OPTS["attn_fused"] if fused is None else fused
    ablate = _OPTS["attn_ablate"] if ablate is None else ablate
    # bit 7: with a q8 copy, the fused divided kernels do not store the bf16 patch rows (the e4m3 bytes are their only output)
    return (0 if tr else 1) | (0 if shared else 2) | (0 if fused else 4) | ((int(ablate) & 7) << 4) | (128 if q8_only else 0)


def gemm_nt_select(M, N, tile=None):
    return _lib.load().tvts_gemm_nt_select(M, N, nt_opts(tile=tile))


def gemm_tn_select(M, Na, Nb, tile=None):
    return _lib.load().tvts_gemm_tn_select(M, Na, Nb, tn_opts(tile=tile))


STREAMK_TAKEN = [0]  # launches that took the stream-K walk / the fused reduce under a forcing option (tests assert the path ran)
NT_WORKSPACE = {}  # per (device, lane): scratch of the stream-K walk of gemm_nt (arrival counters + fp32 partial tiles)


def _nt_workspace(dev):
    """zeroed once: every launch leaves the arrival counters at zero again (include/tvts_hip.h)"""
    key = (dev, current_lane())
    ws = NT_WORKSPACE.get(key)
    if ws is None:
        ws = NT_WORKSPACE[key] = torch.zeros(_lib.load().tvts_gemm_nt_workspace_bytes(), dtype=torch.uint8, device=dev)
    return ws


def gemm_nt(a, b, out, *, M=None, bias=None, residual=None, act=None, preact=None, gate_h=None, gate_act=None, tile=None, cus=None,
            streamk=None, workspace=True, side_deriv=False):
    """out[M,N] = [act'(gate_h) *] act(a[M,K] @ b[N,K]^T + bias) [+ residual]; a, b bf16; out bf16 or fp32.
    streamk: None = the entry point's own choice, True / False force / forbid the stream-K walk (needs the workspace)."""
    lib = _lib.load()
    ws = _nt_workspace(a.device) if workspace else None
    M = a.shape[0] if M is None else M
    N, K = b.shape
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.shape[1] == K
    assert out.shape[1] == N and out.dtype in (torch.bfloat16, torch.float32)
    if residual is not None and residual.dtype == torch.bfloat16:  # the bf16 residual stream: the gate slot used additively
        assert gate_h is None and act is None
        gate_h, gate_act, residual = residual, "add", None
    if GEMM_PROFILE is not None:
        ev0, ev1 = Event(), Event()
        ev0.record()
    # the instrumented step of bench.py: plain bf16 launches of the 256 x 256 kernel sample the shader clock inside the kernel
    # (TVTS_GEMM_CLOCK_SAMPLE: 4 x u64 in the last 32 bytes of the workspace, copied to the probe buffer behind the launch)
    cp = CLOCK_PROBE
    sample = (cp is not None and ws is not None and cp["i"] < cp["buf"].shape[0] and out.dtype == torch.bfloat16
              and residual is None and act is None and gate_h is None and M >= 65536)
    if sample:
        zero_(ws[-32:])
    def launch(sk):
        return lib.tvts_gemm_nt_bf16(_p(a), _ld(a), _p(b), _ld(b), M, N, K, _p(bias), _p(residual),
                                     _ld(residual) if residual is not None else 0, ACT[act], _p(preact),
                                     _ld(preact) if preact is not None else 0, _p(gate_h),
                                     _ld(gate_h) if gate_h is not None else 0, ACT[gate_act], _p(out), _ld(out),
                                     1 if out.dtype == torch.float32 else 0, _p(ws), ws.numel() if ws is not None else 0,
                                     nt_opts(tile, cus, streamk=sk, side_deriv=side_deriv) | ((1 << 21) if sample else 0), _stream())
    want_sk = _OPTS["nt_streamk"] if streamk is None else streamk
    rc = launch(streamk)
    if rc == -22 and want_sk and streamk is None:  # the process-wide option means "wherever the shape can take it"
        rc = launch(False)
    elif rc == 0 and want_sk:
        STREAMK_TAKEN[0] += 1
    _chk(rc, "tvts_gemm_nt_bf16")
    if GEMM_PROFILE is not None:
        ev1.record()
        GEMM_PROFILE.append(("gemm_nt", 2.0 * M * N * K, ev0, ev1, (M, N, K, "f32" if out.dtype == torch.float32 else "bf16", "res" if residual is not None else "", str(act or ""), "gate" if gate_h is not None else "")))
    if sample:
        cp["buf"][cp["i"]].copy_(ws[-32:].view(torch.int64))
        cp["shape"].append((M, N, K))
        cp["i"] += 1


def quantize_fp8(x, q=None, scale=None, amax=None, amax_given=False):
    """per-tensor e4m3 quantisation of a bf16 / fp32 matrix -> (q uint8 [rows, cols], scale float32[1]); x ~ q * scale.
    q / scale / amax may be preallocated (the engine's workspace)."""
    lib = _lib.load()
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype in (torch.bfloat16, torch.float32)
    assert not (amax_given and amax is None)
    amax = torch.empty(1, dtype=torch.float32, device=x.device) if amax is None else amax
    scale = torch.empty(1, dtype=torch.float32, device=x.device) if scale is None else scale
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if q is None else q
    f32 = 1 if x.dtype == torch.float32 else 0
    if not amax_given:  # amax_given: `amax` already holds max |x| (values beyond it saturate at +-448)
        _chk(lib.tvts_amax(_p(x), f32, x.stride(0), x.shape[0], x.shape[1], _p(amax), _stream()), "tvts_amax")
    _chk(lib.tvts_quant_fp8(_p(x), f32, x.stride(0), x.shape[0], x.shape[1], _p(amax), _p(q), q.stride(0), _p(scale), _stream()),
         "tvts_quant_fp8")
    return q, scale


def quantize_fp8_multi_table(entries, device):
    """device table for quantize_fp8_multi.  entries: (w fp32 [rows, cols] contiguous, q uint8, wt bf16 [cols, rows] or None,
    qt uint8 or None, amax float32[1], scale float32[1], scale_t float32[1] or None)"""
    import numpy as np
    rec = np.zeros(len(entries), dtype=[("w", "<u8"), ("q", "<u8"), ("wt", "<u8"), ("qt", "<u8"), ("amax", "<u8"), ("scale", "<u8"),
                                        ("scale_t", "<u8"), ("rows", "<i4"), ("cols", "<i4")])
    for i, (w, q, wt, qt, am, sc, sct) in enumerate(entries):
        assert w.dtype == torch.float32 and w.is_contiguous() and q.is_contiguous() and w.numel() % 4 == 0
        assert wt is None or (wt.dtype == torch.bfloat16 and wt.is_contiguous() and qt.is_contiguous() and wt.numel() == w.numel())
        rows, cols = w.shape[0], w.numel() // w.shape[0]
        rec[i] = (w.data_ptr(), q.data_ptr(), 0 if wt is None else wt.data_ptr(), 0 if qt is None else qt.data_ptr(), am.data_ptr(),
                  sc.data_ptr(), 0 if sct is None else sct.data_ptr(), rows, cols)
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device), len(entries)


def quantize_fp8_multi(table, n):
    """per-tensor e4m3 copies of all the weights of the table (and of their transposed shadows) in three launches"""
    _chk(_lib.load().tvts_quant_fp8_multi(_p(table), n, _stream()), "tvts_quant_fp8_multi")


def quantize_fp8_rows(x, q=None, row_scale=None, tscale=None, amax=None):
    """per-row (per-token) e4m3 quantisation of a bf16 matrix in one pass -> (q uint8 [rows, cols], row_scale float32[rows]);
    x[r] ~ q[r] * row_scale[r].  tscale (float32[1], device): every row under THAT scale instead (per-tensor, delayed scaling;
    row_scale is then optional and returned as None when absent); amax (float32[1]): receives max(amax, max |x|)."""
    lib = _lib.load()
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.bfloat16
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if q is None else q
    if row_scale is None and tscale is None:
        row_scale = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    assert row_scale is None or (row_scale.numel() >= x.shape[0] and row_scale.dtype == torch.float32)
    with _hbm("quant_fp8_rows", _nb((x, x.shape[0]), (q, x.shape[0]))):
        rc = lib.tvts_quant_fp8_rows(_p(x), x.stride(0), x.shape[0], x.shape[1], _p(q), q.stride(0), _p(row_scale), _p(tscale), _p(amax),
                                     _stream())
    _chk(rc, "tvts_quant_fp8_rows")
    return q, row_scale


def fp8_update_scales(amax, scale):
    """scale[i] = amax[i] / 448 where amax[i] > 0, then amax[i] = 0: a step's running maxima become the next step's per-tensor scales"""
    assert amax.dtype == scale.dtype == torch.float32 and amax.numel() == scale.numel()
    _chk(_lib.load().tvts_fp8_update_scales(_p(amax), _p(scale), amax.numel(), _stream()), "tvts_fp8_update_scales")


def fp8_update_scales_guarded(amax, scale, guard_norm=None):
    """fp8_update_scales under the overflow guard: only a finite amax[i] > 0 becomes a scale, every other slot keeps its scale; a
    scale that is then not finite and positive becomes 1.0; amax[i] = 0.  guard_norm (device fp32, the global gradient norm): not
    finite -- the step the optimizer skips -- keeps every scale."""
    assert amax.dtype == scale.dtype == torch.float32 and amax.numel() == scale.numel()
    assert guard_norm is None or (guard_norm.dtype == torch.float32 and guard_norm.numel() >= 1)
    _chk(_lib.load().tvts_fp8_update_scales_guarded(_p(amax), _p(scale), amax.numel(), _p(guard_norm), _stream()),
         "tvts_fp8_update_scales_guarded")


def gemm_nt_fp8(a8, sa, b8, sb, out, *, bias=None, residual=None, act=None, preact=None, gate_h=None, gate_act=None, k32=None,
                cus=None, q8out=None, q8_scale=None, q8_amax=None, store_out=True, side_deriv=False):
    """out[M,N] = act(sa*sb * (a8[M,K] @ b8[N,K]^T) + bias) [+ residual]; a8 / b8 uint8 e4m3 bit patterns; sb float32[1]; sa
    float32[1] (one scale for the tensor) or float32[>= M] (one per row, quantize_fp8_rows); preact receives the bf16
    pre-activation like gemm_nt.  gate_h / gate_act: the input-gradient form, out = gate_act'(gate_h) * (sa*sb * (a8 @ b8^T)).
    k32: the 16x16x32 fp8 main loop instead of the K = 128 scaled MFMA (same products, same fp32 accumulation).
    store_out=False (with q8out): the bf16 result is not written, the e4m3 copy is the only output."""
    lib = _lib.load()
    assert store_out or q8out is not None
    po = _p(out) if store_out else None
    M, Kd = a8.shape
    N = b8.shape[0]
    assert a8.dtype == torch.uint8 and b8.dtype == torch.uint8 and b8.shape[1] == Kd
    sa_rows = 0 if sa.numel() == 1 else 1
    assert sa_rows == 0 or sa.numel() >= M
    if GEMM_PROFILE is not None:
        ev0, ev1 = Event(), Event()
        ev0.record()
    if residual is not None and residual.dtype == torch.bfloat16:
        assert gate_h is None and act is None and preact is None
        gate_h, gate_act, residual = residual, "add", None
    if gate_h is not None:
        assert residual is None and act is None and preact is None and out.dtype == torch.bfloat16
        assert bias is None or gate_act == "add"
        rc = lib.tvts_gemm_nt_fp8_gate(_p(a8), a8.stride(0), _p(b8), b8.stride(0), M, N, Kd, _p(sa), sa_rows, _p(sb), _p(bias), _p(gate_h),
                                       _ld(gate_h), ACT[gate_act], po, _ld(out), _p(q8out), q8out.stride(0) if q8out is not None else 0, _p(q8_scale),
                                       _p(q8_amax), nt_opts(None, cus, k32, side_deriv=side_deriv), _stream())
        _chk(rc, "tvts_gemm_nt_fp8_gate")
        if GEMM_PROFILE is not None:
            ev1.record()
            GEMM_PROFILE.append(("gemm_nt_fp8", 2.0 * M * N * Kd, ev0, ev1, (M, N, Kd, "fp8", "", "", "gate")))
        return
    rc = lib.tvts_gemm_nt_fp8(_p(a8), a8.stride(0), _p(b8), b8.stride(0), M, N, Kd, _p(sa), sa_rows, _p(sb), _p(bias), _p(residual),
                              _ld(residual) if residual is not None else 0, ACT[act], _p(preact),
                              _ld(preact) if preact is not None else 0, po, _ld(out),
                              1 if out.dtype == torch.float32 else 0, _p(q8out), q8out.stride(0) if q8out is not None else 0,
                              _p(q8_scale), _p(q8_amax), nt_opts(None, cus, k32, side_deriv=side_deriv), _stream())
    _chk(rc, "tvts_gemm_nt_fp8")
    if GEMM_PROFILE is not None:
        ev1.record()
        GEMM_PROFILE.append(("gemm_nt_fp8", 2.0 * M * N * Kd, ev0, ev1, (M, N, Kd, "fp8", "res" if residual is not None else "", str(act or ""), "")))


# Scratch LANES: the shared scratch buffers of this module (split partials of the weight gradients, LayerNorm dgamma / dbeta partials,
# stream-K workspace) belong to ONE stream's launch order.  A second stream that runs kernels beside it (the text tower next to the
# ViT, Engine.text_side) selects its own set with `with K.lane(1):` -- per host thread, like torch's current stream.
import threading

_LANE = threading.local()


def current_lane() -> int:
    return getattr(_LANE, "i", 0)


class lane:
    def __init__(self, i: int):
        self.i = int(i)

    def __enter__(self):
        self.prev = current_lane()
        _LANE.i = self.i

    def __exit__(self, *exc):
        _LANE.i = self.prev


TN_WORKSPACE = {}  # per (device, lane): fp32 scratch tensor for the split partials of gemm_tn (allocated lazily, 256 MiB: 8 partials of the largest weight, H/14 mlp 1280 x 5120)


def _tn_workspace(dev):
    key = (dev, current_lane())
    ws = TN_WORKSPACE.get(key)
    if ws is None:
        ws = TN_WORKSPACE[key] = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device=dev)  # (every lane the same size: the split plan depends on it)
    return ws


def warm_scratch(dev, lanes=(0, 1)):
    """allocate every lane's shared scratch NOW (Engine.__init__): a buffer that is first touched inside a hipGraph capture would live
    in that graph's private pool and die with it, while this module keeps handing it out"""
    for i in lanes:
        with lane(i):
            _tn_counters(_tn_workspace(dev))
            _ln_workspace(dev)
            _nt_workspace(dev)


TN_COUNTERS = {}  # per workspace: zeroed arrival counters of the fused reduce (every launch leaves them at zero again)


def _tn_counters(ws):
    c = TN_COUNTERS.get(ws.data_ptr())
    if c is None:
        c = TN_COUNTERS[ws.data_ptr()] = torch.zeros(4096, dtype=torch.int32, device=ws.device)
    return c


def gemm_tn(p, q, out, *, M=None, accumulate=True, colsum=None, workspace=True, tile=None, splits=None, early_dma=None, a_fast=None,
            fused=None):
    """out[Na,Nb] (+)= p[M,Na]^T @ q[M,Nb]; p, q bf16; out fp32.  fused: None = the entry point's choice, True / False force /
    forbid the in-kernel reduce of the split partials (the last block of a tile adds them) against the separate reduce pass."""
    lib = _lib.load()
    M = p.shape[0] if M is None else M
    assert p.dtype == torch.bfloat16 and q.dtype == torch.bfloat16 and out.dtype == torch.float32
    # workspace: True = this process's shared scratch (one stream), a float32 tensor = the caller's (a second stream's own), False = none
    ws = workspace if isinstance(workspace, torch.Tensor) else (_tn_workspace(p.device) if workspace else None)
    cnt = _tn_counters(ws) if ws is not None else None
    if GEMM_PROFILE is not None:
        ev0, ev1 = Event(), Event()
        ev0.record()
    def launch(fu):
        return lib.tvts_gemm_tn_bf16(_p(p), _ld(p), _p(q), _ld(q), M, p.shape[1], q.shape[1], _p(out), _ld(out),
                                     1 if accumulate else 0, _p(colsum), _p(ws), ws.numel() if ws is not None else 0,
                                     _p(cnt), cnt.numel() if cnt is not None else 0,
                                     tn_opts(tile, splits, early_dma, a_fast, fu), _stream())
    want_fu = _OPTS["tn_streamk"] if fused is None else fused
    rc = launch(fused)
    if rc == -22 and want_fu and fused is None:
        rc = launch(False)
    elif rc == 0 and want_fu:
        STREAMK_TAKEN[0] += 1
    _chk(rc, "tvts_gemm_tn_bf16")
    if GEMM_PROFILE is not None:
        ev1.record()
        GEMM_PROFILE.append(("gemm_tn", 2.0 * M * p.shape[1] * q.shape[1], ev0, ev1, (M, p.shape[1], q.shape[1], "cs" if colsum is not None else "")))


class TnGroup:
    """The weight gradients of one group (a ViT block's six) launched together: tvts_gemm_tn_bf16_grouped.  Build it once with the
    problems -- dicts of the gemm_tn arguments p, q, out, M, accumulate, colsum -- and call run(); the device plan is uploaded by the
    first run -- one asynchronous copy from page-locked staging memory ON THE LAUNCH STREAM, in front of the kernels that read it --
    and re-used while the problems stay the same tensors (the engine's buffers are persistent)."""

    class _Rec(ctypes.Structure):
        _fields_ = [("P", ctypes.c_void_p), ("ldp", ctypes.c_int), ("Q", ctypes.c_void_p), ("ldq", ctypes.c_int), ("M", ctypes.c_int),
                    ("Na", ctypes.c_int), ("Nb", ctypes.c_int), ("out", ctypes.c_void_p), ("ldo", ctypes.c_int),
                    ("accumulate", ctypes.c_int), ("colsum", ctypes.c_void_p)]

    def __init__(self, problems, workspace, splits=0):
        lib = _lib.load()
        self.n = len(problems)
        self.keep = problems  # the tensors stay alive with the plan
        self.recs = (self._Rec * self.n)()
        for r, pr in zip(self.recs, problems):
            p, q, out = pr["p"], pr["q"], pr["out"]
            assert p.dtype == torch.bfloat16 and q.dtype == torch.bfloat16 and out.dtype == torch.float32
            r.P, r.ldp, r.Q, r.ldq = p.data_ptr(), _ld(p), q.data_ptr(), _ld(q)
            r.M, r.Na, r.Nb = int(pr.get("M") or p.shape[0]), p.shape[1], q.shape[1]
            r.out, r.ldo, r.accumulate = out.data_ptr(), _ld(out), 1 if pr.get("accumulate", True) else 0
            r.colsum = pr["colsum"].data_ptr() if pr.get("colsum") is not None else None
        self.key = tuple((r.P, r.Q, r.out, r.colsum, r.M, r.Na, r.Nb, r.ldp, r.ldq, r.ldo, r.accumulate) for r in self.recs)
        self.ws = workspace
        nbytes = lib.tvts_gemm_tn_grouped_table_bytes(self.n)
        self.table = torch.empty(nbytes, dtype=torch.uint8, device=workspace.device)  # (no fill: a fill on another stream could land after the upload)
        self.table_host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)    # stays alive and untouched with the plan
        self.uploaded = False
        self.captured = False  # a hipGraph holds the addresses of table / table_host: the plan must outlive it (Engine never evicts it)
        self.opts = int(splits) << 8
        self.flops = sum(2.0 * r.M * r.Na * r.Nb for r in self.recs)

    def run(self):
        lib = _lib.load()
        if GEMM_PROFILE is not None:
            ev0, ev1 = Event(), Event()
            ev0.record()
        # An upload issued while the stream is being captured becomes a memcpy NODE of the graph: it runs at every replay, not now.  The
        # table then counts as uploaded for the replays only -- an eager run of the same plan (before or between replays) uploads again.
        capturing = torch.cuda.is_current_stream_capturing()
        rc = lib.tvts_gemm_tn_bf16_grouped(ctypes.cast(self.recs, ctypes.c_void_p), self.n, _p(self.table), ctypes.c_void_p(self.table_host.data_ptr()),
                                           self.table.numel(), 0 if (self.uploaded and not capturing) else 1, _p(self.ws), self.ws.numel(), self.opts, _stream())
        _chk(rc, "tvts_gemm_tn_bf16_grouped")
        if capturing:
            self.captured = True
        else:
            self.uploaded = True
        if GEMM_PROFILE is not None:
            ev1.record()
            r0 = self.recs[0]
            GEMM_PROFILE.append(("gemm_tn", self.flops, ev0, ev1, (r0.M, sum(r.Na * r.Nb for r in self.recs) // max(r0.Nb, 1), r0.Nb, "grouped")))


def gemm_tn_fp8(p8, sp, q8, sq, out, *, M=None, accumulate=True, colsum=None, workspace=True, splits=None):
    """out[Na,Nb] (+)= sp * sq * p8[M,Na]^T @ q8[M,Nb]; p8 / q8 uint8 e4m3 bytes under one scale per tensor (float32[1] each);
    colsum[a] += sp * sum_m p8[m,a] (the bias gradient from the same bytes)."""
    lib = _lib.load()
    M = p8.shape[0] if M is None else M
    assert p8.dtype == torch.uint8 and q8.dtype == torch.uint8 and out.dtype == torch.float32 and sp.numel() == 1 and sq.numel() == 1
    ws = workspace if isinstance(workspace, torch.Tensor) else (_tn_workspace(p8.device) if workspace else None)
    if GEMM_PROFILE is not None:
        ev0, ev1 = Event(), Event()
        ev0.record()
    rc = lib.tvts_gemm_tn_fp8(_p(p8), p8.stride(0), _p(q8), q8.stride(0), M, p8.shape[1], q8.shape[1], _p(sp), _p(sq), _p(out), _ld(out),
                              1 if accumulate else 0, _p(colsum), _p(ws), ws.numel() if ws is not None else 0, int(splits or 0) << 8, _stream())
    _chk(rc, "tvts_gemm_tn_fp8")
    if GEMM_PROFILE is not None:
        ev1.record()
        GEMM_PROFILE.append(("gemm_tn_fp8", 2.0 * M * p8.shape[1] * q8.shape[1], ev0, ev1, (M, p8.shape[1], q8.shape[1], "fp8")))


def gemm_small(a, b, out, *, M, N, K, sa, sb, alpha=1.0, bias=None, accumulate=False):
    """out[i,j] (+)= alpha * sum_k a[i*sa[0]+k*sa[1]] * b[k*sb[0]+j*sb[1]] + bias[j] (fp32)."""
    lib = _lib.load()
    assert a.dtype == b.dtype == out.dtype == torch.float32
    rc = lib.tvts_gemm_small_f32(_p(a), sa[0], sa[1], _p(b), sb[0], sb[1], M, N, K, alpha, _p(bias), _p(out),
                                 out.stride(0), 1 if accumulate else 0, _stream())
    _chk(rc, "tvts_gemm_small_f32")


def rows_linear(a, w, out, *, bias=None, residual=None):
    """out[R, N] (fp32) = residual + bias + a[R, K] @ w[N, K]^T for a FEW rows (a may be a strided row view: one row per clip)"""
    lib = _lib.load()
    assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and out.dtype == torch.float32 and a.stride(1) == 1
    R, Kd = a.shape
    N = w.shape[0]
    _chk(lib.tvts_rows_linear_bf16(_p(a), a.stride(0), _p(w), _ld(w), R, N, Kd, _p(bias), _p(residual),
                                   _ld(residual) if residual is not None else 0, _p(out), _ld(out), _stream()), "tvts_rows_linear_bf16")


def rows_linear_fp8(a8, row_scale, w8, w_scale, out, *, bias=None, residual=None):
    """out[R, N] (fp32) = residual + bias + row_scale[r] * w_scale * (a8[R, K] @ w8[N, K]^T) for a FEW rows on e4m3 operands: a8 uint8
    (a strided row view is fine: one row per clip) under one scale per row (quantize_fp8_rows), w8 / w_scale as in ParamStore.w8"""
    lib = _lib.load()
    assert a8.dtype == torch.uint8 and w8.dtype == torch.uint8 and out.dtype == torch.float32 and a8.stride(1) == 1
    R, Kd = a8.shape
    N = w8.shape[0]
    assert w8.shape[1] == Kd and tuple(out.shape) == (R, N) and (residual is None or tuple(residual.shape) == (R, N))
    assert row_scale.dtype == torch.float32 and row_scale.numel() >= R and w_scale.dtype == torch.float32 and (bias is None or bias.numel() == N)
    _chk(lib.tvts_rows_linear_fp8(_p(a8), a8.stride(0), _p(row_scale), _p(w8), _ld(w8), _p(w_scale), R, N, Kd, _p(bias), _p(residual),
                                  _ld(residual) if residual is not None else 0, _p(out), _ld(out), _stream()), "tvts_rows_linear_fp8")


def colsum(x, out, *, M=None):
    lib = _lib.load()
    M = x.shape[0] if M is None else M
    ws = _tn_workspace(x.device)
    _chk(lib.tvts_colsum_bf16(_p(x), _ld(x), M, x.shape[1], _p(out), _p(ws), ws.numel(), _stream()), "tvts_colsum_bf16")


def layernorm_fwd(x, gamma, beta, eps, y, mean=None, rstd=None, rows=None, M=None, q8=None, row_scale=None, tscale=None, amax=None,
                  cls_x=None, cls_period=0, refresh=True):
    """q8 (uint8 [M, W]) + row_scale (float32 [>= M]): also write the bf16 output as e4m3 bytes with one scale per row.
    y = None (with q8, bf16 x, W % 8 == 0, W <= 1536): the e4m3 bytes are the only output.
    cls_x (float32 [M / cls_period, W]) + cls_period: the hybrid residual stream -- x bf16, the rows r % cls_period == 0 are read
    from cls_x and (refresh) their bf16 rounding is written back into x."""
    lib = _lib.load()
    M = (rows.numel() if rows is not None else x.shape[0]) if M is None else M
    fam = "ln_fwd" if M >= 4096 else "ln_fwd_small"
    assert y is not None or q8 is not None
    ldy = _ld(y) if y is not None else 0
    if cls_x is not None:
        assert rows is None and x.dtype == torch.bfloat16 and (y is None or y.dtype == torch.bfloat16) and cls_x.dtype == torch.float32
        assert cls_x.is_contiguous() and cls_x.shape[1] == x.shape[1] and cls_x.shape[0] * cls_period == M
        with _hbm(fam, _nb((x, M), (y, M), (q8, M)) + 8 * M):
            rc = lib.tvts_layernorm_fwd_cls(_p(x), _ld(x), _p(cls_x), cls_period, _p(x) if refresh else None, _p(gamma), _p(beta), eps, M,
                                            x.shape[1], _p(y), ldy, _p(q8), q8.stride(0) if q8 is not None else 0, _p(row_scale), _p(tscale),
                                            _p(amax), _p(mean), _p(rstd), _stream())
        _chk(rc, "tvts_layernorm_fwd_cls")
        return
    if q8 is not None:
        assert (y is None or y.dtype == torch.bfloat16) and q8.dtype == torch.uint8 and (tscale is not None or (row_scale.dtype == torch.float32 and row_scale.numel() >= M))
        with _hbm(fam, _nb((x, M), (y, M), (q8, M)) + 12 * M):
            rc = lib.tvts_layernorm_fwd_fp8(_p(x), _ld(x), 1 if x.dtype == torch.bfloat16 else 0, _p(rows), _p(gamma), _p(beta), eps, M,
                                            x.shape[1], _p(y), ldy, _p(q8), q8.stride(0), _p(row_scale), _p(tscale), _p(amax), _p(mean), _p(rstd), _stream())
        _chk(rc, "tvts_layernorm_fwd_fp8")
        return
    with _hbm(fam, _nb((x, M), (y, M)) + 8 * M):
        rc = lib.tvts_layernorm_fwd(_p(x), _ld(x), 1 if x.dtype == torch.bfloat16 else 0, _p(rows), _p(gamma), _p(beta), eps, M, x.shape[1], _p(y), _ld(y),
                                    1 if y.dtype == torch.float32 else 0, _p(mean), _p(rstd), _stream())
    _chk(rc, "tvts_layernorm_fwd")


LN_WORKSPACE = {}  # per (device, lane): fp32 scratch for the per-block dgamma/dbeta partials of layernorm_bwd (1024 blocks x 2 x 1280)


def _ln_workspace(dev):
    key = (dev, current_lane())
    ws = LN_WORKSPACE.get(key)
    if ws is None:
        ws = LN_WORKSPACE[key] = torch.empty(1024 * 2 * 1280, dtype=torch.float32, device=dev)
    return ws


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, *, dx_bf16=None, res1=None, res2=None, dgamma=None, dbeta=None,
                  rows=None, M=None, workspace=True, q8=None, row_scale=None, tscale=None, amax=None,
                  cls_period=0, cls_x=None, cls_res1=None, cls_dx=None):
    """dx (fp32, may be None when only the bf16 copy is wanted) = LN backward [+ res1 (fp32 or bf16) + res2 (bf16)];
    dgamma / dbeta are ACCUMULATED (+=) from per-block partials in a shared scratch buffer.  q8 / row_scale: also the e4m3
    copy of dx_bf16 with one scale per row (bf16 dy, every row).
    cls_period > 0: the hybrid residual stream (bf16 dy / x / res1, bf16 output only) -- for the rows r % cls_period == 0 the input
    comes from cls_x, the stream gradient from cls_res1 (both float32 [M / cls_period, W], optional) and the result also goes to
    cls_dx in fp32 (optional)."""
    lib = _lib.load()
    ws = _ln_workspace(x.device) if (workspace and dgamma is not None) else None
    M = (rows.numel() if rows is not None else x.shape[0]) if M is None else M
    assert res2 is None or res2.dtype == torch.bfloat16
    fam = "ln_bwd" if M >= 4096 else "ln_bwd_small"
    nbytes = _nb((dy, M), (x, M), (res1, M), (res2, M), (dx, M), (dx_bf16, M), (q8, M)) + 8 * M
    if cls_period:
        assert rows is None and dx is None and dx_bf16 is not None and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
        assert res1 is None or res1.dtype == torch.bfloat16
        for t in (cls_x, cls_res1, cls_dx):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] * cls_period == M and t.shape[1] == x.shape[1])
        with _hbm(fam, nbytes):
            rc = lib.tvts_layernorm_bwd_cls(_p(dy), _ld(dy), _p(x), _ld(x), _p(cls_x), _p(cls_res1), _p(cls_dx), cls_period, _p(mean), _p(rstd),
                                            _p(gamma), _p(res1), _ld(res1) if res1 is not None else 0, _p(res2), _ld(res2) if res2 is not None else 0,
                                            M, x.shape[1], _p(dx_bf16), _ld(dx_bf16), _p(q8), q8.stride(0) if q8 is not None else 0, _p(row_scale),
                                            _p(tscale), _p(amax), _p(dgamma), _p(dbeta), _p(ws), ws.numel() if ws is not None else 0, _stream())
        _chk(rc, "tvts_layernorm_bwd_cls")
        return
    if q8 is not None:
        assert rows is None and dx_bf16 is not None and dy.dtype == torch.bfloat16 and (tscale is not None or (row_scale is not None and row_scale.numel() >= M))
        with _hbm(fam, nbytes):
            rc = lib.tvts_layernorm_bwd_fp8(_p(dy), _ld(dy), _p(x), _ld(x), 1 if x.dtype == torch.bfloat16 else 0, _p(mean), _p(rstd),
                                        _p(gamma), _p(res1), 1 if (res1 is not None and res1.dtype == torch.bfloat16) else 0,
                                        _ld(res1) if res1 is not None else 0, _p(res2),
                                        _ld(res2) if res2 is not None else 0, M, x.shape[1], _p(dx), _ld(dx) if dx is not None else 0,
                                            _p(dx_bf16), _ld(dx_bf16), _p(q8), q8.stride(0), _p(row_scale), _p(tscale), _p(amax), _p(dgamma), _p(dbeta), _p(ws),
                                            ws.numel() if ws is not None else 0, _stream())
        _chk(rc, "tvts_layernorm_bwd_fp8")
        return
    with _hbm(fam, nbytes):
        rc = lib.tvts_layernorm_bwd(_p(dy), _ld(dy), 1 if dy.dtype == torch.float32 else 0, _p(x), _ld(x),
                                1 if x.dtype == torch.bfloat16 else 0, _p(rows),
                                _p(mean), _p(rstd), _p(gamma), _p(res1), 1 if (res1 is not None and res1.dtype == torch.bfloat16) else 0,
                                _ld(res1) if res1 is not None else 0, _p(res2),
                                _ld(res2) if res2 is not None else 0, M, x.shape[1], _p(dx),
                                    _ld(dx) if dx is not None else 0, _p(dx_bf16), _ld(dx_bf16) if dx_bf16 is not None else 0,
                                    _p(dgamma), _p(dbeta), _p(ws), ws.numel() if ws is not None else 0, _stream())
    _chk(rc, "tvts_layernorm_bwd")


def _attn_fn(lib, name, head_dim):
    if head_dim == 64:
        return getattr(lib, "tvts_attn_" + name)
    if head_dim == 80:
        return getattr(lib, "tvts_attn80_" + name)
    raise HipError(f"attention kernels are built for head dim 64 and 80, not {head_dim}")


def attn_fwd(mode, qkv, out, lse2, *, B, heads, S, T=0, n=0, causal=False, head_dim=64, **opt):
    lib = _lib.load()
    M = B * S
    with _hbm("attn_fwd_" + mode, _nb((qkv, M), (out, M)) + 8 * M * heads):
        rc = _attn_fn(lib, "fwd", head_dim)(MODE[mode], _p(qkv), _ld(qkv), B, heads, S, T, n, int(causal), _p(out), _ld(out), _p(lse2),
                                            attn_opts(**opt), _stream())
    _chk(rc, "tvts_attn_fwd")


def attn_fwd_len(qkv, kv_len, out, lse2, *, B, heads, S, head_dim=64):
    """FULL attention, keys at positions >= kv_len[b] masked (padding)."""
    lib = _lib.load()
    assert kv_len.dtype == torch.int32 and kv_len.numel() == B
    _chk(_attn_fn(lib, "fwd_len", head_dim)(_p(qkv), _ld(qkv), B, heads, S, _p(kv_len), _p(out), _ld(out), _p(lse2), _stream()),
         "tvts_attn_fwd_len")


def attn_bwd_len(qkv, kv_len, dO, O, lse2, delta, dqkv, *, B, heads, S, head_dim=64):
    """backward of attn_fwd_len into dqkv (zeroed here first: the padded positions' dK / dV rows are not written).
    dqkv: bf16 [B * S, 3W], contiguous or a row-major view with a wider leading dimension (a multiple of 8, 16-byte base)."""
    lib = _lib.load()
    _zero_rows(dqkv)
    _chk(_attn_fn(lib, "bwd_len", head_dim)(_p(qkv), _ld(qkv), B, heads, S, _p(kv_len), _p(dO), _ld(dO), _p(O), _ld(O), _p(lse2),
                                            _p(delta), _p(dqkv), _ld(dqkv), _stream()), "tvts_attn_bwd_len")


def _zero_rows(t):
    """t[...] = 0 for a row-major bf16 matrix: one fill when it is contiguous, row by row when it is a view with a wider leading
    dimension (the columns right of it are not touched; columns and leading dimension multiples of 8, 16-byte base)"""
    assert t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1, "dqkv: a row-major bf16 matrix"
    if t.is_contiguous():
        zero_(t)
    else:
        zero_cols_bf16(t, t.shape[1])


DROP_SITE_STRIDE = 0x632BE59BD9B4E019  # odd 64-bit constant: site k of a step uses seed_dev[0] + k * this (mod 2^64)


def _site(site: int) -> int:
    v = (site * DROP_SITE_STRIDE) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v  # the same bits as a C long


def attn_fwd_len_drop(qkv, kv_len, out, lse2, *, B, heads, S, p, seed, site, head_dim=64):
    """attn_fwd_len with dropout p on the attention probabilities; seed: int64 device tensor [1], site: small int (per call site)"""
    lib = _lib.load()
    assert kv_len.dtype == torch.int32 and kv_len.numel() == B and seed.dtype == torch.int64 and seed.is_cuda
    _chk(_attn_fn(lib, "fwd_len_drop", head_dim)(_p(qkv), _ld(qkv), B, heads, S, _p(kv_len), _p(out), _ld(out), _p(lse2), float(p),
                                                 _p(seed), _site(site), _stream()), "tvts_attn_fwd_len_drop")


def attn_bwd_len_drop(qkv, kv_len, dO, O, lse2, delta, dqkv, *, B, heads, S, p, seed, site, head_dim=64):
    """backward of attn_fwd_len_drop (the mask regenerated from seed / site); dqkv as in attn_bwd_len, zeroed here first"""
    lib = _lib.load()
    _zero_rows(dqkv)
    _chk(_attn_fn(lib, "bwd_len_drop", head_dim)(_p(qkv), _ld(qkv), B, heads, S, _p(kv_len), _p(dO), _ld(dO), _p(O), _ld(O),
                                                 _p(lse2), _p(delta), _p(dqkv), _ld(dqkv), float(p), _p(seed), _site(site),
                                                 _stream()), "tvts_attn_bwd_len_drop")


def dropout_rows(x, *, p, seed, site, residual=None, out=None, out_bf16=None):
    """out = x * mask / (1 - p) (+ residual), fp32 and / or bf16 output; the backward is the same call on the gradient."""
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.dim() == 2 and seed.dtype == torch.int64
    _chk(lib.tvts_dropout_rows(_p(x), _ld(x), x.shape[0], x.shape[1], float(p), _p(seed), _site(site), _p(residual),
                               _ld(residual) if residual is not None else 0, _p(out), _ld(out) if out is not None else 0,
                               _p(out_bf16), _ld(out_bf16) if out_bf16 is not None else 0, _stream()), "tvts_dropout_rows")


def attn_fwd_tail(qkv, out, lse2, *, B, heads, S, nq, head_dim=64):
    """FULL attention whose only queries are the last nq tokens of every sequence (rows b*S + S-nq .. of out / lse2 are written)."""
    lib = _lib.load()
    _chk(_attn_fn(lib, "fwd_tail", head_dim)(_p(qkv), _ld(qkv), B, heads, S, nq, _p(out), _ld(out), _p(lse2), _stream()),
         "tvts_attn_fwd_tail")


def attn_bwd_tail(qkv, dO, O, lse2, delta, dqkv, *, B, heads, S, nq, head_dim=64):
    """backward of attn_fwd_tail: dQ into the query rows, dK / dV into every row of dqkv; the dQ third of the other rows is the
    caller's to zero."""
    lib = _lib.load()
    _chk(_attn_fn(lib, "bwd_tail", head_dim)(_p(qkv), _ld(qkv), B, heads, S, nq, _p(dO), _ld(dO), _p(O), _ld(O), _p(lse2), _p(delta),
                                             _p(dqkv), _ld(dqkv), _stream()), "tvts_attn_bwd_tail")


def attn_fwd_rowq(qkv, qpos, out, lse2, *, B, heads, S, head_dim=64):
    """one query per sequence at token qpos[b] (int32 device tensor) attending the keys 0 .. qpos[b]; row b*S + qpos[b] of out / lse2."""
    lib = _lib.load()
    assert qpos.dtype == torch.int32 and qpos.numel() == B
    _chk(_attn_fn(lib, "fwd_rowq", head_dim)(_p(qkv), _ld(qkv), B, heads, S, _p(qpos), _p(out), _ld(out), _p(lse2), _stream()),
         "tvts_attn_fwd_rowq")


def attn_fwd_first(qkv, kv_len, out, lse2, *, B, heads, S, head_dim=64):
    """one query per sequence at token row 0 over the keys 0 .. nk - 1 (nk = S, or clamp(kv_len[b], 1, S) with the int32 device
    tensor kv_len); forward-only: row b*S of out (and of lse2, if given) is written and no other."""
    lib = _lib.load()
    assert kv_len is None or (kv_len.dtype == torch.int32 and kv_len.numel() == B)
    assert qkv.shape[0] >= B * S and out.shape[0] >= B * S
    _chk(_attn_fn(lib, "fwd_first", head_dim)(_p(qkv), _ld(qkv), B, heads, S, _p(kv_len), _p(out), _ld(out), _p(lse2), _stream()),
         "tvts_attn_fwd_first")


def attn_fwd_packed(qkv, seq_start, out, *, N, heads, max_len, last_only=False, lse2=None):
    """causal attention inside each sequence of a packed batch (seq_start int32 [N + 1], rows seq_start[i] .. seq_start[i + 1] - 1),
    head dim 64.  last_only: one query per sequence at its last row; only those N rows of out are written.  lse2 (fp32 [M, heads]):
    the training entries -- the same kernels and the same bits in out, and the log-sum-exp of every row they compute stored for
    attn_bwd_packed."""
    lib = _lib.load()
    assert seq_start.dtype == torch.int32 and seq_start.numel() == N + 1
    M = qkv.shape[0]
    assert out.shape[0] == M
    name = "tvts_attn_fwd_packed" + ("_last" if last_only else "") + ("_lse" if lse2 is not None else "")
    args = (_p(qkv), _ld(qkv), _p(seq_start), N, M, heads, max_len, _p(out), _ld(out))
    if lse2 is not None:
        assert lse2.dtype == torch.float32 and lse2.is_contiguous() and lse2.numel() >= M * heads
        args += (_p(lse2),)
    _chk(getattr(lib, name)(*args, _stream()), name)


def attn_bwd_packed(qkv, seq_start, dO, O, lse2, delta, dqkv, *, N, heads, max_len, last_only=False):
    """backward of attn_fwd_packed(..., lse2=...) into dqkv bf16 [M, 3W] (contiguous or a row-major view with a wider leading
    dimension, a multiple of 8): every row of a valid sequence is written in all three thirds, so dqkv needs no zeroing -- with
    last_only the KERNEL zeroes the dQ third of the rows that are no sequence's last one (no _zero_rows here).  delta fp32 [M, heads] is
    written on the way.  One wave owns a (sequence, head) group: no atomics, two runs give the same bits."""
    lib = _lib.load()
    assert seq_start.dtype == torch.int32 and seq_start.numel() == N + 1
    M = qkv.shape[0]
    assert dO.shape[0] == M and O.shape[0] == M and dqkv.shape[0] == M
    assert lse2 is None or (lse2.dtype == torch.float32 and lse2.numel() >= M * heads)
    assert delta is None or (delta.dtype == torch.float32 and delta.numel() >= M * heads)
    name = "tvts_attn_bwd_packed_last" if last_only else "tvts_attn_bwd_packed"
    _chk(getattr(lib, name)(_p(qkv), _ld(qkv), _p(seq_start), N, M, heads, max_len, _p(dO), _ld(dO), _p(O), _ld(O), _p(lse2), _p(delta),
                            _p(dqkv), _ld(dqkv), _stream()), name)


def attn_fwd_packed_bidir(qkv, seq_start, out, lse2=None, *, N, heads, max_len, L_pad, p=0.0, seed=None, site=0):
    """bidirectional attention inside each sequence of a packed batch (the DistilBERT tower of v1), dropout p on the probabilities
    with the mask tvts_attn_fwd_len_drop draws on [N, L_pad] padded captions from the same (seed, site).  lse2 fp32 [M, heads] or None."""
    lib = _lib.load()
    assert seq_start.dtype == torch.int32 and seq_start.numel() == N + 1
    M = qkv.shape[0]
    assert out.shape[0] == M and (seed is None or (seed.dtype == torch.int64 and seed.is_cuda))
    assert lse2 is None or (lse2.dtype == torch.float32 and lse2.is_contiguous() and lse2.numel() >= M * heads)
    _chk(lib.tvts_attn_fwd_packed_bidir(_p(qkv), _ld(qkv), _p(seq_start), N, M, heads, max_len, _p(out), _ld(out), _p(lse2), float(p),
                                        _p(seed), _site(site), L_pad, _stream()), "tvts_attn_fwd_packed_bidir")


def attn_bwd_packed_bidir(qkv, seq_start, dO, O, lse2, delta, dqkv, *, N, heads, max_len, L_pad, p=0.0, seed=None, site=0):
    """backward of attn_fwd_packed_bidir (the mask regenerated from seed / site) into dqkv bf16 [M, 3W]: every row of a valid sequence
    is written in all three thirds (no zeroing here), delta fp32 [M, heads] on the way; two runs give the same bits."""
    lib = _lib.load()
    assert seq_start.dtype == torch.int32 and seq_start.numel() == N + 1
    M = qkv.shape[0]
    assert dO.shape[0] == M and O.shape[0] == M and dqkv.shape[0] == M
    assert lse2 is None or (lse2.dtype == torch.float32 and lse2.numel() >= M * heads)
    assert delta is None or (delta.dtype == torch.float32 and delta.numel() >= M * heads)
    assert seed is None or (seed.dtype == torch.int64 and seed.is_cuda)
    _chk(lib.tvts_attn_bwd_packed_bidir(_p(qkv), _ld(qkv), _p(seq_start), N, M, heads, max_len, _p(dO), _ld(dO), _p(O), _ld(O), _p(lse2),
                                        _p(delta), _p(dqkv), _ld(dqkv), float(p), _p(seed), _site(site), L_pad, _stream()),
         "tvts_attn_bwd_packed_bidir")


def attn_fwd_packed_first(qkv, seq_start, out, *, N, heads, max_len):
    """one query per packed sequence at its FIRST row ([CLS]) over all its keys; only the rows seq_start[i] of out are written"""
    lib = _lib.load()
    assert seq_start.dtype == torch.int32 and seq_start.numel() == N + 1
    M = qkv.shape[0]
    assert out.shape[0] == M
    _chk(lib.tvts_attn_fwd_packed_first(_p(qkv), _ld(qkv), _p(seq_start), N, M, heads, max_len, _p(out), _ld(out), _stream()),
         "tvts_attn_fwd_packed_first")


def dropout_rows_packed(x, seq_start, *, N, L_pad, p, seed, site, residual=None, out=None, out_bf16=None):
    """dropout_rows over packed captions x fp32 [M, cols]: the mask dropout_rows draws on the [N * L_pad, cols] padded buffer, read
    at every row's padded position; the backward is the same call on the gradient."""
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.dim() == 2 and seed.dtype == torch.int64
    assert seq_start.dtype == torch.int32 and seq_start.numel() == N + 1
    _chk(lib.tvts_dropout_rows_packed(_p(x), _ld(x), _p(seq_start), N, x.shape[0], x.shape[1], L_pad, float(p), _p(seed), _site(site),
                                      _p(residual), _ld(residual) if residual is not None else 0, _p(out),
                                      _ld(out) if out is not None else 0, _p(out_bf16), _ld(out_bf16) if out_bf16 is not None else 0,
                                      _stream()), "tvts_dropout_rows_packed")


def attn_bwd_rowq(qkv, qpos, dO, O, lse2, delta, dqkv, *, B, heads, S, head_dim=64):
    """backward of attn_fwd_rowq into dqkv (zeroed here first: only the query row's dQ and the dK / dV of the keys it sees exist).
    dqkv: bf16 [B * S, 3W], contiguous or a row-major view with a wider leading dimension (a multiple of 8, 16-byte base)."""
    lib = _lib.load()
    _zero_rows(dqkv)
    _chk(_attn_fn(lib, "bwd_rowq", head_dim)(_p(qkv), _ld(qkv), B, heads, S, _p(qpos), _p(dO), _ld(dO), _p(O), _ld(O), _p(lse2),
                                             _p(delta), _p(dqkv), _ld(dqkv), _stream()), "tvts_attn_bwd_rowq")


def attn_delta(dO, O, delta, *, rows, heads, head_dim=64):
    lib = _lib.load()
    _chk(_attn_fn(lib, "delta", head_dim)(_p(dO), _ld(dO), _p(O), _ld(O), rows, heads, _p(delta), _stream()), "tvts_attn_delta")


def attn_bwd_dq(mode, qkv, dO, lse2, delta, dqkv, *, B, heads, S, T=0, n=0, causal=False, head_dim=64, **opt):
    lib = _lib.load()
    rc = _attn_fn(lib, "bwd_dq", head_dim)(MODE[mode], _p(qkv), _ld(qkv), B, heads, S, T, n, int(causal), _p(dO), _ld(dO), _p(lse2),
                              _p(delta), _p(dqkv), _ld(dqkv), attn_opts(**opt), _stream())
    _chk(rc, "tvts_attn_bwd_dq")


def attn_bwd_dkv(mode, qkv, dO, lse2, delta, dqkv, *, B, heads, S, T=0, n=0, causal=False, cls_acc=None, head_dim=64, **opt):
    lib = _lib.load()
    rc = _attn_fn(lib, "bwd_dkv", head_dim)(MODE[mode], _p(qkv), _ld(qkv), B, heads, S, T, n, int(causal), _p(dO), _ld(dO),
                               _p(lse2), _p(delta), _p(dqkv), _ld(dqkv), _p(cls_acc), attn_opts(**opt), _stream())
    _chk(rc, "tvts_attn_bwd_dkv")


def attn_fwd_divided(mode, qkv, out, lse2, cls_ws, *, B, heads, S, T, n, head_dim=64, q8out=None, q8_scale=None, q8_amax=None, **opt):
    """Forward of one divided-attention site (patch rows + CLS row); cls_ws is fp32 scratch.  q8out (uint8, out's shape and row
    stride) + q8_scale / q8_amax: the kernels also write the per-tensor e4m3 copy of the output.  lse2 = None (also in attn_fwd,
    attn_fwd_rowq, attn_fwd_tail): a forward-only call, no log-sum-exp is stored (full-frame SPACE groups: a kernel of its own)."""
    lib = _lib.load()
    M = B * S
    with _hbm("attn_fwd_" + mode, _nb((qkv, M), (out, M), (q8out, M)) + 8 * M * heads):  # (launches its CLS merge kernel as well)
        if q8out is not None:
            rc = _attn_fn(lib, "fwd_divided_q8", head_dim)(MODE[mode], _p(qkv), _ld(qkv), B, heads, S, T, n, _p(out), _ld(out), _p(lse2),
                                                           _p(cls_ws), cls_ws.numel(), _p(q8out), q8out.stride(0), _p(q8_scale),
                                                           _p(q8_amax), attn_opts(**opt), _stream())
        else:
            rc = _attn_fn(lib, "fwd_divided", head_dim)(MODE[mode], _p(qkv), _ld(qkv), B, heads, S, T, n, _p(out), _ld(out), _p(lse2),
                                                        _p(cls_ws), cls_ws.numel(), attn_opts(**opt), _stream())
    _chk(rc, "tvts_attn_fwd_divided")


def attn_bwd(mode, qkv, dO, O, lse2, delta, dqkv, *, B, heads, S, T=0, n=0, causal=False, cls_acc=None, head_dim=64, q8out=None,
             q8_scale=None, q8_amax=None, **opt):
    """Whole backward of one attention site into dqkv (delta / cls_acc are scratch).  q8out (uint8, dqkv's shape and row stride): the
    kernels also write the per-tensor e4m3 copy of dqkv (fused divided geometries)."""
    lib = _lib.load()
    M = B * S
    if q8out is not None:
        with _hbm("attn_bwd_" + mode, _nb((qkv, M), (dO, M), (O, M), (dqkv, M), (q8out, M)) + 8 * M * heads):
            rc = _attn_fn(lib, "bwd_q8", head_dim)(MODE[mode], _p(qkv), _ld(qkv), B, heads, S, T, n, int(causal), _p(dO), _ld(dO), _p(O),
                                                   _ld(O), _p(lse2), _p(delta), _p(dqkv), _ld(dqkv), _p(cls_acc),
                                                   cls_acc.numel() if cls_acc is not None else 0, _p(q8out), q8out.stride(0),
                                                   _p(q8_scale), _p(q8_amax), attn_opts(**opt), _stream())
        _chk(rc, "tvts_attn_bwd_q8")
        return
    with _hbm("attn_bwd_" + mode, _nb((qkv, M), (dO, M), (O, M), (dqkv, M)) + 8 * M * heads):  # (delta / CLS finalize kernels included)
        rc = _attn_fn(lib, "bwd", head_dim)(MODE[mode], _p(qkv), _ld(qkv), B, heads, S, T, n, int(causal), _p(dO), _ld(dO), _p(O),
                                            _ld(O), _p(lse2), _p(delta), _p(dqkv), _ld(dqkv), _p(cls_acc),
                                            cls_acc.numel() if cls_acc is not None else 0, attn_opts(**opt), _stream())
    _chk(rc, "tvts_attn_bwd")


def attn_cls_finalize(cls_acc, dqkv, *, B, heads, S, head_dim=64):
    lib = _lib.load()
    _chk(_attn_fn(lib, "cls_finalize", head_dim)(_p(cls_acc), B, heads, S, _p(dqkv), _ld(dqkv), _stream()), "tvts_attn_cls_finalize")


def patch_gather(video, keep, out, *, B, T, n, img, patch):
    lib = _lib.load()
    assert video.dtype == torch.float32 and keep.dtype == torch.int32 and video.is_contiguous()
    _chk(lib.tvts_patch_gather(_p(video), _p(keep), B, T, n, img, patch, _p(out), _ld(out), _stream()), "tvts_patch_gather")


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # video_transforms/videoaug.py:17,26


def patch_gather_u8(frames, keep, out, *, B, T, n, img, patch, crop=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, resize=None):
    """frames: uint8 [B, T, H0, W0, 3] on the device; crop: int32 [B, 2] (top, left) or None (centre crop).
    resize = (ytab int32 [H0], xtab int32 [W0]) device tables: the frames are the decoder's pictures and the crop applies to
    their nearest-neighbour resize to H0 x W0 (the reference's video_transform.Resize)."""
    import ctypes
    lib = _lib.load()
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.shape[-1] == 3 and keep.dtype == torch.int32
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    if resize is not None:
        ytab, xtab = resize
        assert ytab.dtype == torch.int32 and xtab.dtype == torch.int32
        _chk(lib.tvts_patch_gather_u8_resized(_p(frames), frames.shape[2], frames.shape[3], _p(ytab), _p(xtab), ytab.numel(),
                                              xtab.numel(), _p(crop), _p(keep), B, T, n, img, patch, m3, s3, _p(out), _ld(out),
                                              _stream()), "tvts_patch_gather_u8_resized")
        return
    _chk(lib.tvts_patch_gather_u8(_p(frames), frames.shape[2], frames.shape[3], _p(crop), _p(keep), B, T, n, img, patch, m3, s3,
                                  _p(out), _ld(out), _stream()), "tvts_patch_gather_u8")


# ---- the ragged uint8 input of the v2 step (embed.hip: tvts_patch_gather_u8_ragged; DESIGN.md 8j "v2 ragged")
_NEAREST_TABLES = {}


def nearest_table(n_in, n_out):
    """the int32 table of one axis as tvts_patch_gather_u8_ragged reads it: (n_in, n_out) | transforms.pil_nearest_table(n_in, n_out),
    cached per (n_in, n_out) -> 1-D numpy int32"""
    import numpy as np
    key = (int(n_in), int(n_out))
    t = _NEAREST_TABLES.get(key)
    if t is None:
        from .data_loader.transforms import pil_nearest_table
        t = _NEAREST_TABLES[key] = np.array(list(key) + pil_nearest_table(*key), dtype=np.int32)
        t.setflags(write=False)
    return t


def gather_plan(sizes, frames, crops, *, size, img, T, offsets=None):
    """the host half of tvts_patch_gather_u8_ragged for a batch of source clips: sizes B x (Hs, Ws); frames B clip lengths (1 .. T);
    crops B x (top, left) in RESIZED coordinates or None (the centre crop of every clip: CenterCrop's round-half-to-even offsets);
    size: video_transform.Resize(size), None = no Resize (identity tables); offsets: the clips' byte offsets in the packed buffer
    (default: back to back) -> dict(desc int64 [B, 8], tables int32, numpy; offsets; nbytes: what the clips occupy).  One table per
    distinct (n_in, n_out), shared between the clips and axes that use it.  ValueError by name for what check_gather_plan refuses."""
    import numpy as np
    from .data_loader.transforms import centre_crop_offset, resize_sizes
    B = len(sizes)
    if B < 1 or len(frames) != B or (crops is not None and len(crops) != B) or (offsets is not None and len(offsets) != B):
        raise ValueError(f"gather plan: {B} sizes, {len(frames)} lengths" + ("" if crops is None else f", {len(crops)} crops")
                         + ("" if offsets is None else f", {len(offsets)} offsets"))
    desc = np.zeros((B, 8), dtype=np.int64)
    where, parts, total, at = {}, [], 0, 0
    for b, (hs, ws) in enumerate(sizes):
        hs, ws, fr = int(hs), int(ws), int(frames[b])
        if hs < 1 or ws < 1:
            raise ValueError(f"gather plan: clip {b} has frames of {hs} x {ws}")
        if fr < 1 or fr > T:
            raise ValueError(f"gather plan: clip {b} has {fr} frames, needs 1 <= frames <= {T}")
        nh, nw = (hs, ws) if size is None else resize_sizes(hs, ws, int(size))
        if nh < img or nw < img:
            raise ValueError(f"gather plan: clip {b} ({hs} x {ws}) " + ("is" if size is None else f"resizes to {nh} x {nw} under "
                             f"Resize({size}),") + f" below the crop of {img} x {img}")
        loc = []
        for key in ((hs, nh), (ws, nw)):
            if key not in where:
                where[key] = total
                parts.append(nearest_table(*key))
                total += parts[-1].size
            loc.append(where[key])
        top, left = (centre_crop_offset(nh - img), centre_crop_offset(nw - img)) if crops is None else (int(crops[b][0]), int(crops[b][1]))
        off = at if offsets is None else int(offsets[b])
        desc[b] = (off, hs, ws, top, left, loc[0], loc[1], fr)
        at = off + fr * hs * ws * 3
    tables = np.concatenate(parts)
    nbytes = int(max(desc[:, 0] + desc[:, 7] * desc[:, 1] * desc[:, 2] * 3))
    check_gather_plan(desc, tables, T=T, img=img, src_bytes=nbytes)
    return dict(desc=desc, tables=tables, offsets=desc[:, 0].copy(), nbytes=nbytes)


def check_gather_plan(desc, tables, *, T, img, src_bytes):
    """the host-side check of a gather plan (the C entry point takes both as unchecked device data): desc integer [B, 8] = (offset,
    Hs, Ws, top, left, ytab, xtab, frames), tables int32.  ValueError for frames outside [1, T], a clip that leaves the src_bytes of
    the packed buffer, a table location outside `tables`, a table that is not the one of its (n_in, n_out) or whose n_in is not the
    clip's side, a resized side below img, a crop outside the resized frame (0 <= top <= new_h - img, 0 <= left <= new_w - img)."""
    import numpy as np
    d, tb = np.asarray(desc), np.asarray(tables)
    if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] != 8 or d.dtype.kind not in "iu" or tb.ndim != 1 or tb.dtype != np.int32:
        raise ValueError(f"gather plan: integer desc [B, 8] and int32 tables [n], got {d.dtype} {d.shape} / {tb.dtype} {tb.shape}")
    if T < 1 or img < 1:
        raise ValueError(f"gather plan: T = {T}, img = {img}")
    seen = {}
    for b, (off, hs, ws, top, left, yt, xt, fr) in enumerate(d.astype(np.int64).tolist()):
        if fr < 1 or fr > T:
            raise ValueError(f"gather plan: clip {b} has {fr} frames, needs 1 <= frames <= {T}")
        if hs < 1 or ws < 1 or off < 0 or off + fr * hs * ws * 3 > src_bytes:
            raise ValueError(f"gather plan: clip {b} ({fr} x {hs} x {ws} x 3 bytes at offset {off}) leaves the buffer of {src_bytes} bytes")
        for loc, n_in, at, ax in ((yt, hs, top, "top"), (xt, ws, left, "left")):
            if loc not in seen:
                if loc < 0 or loc + 2 > tb.size:
                    raise ValueError(f"gather plan: clip {b} names a table at {loc}, outside the {tb.size} table elements")
                t_in, n_out = int(tb[loc]), int(tb[loc + 1])
                if t_in < 1 or n_out < 1 or loc + 2 + n_out > tb.size or not np.array_equal(tb[loc:loc + 2 + n_out],
                                                                                         nearest_table(t_in, n_out)):
                    raise ValueError(f"gather plan: the table at {loc} is not pil_nearest_table({t_in}, {n_out})")
                seen[loc] = (t_in, n_out)
            t_in, n_out = seen[loc]
            if t_in != n_in:
                raise ValueError(f"gather plan: clip {b} has a side of {n_in}, its table resamples {t_in}")
            if n_out < img:
                raise ValueError(f"gather plan: clip {b} resizes to a side of {n_out}, below the crop of {img}")
            if at < 0 or at > n_out - img:
                raise ValueError(f"gather plan: clip {b}: crop outside the resized frame, needs 0 <= {ax} <= {n_out - img}, got {at}")


def patch_gather_u8_ragged(src, desc, tables, keep, out, *, B, T, n, img, patch, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """the tube-mask gather over RAGGED uint8 clips: src uint8 [nbytes], the packed source clips; desc int64 [B, 8] and tables int32,
    the device copies of a gather_plan(); keep int32 [B, n]; out bf16 [B * T * n, ldo] -- the rows of patch_gather_u8(resize=...) on
    every clip alone, zero rows for the frames behind a short clip's end"""
    import ctypes
    assert src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous() and keep.dtype == torch.int32 and keep.is_contiguous()
    assert desc.dtype == torch.int64 and desc.is_contiguous() and tuple(desc.shape) == (B, 8) and tables.dtype == torch.int32
    assert tuple(keep.shape) == (B, n) and out.dtype == torch.bfloat16 and out.shape[0] == B * T * n
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    _chk(_lib.load().tvts_patch_gather_u8_ragged(_p(src), _p(desc), _p(tables), _p(keep), B, T, n, img, patch, m3, s3, _p(out),
                                                 _ld(out), _stream()), "tvts_patch_gather_u8_ragged")


def tube_mask(seed, first_sample, B, ppf, n_keep, out=None, device=None):
    """keep_ind int32 [B, n_keep] drawn on the device: sample number first_sample + b gets the n_keep patch indices with the
    smallest counter-based random keys (an unsorted prefix of a random permutation, YTTemporal_dataset.py:207-213)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(B, n_keep, dtype=torch.int32, device=device if device is not None else "cuda")
    assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (B, n_keep)
    s64 = lambda v: (int(v) & (2 ** 64 - 1)) - (2 ** 64 if int(v) & (1 << 63) else 0)  # unsigned 64-bit through a C long
    _chk(lib.tvts_tube_mask(s64(seed), s64(first_sample), B, ppf, n_keep, _p(out), _stream()), "tvts_tube_mask")
    return out


def vit_assemble(patch, cls, pos, temporal, keep, tok, *, B, T, n):
    """keep [B, n] (one tube mask per clip, v2) or [B, T, n] (one per frame / tubelet, v1)"""
    lib = _lib.load()
    _chk(lib.tvts_vit_assemble(_p(patch), _ld(patch), _p(cls), _p(pos), _p(temporal), _p(keep), 1 if keep.dim() == 3 else 0,
                               B, T, n, tok.shape[1], _p(tok), _ld(tok), _stream()), "tvts_vit_assemble")


def vit_assemble_bwd(dtok, keep, dpatch, dcls, dpos, dtemporal, *, B, T, n):
    lib = _lib.load()
    ws = _tn_workspace(dtok.device)  # ordered partials of the temporal / class embedding sums (shared fp32 scratch of this stream)
    _chk(lib.tvts_vit_assemble_bwd(_p(dtok), _ld(dtok), _p(keep), 1 if keep.dim() == 3 else 0, B, T, n, dtok.shape[1],
                                   _p(dpatch), _ld(dpatch), _p(dcls), _p(dpos), dpos.shape[0] - 1, _p(dtemporal), _p(ws), ws.numel(),
                                   _stream()),
         "tvts_vit_assemble_bwd")


# ---- the v1 tubelet gathers (embed.hip: one kernel frame over four source policies).  What their wrappers check, stated once:
def _tube_rows(keep, out, *, B, tubes, n):
    assert keep.dtype == torch.int32 and keep.is_contiguous() and tuple(keep.shape) == (B, tubes, n), "keep: int32 [B, tubes, n]"
    assert out.dtype == torch.bfloat16


def _cm_clip(video, *, B, T, img):
    assert video.dtype == torch.float32 and video.is_contiguous() and tuple(video.shape) == (B, 3, T, img, img)


def _u8_clips(frames, T=None, B=None):
    """uint8 clips [B, T, H0, W0, 3] as the decoder leaves them, contiguous -> (B, T, H0, W0)"""
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.dim() == 5 and frames.shape[-1] == 3
    assert (B is None or frames.shape[0] == B) and (T is None or frames.shape[1] == T)
    return frames.shape[:4]


def _crop_dev(crop, B):
    assert crop is None or (crop.dtype == torch.int32 and crop.is_contiguous() and tuple(crop.shape) == (B, 2))
    return _p(crop)


def _norm3(mean, std):
    return (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)


def patch_gather_tube(video, keep, out, *, B, tubes, tubelet, n, img, patch, channel_major=False):
    """v1 tubelet im2col: video fp32 [B, T, 3, img, img] (channel_major: [B, 3, T, img, img], the layout of the v1 downstream
    classes), keep int32 [B, tubes, n] -> out bf16 [B*tubes*n, 3*tubelet*patch^2]"""
    lib = _lib.load()
    _tube_rows(keep, out, B=B, tubes=tubes, n=n)
    if channel_major:
        _cm_clip(video, B=B, T=tubes * tubelet, img=img)
        _chk(lib.tvts_patch_gather_tube_cm(_p(video), _p(keep), B, tubes, tubelet, n, img, patch, _p(out), _ld(out), _stream()),
             "tvts_patch_gather_tube_cm")
        return
    assert video.dtype == torch.float32
    _chk(lib.tvts_patch_gather_tube(_p(video), _p(keep), B, tubes, tubelet, n, img, patch, _p(out), _ld(out), _stream()),
         "tvts_patch_gather_tube")


def patch_gather_tube_u8(frames, keep, out, *, B, tubes, tubelet, n, img, patch, crop=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """v1 tubelet im2col from uint8 frames [B, T, H0, W0, 3] on the device: crop (int32 [B, 2] (top, left), None = centre crop),
    / 255 and Normalize fused into the gather; keep int32 [B, tubes, n] -> out bf16 [B*tubes*n, 3*tubelet*patch^2]"""
    _, _, H0, W0 = _u8_clips(frames, T=tubes * tubelet, B=B)
    _tube_rows(keep, out, B=B, tubes=tubes, n=n)
    _chk(_lib.load().tvts_patch_gather_tube_u8(_p(frames), H0, W0, _crop_dev(crop, B), _p(keep), B, tubes, tubelet, n, img, patch,
                                               *_norm3(mean, std), _p(out), _ld(out), _stream()), "tvts_patch_gather_tube_u8")


def check_mix_plan(mix_i, mix_f, *, B, img):
    """the host-side check of a Mixup / CutMix plan (the C entry points take the table as unchecked device data): mix_i integer
    [B, 6] = (partner, mode, yl, yh, xl, xh), mix_f float [B, 2] = (lam, one_minus_lam) -> (int32, float32) numpy arrays.
    ValueError for a partner outside [0, B), a mode outside {0, 1, 2, 3} or a box that is not 0 <= lo <= hi <= img."""
    import numpy as np
    mi, mf = np.asarray(mix_i), np.asarray(mix_f)
    if mi.shape != (B, 6) or mi.dtype.kind not in "iu" or mf.shape != (B, 2) or mf.dtype.kind != "f":
        raise ValueError(f"mix plan: integer mix_i [{B}, 6] and float mix_f [{B}, 2], got {mi.dtype} {mi.shape} / {mf.dtype} {mf.shape}")
    mi = mi.astype(np.int64)
    if ((mi[:, 0] < 0) | (mi[:, 0] >= B)).any():
        raise ValueError(f"mix plan: partner outside [0, {B})")
    if ((mi[:, 1] < 0) | (mi[:, 1] > 3)).any():
        raise ValueError("mix plan: mode must be 0 (none), 1 (mixup), 2 (cutmix) or 3 (pair-mode cutmix: the box over frames x rows)")
    for lo, hi, ax in ((2, 3, "y"), (4, 5, "x")):
        if ((mi[:, lo] < 0) | (mi[:, lo] > mi[:, hi]) | (mi[:, hi] > img)).any():
            raise ValueError(f"mix plan: box needs 0 <= {ax}l <= {ax}h <= {img}")
    if not np.isfinite(mf).all():
        raise ValueError("mix plan: lam / one_minus_lam must be finite")
    return np.ascontiguousarray(mi, dtype=np.int32), np.ascontiguousarray(mf, dtype=np.float32)


def mix_table(mix_i, mix_f, *, B, img, device="cuda"):
    """check_mix_plan, then the upload -> (mix_i int32 [B, 6], mix_f fp32 [B, 2]) on the device, as the _mix kernels read them"""
    mi, mf = check_mix_plan(mix_i, mix_f, B=B, img=img)
    return torch.from_numpy(mi).to(device), torch.from_numpy(mf).to(device)


def _mix_dev(mix, B):
    mi, mf = mix
    assert mi.dtype == torch.int32 and mi.is_contiguous() and tuple(mi.shape) == (B, 6), "mix_i: int32 [B, 6] from mix_table()"
    assert mf.dtype == torch.float32 and mf.is_contiguous() and tuple(mf.shape) == (B, 2), "mix_f: fp32 [B, 2] from mix_table()"
    return mi, mf


def patch_gather_tube_mix(video, keep, out, mix, *, B, tubes, tubelet, n, img, patch):
    """patch_gather_tube(channel_major=True) with Mixup / CutMix applied per element in front of the bf16 rounding; mix: the device
    table of mix_table()"""
    mi, mf = _mix_dev(mix, B)
    _cm_clip(video, B=B, T=tubes * tubelet, img=img)
    _tube_rows(keep, out, B=B, tubes=tubes, n=n)
    _chk(_lib.load().tvts_patch_gather_tube_cm_mix(_p(video), _p(keep), _p(mi), _p(mf), B, tubes, tubelet, n, img, patch, _p(out),
                                                   _ld(out), _stream()), "tvts_patch_gather_tube_cm_mix")


def patch_gather_tube_u8_mix(frames, keep, out, mix, *, B, tubes, tubelet, n, img, patch, crop=None, mean=IMAGENET_MEAN,
                             std=IMAGENET_STD):
    """patch_gather_tube_u8 with Mixup / CutMix: both samples cropped (each by its own offset) and normalised, then mixed"""
    mi, mf = _mix_dev(mix, B)
    _, _, H0, W0 = _u8_clips(frames, T=tubes * tubelet, B=B)
    _tube_rows(keep, out, B=B, tubes=tubes, n=n)
    _chk(_lib.load().tvts_patch_gather_tube_u8_mix(_p(frames), H0, W0, _crop_dev(crop, B), _p(keep), _p(mi), _p(mf), B, tubes, tubelet,
                                                   n, img, patch, *_norm3(mean, std), _p(out), _ld(out), _stream()),
         "tvts_patch_gather_tube_u8_mix")


def check_aug_plan(aug_i, *, Bs, H0, W0, img):
    """the host-side check of an augmentation plan (the C entry point takes the table as unchecked device data): aug_i integer
    [B, 16] = (src, top, left, h, w, flip, emode, etop, eleft, eh, ew, key_lo, key_hi, 0, 0, 0) -> int32 numpy array.
    ValueError for a src outside [0, Bs), a crop that is not 1 <= h, 1 <= w inside the H0 x W0 frame, a flip outside {0, 1}, an
    emode outside 0-3, an erase box outside the img x img picture, or a nonzero reserved column."""
    import numpy as np
    ai = np.asarray(aug_i)
    if ai.ndim != 2 or ai.shape[0] < 1 or ai.shape[1] != 16 or ai.dtype.kind not in "iu":
        raise ValueError(f"aug plan: integer aug_i [B, 16], got {ai.dtype} {ai.shape}")
    ai = ai.astype(np.int64)
    if ((ai[:, 11:13] < -(1 << 31)) | (ai[:, 11:13] >= (1 << 32))).any():
        raise ValueError("aug plan: key_lo / key_hi are 32-bit words")
    ai[:, 11:13] = ai[:, 11:13].astype(np.uint32).astype(np.int32)  # (unsigned words are stored by their bits)
    if ((ai[:, 0] < 0) | (ai[:, 0] >= Bs)).any():
        raise ValueError(f"aug plan: src outside [0, {Bs})")
    for lo, ext, size, ax in ((1, 3, H0, "top / h"), (2, 4, W0, "left / w")):
        if ((ai[:, ext] < 1) | (ai[:, lo] < 0) | (ai[:, lo] + ai[:, ext] > size)).any():
            raise ValueError(f"aug plan: crop ({ax}) needs 1 <= extent, 0 <= offset and offset + extent <= {size}")
    if ((ai[:, 5] < 0) | (ai[:, 5] > 1)).any():
        raise ValueError("aug plan: flip must be 0 or 1")
    if ((ai[:, 6] < 0) | (ai[:, 6] > 3)).any():
        raise ValueError("aug plan: emode must be 0 (none), 1 (const), 2 (rand) or 3 (pixel)")
    for lo, ext, ax in ((7, 9, "etop / eh"), (8, 10, "eleft / ew")):
        if ((ai[:, ext] < 0) | (ai[:, lo] < 0) | (ai[:, lo] + ai[:, ext] > img)).any():
            raise ValueError(f"aug plan: erase box ({ax}) needs 0 <= offset, 0 <= extent and offset + extent <= {img}")
    if ai[:, 13:].any():
        raise ValueError("aug plan: columns 13-15 are reserved and must be 0")
    return np.ascontiguousarray(ai, dtype=np.int32)


def aug_table(aug_i, *, Bs, H0, W0, img, device="cuda"):
    """check_aug_plan, then the upload -> aug_i int32 [B, 16] on the device, as tvts_patch_gather_tube_u8_aug reads it"""
    return torch.from_numpy(check_aug_plan(aug_i, Bs=Bs, H0=H0, W0=W0, img=img)).to(device)


def patch_gather_tube_u8_aug(frames, keep, out, aug, mix=None, *, B, tubes, tubelet, n, img, patch, mean=IMAGENET_MEAN,
                             std=IMAGENET_STD):
    """v1 tubelet im2col with the per-sample augmentation fused in: frames uint8 [Bs, T, H0, W0, 3] on the device (any H0, W0 >= 1),
    aug the device table of aug_table() for B samples (each names its source clip) -- Normalize, random-resized crop (bilinear),
    flip, random erasing --, mix (optional) the device table of mix_table() for the same B samples, applied behind the erase;
    keep int32 [B, tubes, n] -> out bf16 [B*tubes*n, 3*tubelet*patch^2]"""
    Bs, _, H0, W0 = _u8_clips(frames, T=tubes * tubelet)
    assert aug.dtype == torch.int32 and aug.is_contiguous() and tuple(aug.shape) == (B, 16), "aug: int32 [B, 16] from aug_table()"
    _tube_rows(keep, out, B=B, tubes=tubes, n=n)
    mi, mf = _mix_dev(mix, B) if mix is not None else (None, None)
    _chk(_lib.load().tvts_patch_gather_tube_u8_aug(_p(frames), Bs, H0, W0, _p(keep), _p(aug), _p(mi), _p(mf), B, tubes, tubelet, n, img,
                                                   patch, *_norm3(mean, std), _p(out), _ld(out), _stream()),
         "tvts_patch_gather_tube_u8_aug")


RA_MAX_LAYERS = 8
_RA_STATS, _RA_INT, _RA_BLEND, _RA_AFFINE = (1, 2, 8), (4, 5, 6), (7, 8, 9, 10), 11


def check_randaug_plan(ra_i, ra_d, *, B):
    """the host-side check of a RandAugment plan (the C entry points take the tables as unchecked device data): ra_i integer
    [B, L, 4] = (op, resample, iarg, 0), ra_d float [B, L, 8] = (a, b, c, d, e, f, factor, 0) -> (int32, float64) numpy arrays.
    ValueError for L outside [1, 8], an op outside 0-11, an active op behind an empty slot (the ops of a view are compacted to the
    front), a resample that is not 2 (bilinear) / 3 (bicubic) on an affine op or not 0 elsewhere, a threshold / add outside
    [0, 256] or a posterize outside [0, 7], a nonzero iarg elsewhere, a coefficient that is not finite, or a nonzero reserved column."""
    import numpy as np
    ri, rd = np.asarray(ra_i), np.asarray(ra_d)
    if ri.ndim != 3 or ri.shape[0] != B or ri.shape[2] != 4 or ri.dtype.kind not in "iu" or not (1 <= ri.shape[1] <= RA_MAX_LAYERS):
        raise ValueError(f"randaug plan: integer ra_i [{B}, L <= {RA_MAX_LAYERS}, 4], got {ri.dtype} {ri.shape}")
    if rd.shape != ri.shape[:2] + (8,) or rd.dtype.kind != "f":
        raise ValueError(f"randaug plan: float ra_d {ri.shape[:2] + (8,)}, got {rd.dtype} {rd.shape}")
    ri = ri.astype(np.int64)
    op, rs, ia = ri[..., 0], ri[..., 1], ri[..., 2]
    if ((op < 0) | (op > _RA_AFFINE)).any():
        raise ValueError(f"randaug plan: op outside [0, {_RA_AFFINE}]")
    if ((op[:, :-1] == 0) & (op[:, 1:] != 0)).any():
        raise ValueError("randaug plan: the active ops of a view must be compacted to the front of its row")
    aff = op == _RA_AFFINE
    if (aff & (rs != 2) & (rs != 3)).any() or (~aff & (rs != 0)).any():
        raise ValueError("randaug plan: resample 2 (bilinear) or 3 (bicubic) on an affine op, 0 elsewhere")
    intop = np.isin(op, _RA_INT)
    if (intop & ((ia < 0) | (ia > 256))).any() or ((op == 6) & (ia > 7)).any() or (~intop & (ia != 0)).any():
        raise ValueError("randaug plan: iarg in [0, 256] for solarize / solarize-add, [0, 7] for posterize, 0 elsewhere")
    if ri[..., 3].any() or rd[..., 7].any():
        raise ValueError("randaug plan: the last column of ra_i and of ra_d is reserved and must be 0")
    if not np.isfinite(rd).all():
        raise ValueError("randaug plan: coefficients must be finite")
    return np.ascontiguousarray(ri, dtype=np.int32), np.ascontiguousarray(rd, dtype=np.float64)


def randaug_rows(ra_i, *, Bs, num_sample):
    """the clip of the work tensor [Bs + 2 * B, ...] every view of a (checked, compacted) plan ends in: its source clip with no
    active op, the first view region with an odd number of them, the second with an even number -> int32 [B]"""
    import numpy as np
    B = Bs * num_sample
    k = (np.asarray(ra_i)[:, :, 0] != 0).sum(axis=1)
    return np.where(k == 0, np.arange(B) // num_sample, Bs + np.where(k % 2 == 1, 0, B) + np.arange(B)).astype(np.int32)


class RandaugTable:
    """a checked RandAugment plan on the device, with what the host needs to launch its layers: ra_i / ra_d the device tables,
    L the layers, stats[j] / active[j] whether some view's op in layer j needs frame statistics / is an op at all, rows[b] the
    clip of the work tensor [Bs + 2 * B, ...] view b ends in (include/tvts_hip.h)"""

    def __init__(self, ra_i, ra_d, *, Bs, num_sample, device="cuda"):
        import numpy as np
        B = Bs * num_sample
        if Bs < 1 or num_sample < 1:
            raise ValueError("randaug plan: Bs >= 1 and num_sample >= 1")
        ri, rd = check_randaug_plan(ra_i, ra_d, B=B)
        self.Bs, self.B, self.num_sample, self.L = Bs, B, num_sample, ri.shape[1]
        self.stats = [bool(np.isin(ri[:, j, 0], _RA_STATS).any()) for j in range(self.L)]
        self.active = [bool((ri[:, j, 0] != 0).any()) for j in range(self.L)]
        self.rows = randaug_rows(ri, Bs=Bs, num_sample=num_sample)
        self.ra_i, self.ra_d = torch.from_numpy(ri).to(device), torch.from_numpy(rd).to(device)


def randaug_u8(work, table, hist=None):
    """RandAugment on the device: work uint8 [Bs + 2 * B, T, H0, W0, 3] with the source clips in its first Bs rows, table a
    RandaugTable; runs the layers (tvts_randaug_hist only for a layer where some view's op needs statistics, tvts_randaug_apply only
    while some view is still active) on the current stream, nothing synchronises with the host.  View b ends in work[table.rows[b]].
    hist: optional uint32 (int32 storage) scratch [B, T, 4, 256]; allocated when a layer needs it and none is given."""
    n, T, H0, W0 = _u8_clips(work)
    Bs, B, ns, L = table.Bs, table.B, table.num_sample, table.L
    assert n == Bs + 2 * B, "work: [Bs + 2 * B, T, H0, W0, 3]"
    if H0 < 3 or W0 < 3:
        raise ValueError("RandAugment needs frames of at least 3 x 3")
    if any(table.stats):
        if hist is None:
            hist = torch.empty((B, T, 4, 256), dtype=torch.int32, device=work.device)
        assert hist.dtype == torch.int32 and hist.is_contiguous() and hist.numel() >= B * T * 1024
    lib = _lib.load()
    for j in range(L):
        if not table.active[j]:
            break
        if table.stats[j]:
            _chk(lib.tvts_randaug_hist(_p(work), Bs, B, ns, T, H0, W0, j, L, _p(table.ra_i), _p(hist), _stream()), "tvts_randaug_hist")
        _chk(lib.tvts_randaug_apply(_p(work), Bs, B, ns, T, H0, W0, j, L, _p(table.ra_i), _p(table.ra_d),
                                    _p(hist) if table.stats[j] else None, _stream()), "tvts_randaug_apply")
    return table.rows


def check_view_plan(view_i, *, Bs, Tsrc, H0, W0, T, img):
    """the host-side check of a test-view table (the C entry point takes it as unchecked device data): view_i integer [B, 8] =
    (src, t0, tstep, top, left, 0, 0, 0) -> int32 numpy array.  ValueError for a src outside [0, Bs), t0 < 0, tstep < 1, a last frame
    t0 + (T - 1) * tstep outside the Tsrc frames of the clip, a crop that leaves the H0 x W0 frame, or a nonzero reserved column."""
    import numpy as np
    vi = np.asarray(view_i)
    if vi.ndim != 2 or vi.shape[0] < 1 or vi.shape[1] != 8 or vi.dtype.kind not in "iu":
        raise ValueError(f"view plan: integer view_i [B, 8], got {vi.dtype} {vi.shape}")
    if T < 1 or H0 < img or W0 < img:
        raise ValueError(f"view plan: T >= 1 and source frames of at least {img} x {img}, got T = {T}, {H0} x {W0}")
    vi = vi.astype(np.int64)
    if ((vi[:, 0] < 0) | (vi[:, 0] >= Bs)).any():
        raise ValueError(f"view plan: src outside [0, {Bs})")
    if (vi[:, 1] < 0).any() or (vi[:, 2] < 1).any():
        raise ValueError("view plan: t0 >= 0 and tstep >= 1")
    if (vi[:, 1] + (T - 1) * vi[:, 2] >= Tsrc).any():
        raise ValueError(f"view plan: t0 + (T - 1) * tstep must stay below Tsrc = {Tsrc} (T = {T})")
    for col, size, ax in ((3, H0, "top"), (4, W0, "left")):
        if ((vi[:, col] < 0) | (vi[:, col] + img > size)).any():
            raise ValueError(f"view plan: crop needs 0 <= {ax} and {ax} + {img} <= {size}")
    if vi[:, 5:].any():
        raise ValueError("view plan: columns 5-7 are reserved and must be 0")
    return np.ascontiguousarray(vi, dtype=np.int32)


def view_table(view_i, *, Bs, Tsrc, H0, W0, T, img, device="cuda"):
    """check_view_plan, then the upload -> view_i int32 [B, 8] on the device, as tvts_patch_gather_tube_u8_view reads it"""
    return torch.from_numpy(check_view_plan(view_i, Bs=Bs, Tsrc=Tsrc, H0=H0, W0=W0, T=T, img=img)).to(device)


def patch_gather_tube_u8_view(frames, keep, out, view, *, B, tubes, tubelet, n, img, patch, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """v1 tubelet im2col of the test views of uint8 source clips: frames uint8 [Bs, Tsrc, H0, W0, 3] on the device, view the device
    table of view_table() for B samples (each names its source clip, its first frame, the frame stride and the crop offset);
    keep int32 [B, tubes, n] -> out bf16 [B*tubes*n, 3*tubelet*patch^2], the bytes of patch_gather_tube_u8 on the host-sliced clips"""
    Bs, Tsrc, H0, W0 = _u8_clips(frames)
    assert view.dtype == torch.int32 and view.is_contiguous() and tuple(view.shape) == (B, 8), "view: int32 [B, 8] from view_table()"
    _tube_rows(keep, out, B=B, tubes=tubes, n=n)
    _chk(_lib.load().tvts_patch_gather_tube_u8_view(_p(frames), Bs, Tsrc, H0, W0, _p(view), _p(keep), B, tubes, tubelet, n, img, patch,
                                                    *_norm3(mean, std), _p(out), _ld(out), _stream()), "tvts_patch_gather_tube_u8_view")


# ---- Resize + crop of the v1 pretraining transform on uint8 source clips (embed.hip: tvts_resize_crop_u8)
_RESIZE_TABLES = {}


def resize_table(n_in, n_out):
    """the int32 table of one axis as tvts_resize_crop_u8 reads it: (n_in, n_out, ksize, 0) | first[n_out] | count[n_out] |
    taps[n_out][ksize] from transforms.pil_bilinear_coeffs, cached per (n_in, n_out) -> 1-D numpy int32"""
    import numpy as np
    key = (int(n_in), int(n_out))
    t = _RESIZE_TABLES.get(key)
    if t is None:
        from .data_loader.transforms import pil_bilinear_coeffs
        rows = pil_bilinear_coeffs(*key)
        ks = max(len(k) for _, k in rows)
        taps = np.zeros((key[1], ks), dtype=np.int32)
        for i, (_, k) in enumerate(rows):
            taps[i, :len(k)] = k
        t = _RESIZE_TABLES[key] = np.concatenate([np.array([key[0], key[1], ks, 0], dtype=np.int32),
                                                  np.array([f for f, _ in rows], dtype=np.int32),
                                                  np.array([len(k) for _, k in rows], dtype=np.int32), taps.reshape(-1)])
        t.setflags(write=False)
    return t


def resize_plan(sizes, crops, *, size, img, T, offsets=None):
    """the host half of tvts_resize_crop_u8 for a batch of source clips: sizes B x (Hs, Ws); crops B x (top, left) in RESIZED
    coordinates or None (the centre crop of every clip: CenterCrop's round-half-to-even offsets, the rule of tvts_patch_gather_tube_u8
    with crop = NULL); size: video_transform.Resize(size); offsets: the clips' byte offsets in the packed buffer (default: back to
    back) -> dict(desc int64 [B, 8], tables int32, numpy; offsets; nbytes: what the clips occupy; tmp_rows).  ValueError by name for
    a resized side below img and a crop outside the resized frame (check_resize_plan)."""
    import numpy as np
    from .data_loader.transforms import centre_crop_offset, resize_sizes
    B = len(sizes)
    desc = np.zeros((B, 8), dtype=np.int64)
    where, parts, total, at = {}, [], 0, 0
    for b, (hs, ws) in enumerate(sizes):
        hs, ws = int(hs), int(ws)
        if hs < 1 or ws < 1:
            raise ValueError(f"resize plan: clip {b} has frames of {hs} x {ws}")
        nh, nw = resize_sizes(hs, ws, int(size))
        if nh < img or nw < img:
            raise ValueError(f"resize plan: clip {b} ({hs} x {ws}) resizes to {nh} x {nw} under Resize({size}), below the crop of "
                             f"{img} x {img}")
        loc = []
        for key in ((hs, nh), (ws, nw)):
            if key not in where:
                where[key] = total
                parts.append(resize_table(*key))
                total += parts[-1].size
            loc.append(where[key])
        top, left = (centre_crop_offset(nh - img), centre_crop_offset(nw - img)) if crops is None else (int(crops[b][0]), int(crops[b][1]))
        off = at if offsets is None else int(offsets[b])
        desc[b] = (off, hs, ws, top, left, loc[0], loc[1], 0)
        at = off + T * hs * ws * 3
    tables = np.concatenate(parts)
    nbytes = int(max(desc[:, 0] + T * desc[:, 1] * desc[:, 2] * 3))
    return dict(desc=desc, tables=tables, offsets=desc[:, 0].copy(), nbytes=nbytes,
                tmp_rows=check_resize_plan(desc, tables, T=T, img=img, src_bytes=nbytes))


def check_resize_plan(desc, tables, *, T, img, src_bytes):
    """the host-side check of a resize plan (the C entry point takes both as unchecked device data): desc integer [B, 8] = (offset,
    Hs, Ws, top, left, ytab, xtab, 0), tables int32 -> tmp_rows, the largest row span of a crop window (the size rule of the entry
    point's tmp).  ValueError for a clip that leaves the src_bytes of the packed buffer, a table location outside `tables`, a table
    that is not the one of its (n_in, n_out) or whose n_in is not the clip's side, a resized side below img, a crop outside the
    resized frame (0 <= top <= new_h - img, 0 <= left <= new_w - img) or a nonzero reserved column."""
    import numpy as np
    d, tb = np.asarray(desc), np.asarray(tables)
    if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] != 8 or d.dtype.kind not in "iu" or tb.ndim != 1 or tb.dtype != np.int32:
        raise ValueError(f"resize plan: integer desc [B, 8] and int32 tables [n], got {d.dtype} {d.shape} / {tb.dtype} {tb.shape}")
    if T < 1 or img < 1:
        raise ValueError(f"resize plan: T = {T}, img = {img}")
    d = d.astype(np.int64)
    tmp_rows, seen = 1, {}
    for b, (off, hs, ws, top, left, yt, xt, zero) in enumerate(d.tolist()):
        if hs < 1 or ws < 1 or off < 0 or off + T * hs * ws * 3 > src_bytes:
            raise ValueError(f"resize plan: clip {b} ({T} x {hs} x {ws} x 3 bytes at offset {off}) leaves the buffer of {src_bytes} bytes")
        if zero:
            raise ValueError("resize plan: column 7 is reserved and must be 0")
        for loc, n_in, at, ax in ((yt, hs, top, "top"), (xt, ws, left, "left")):
            if loc not in seen:
                if loc < 0 or loc + 4 > tb.size:
                    raise ValueError(f"resize plan: clip {b} names a table at {loc}, outside the {tb.size} table elements")
                t_in, n_out = int(tb[loc]), int(tb[loc + 1])
                want = resize_table(t_in, n_out) if t_in >= 1 and n_out >= 1 else None
                if want is None or loc + want.size > tb.size or not np.array_equal(tb[loc:loc + want.size], want):
                    raise ValueError(f"resize plan: the table at {loc} is not pil_bilinear_coeffs({t_in}, {n_out})")
                seen[loc] = (t_in, n_out, want)
            t_in, n_out, want = seen[loc]
            if t_in != n_in:
                raise ValueError(f"resize plan: clip {b} has a side of {n_in}, its table resamples {t_in}")
            if n_out < img:
                raise ValueError(f"resize plan: clip {b} resizes to a side of {n_out}, below the crop of {img}")
            if at < 0 or at > n_out - img:
                raise ValueError(f"resize plan: clip {b}: crop outside the resized frame, needs 0 <= {ax} <= {n_out - img}, got {at}")
            if ax == "top":
                first, count = want[4:4 + n_out], want[4 + n_out:4 + 2 * n_out]
                tmp_rows = max(tmp_rows, int(first[at + img - 1] + count[at + img - 1] - first[at]))
    return tmp_rows


def resize_crop_u8(src, desc, tables, tmp, out, *, B, T, img, tmp_rows):
    """Pillow's 8-bit bilinear Resize + crop on the device: src uint8 [nbytes], the packed source clips; desc int64 [B, 8] and tables
    int32, the device copies of a resize_plan(); tmp uint8 with >= B * T * tmp_rows * img * 3 elements; out uint8 [B, T, img, img, 3]
    (or a row-strided 2-D view [B * T * img, 3 * img] of a wider buffer)"""
    assert src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous() and tmp.dtype == torch.uint8 and tmp.is_contiguous()
    assert desc.dtype == torch.int64 and desc.is_contiguous() and tuple(desc.shape) == (B, 8) and tables.dtype == torch.int32
    assert out.dtype == torch.uint8
    if out.dim() == 2:
        assert tuple(out.shape) == (B * T * img, 3 * img)
        ldo = _ld(out)
    else:
        assert out.is_contiguous() and tuple(out.shape) == (B, T, img, img, 3)
        ldo = 3 * img
    _chk(_lib.load().tvts_resize_crop_u8(_p(src), _p(desc), _p(tables), B, T, img, tmp_rows, _p(tmp), tmp.numel(), _p(out), ldo,
                                         _stream()), "tvts_resize_crop_u8")


def text_embed(ids, emb, pos, x, *, N, L):
    lib = _lib.load()
    assert ids.dtype == torch.int32
    _chk(lib.tvts_text_embed(_p(ids), ids.stride(0), N, L, _p(emb), _p(pos), emb.shape[1], _p(x), _ld(x), _stream()),
         "tvts_text_embed")


def text_embed_packed(ids, seq_start, emb, pos, x, *, N):
    """x[r] = emb[ids[r]] + pos[r - seq_start[i]] for packed captions: ids int32 [M], seq_start int32 [N + 1] on the device."""
    lib = _lib.load()
    assert ids.dtype == torch.int32 and seq_start.dtype == torch.int32 and seq_start.numel() == N + 1
    M = ids.numel()
    assert x.shape[0] == M
    _chk(lib.tvts_text_embed_packed(_p(ids), _p(seq_start), N, M, _p(emb), _p(pos), emb.shape[1], emb.shape[0], pos.shape[0], _p(x),
                                    _ld(x), _stream()), "tvts_text_embed_packed")


def token_sort(ids_cpu):
    """(order, seg) of tvts_text_embed_bwd for the [N, L] token ids of a batch (host tensors in, int32 host tensors out): the rows
    grouped into runs of equal token id (rows of a run in row order) and the starts of the runs padded to N * L + 1 entries.  The
    runs of more than 64 rows come first (the kernel gives each of the first 64 runs a block per 64 columns), the others by id.
    numpy on the host: ~1 ms for the 24 576 tokens of a 192-pair batch (it runs once per step in the trainer's prepare_batch)."""
    import numpy as np
    flat = ids_cpu.reshape(-1).numpy().astype(np.int64, copy=False)
    n = flat.size
    order = np.argsort(flat, kind="stable")
    srt = flat[order]
    first = np.empty(n, dtype=bool)
    first[0] = True
    np.not_equal(srt[1:], srt[:-1], out=first[1:])
    starts = np.flatnonzero(first)
    lens = np.diff(np.append(starts, n))
    if (lens > 64).any():  # long runs to the front: stable, so the others stay in id order
        run_of = np.cumsum(first) - 1                                  # run index of every sorted row
        order = order[np.argsort(lens[run_of] <= 64, kind="stable")]   # rows of long runs first
        lens = lens[np.argsort(lens <= 64, kind="stable")]
        starts = np.cumsum(lens) - lens
    seg = np.full(n + 1, n, dtype=np.int32)
    seg[:starts.size] = starts
    return torch.from_numpy(order.astype(np.int32)), torch.from_numpy(seg)


def text_embed_bwd(dx, ids, demb, dpos, *, N, L, tok_sort=None):
    """tok_sort = (order, seg) device tensors of token_sort(): ordered sums; None: fp32 atomics."""
    lib = _lib.load()
    order, seg = tok_sort if tok_sort is not None else (None, None)
    if order is not None:
        assert order.dtype == torch.int32 and seg.dtype == torch.int32 and order.numel() == N * L and seg.numel() == N * L + 1
    _chk(lib.tvts_text_embed_bwd(_p(dx), _ld(dx), _p(ids), ids.stride(0), N, L, dx.shape[1], _p(demb), _p(dpos),
                                 _p(order), _p(seg), _stream()), "tvts_text_embed_bwd")


def pack_captions(ids_cpu, context=None, lens=None):
    """The host half of the packed text tower: [N, L] token ids (a host tensor; the EOT token is each row's largest id,
    CLIP/clip/model.py:343-354) -> the descriptors of the packed batch, all host tensors, no device access:
    ids int32 [M] (caption i's tokens up to and including its EOT, captions in the given order), seq_start int32 [N + 1],
    eot_rows int32 [N] (= seq_start[1:] - 1), cls_rows int32 [N] (= seq_start[:-1]), max_len (int), tok_order / tok_seg (token_sort of
    the packed ids) and pos_order int32 [M] / pos_seg int32 [context + 1]: the rows sorted stably by their position inside their
    caption and the starts of the runs of equal position (context: the rows of the positional table, default L).
    lens (host integers [N], optional): pack caption i's first lens[i] tokens instead of the CLIP rule -- the right-padded captions of
    a tokenizer with their attention-mask sums (the kv_len of tokenizer_inputs: the DistilBERT tower of v1)."""
    import numpy as np
    assert ids_cpu.dim() == 2 and ids_cpu.shape[0] > 0 and ids_cpu.shape[1] > 0 and not ids_cpu.is_cuda
    a = ids_cpu.numpy()
    N, L = a.shape
    context = L if context is None else int(context)
    if lens is None:
        lens = a.argmax(axis=1).astype(np.int64) + 1
    else:
        lens = np.asarray(lens.numpy() if isinstance(lens, torch.Tensor) else lens).astype(np.int64).reshape(-1)
        if lens.size != N or int(lens.min()) < 1 or int(lens.max()) > L:
            raise ValueError(f"lens: expected {N} caption lengths in [1, {L}]")
    if int(lens.max()) > context:
        raise ValueError(f"a caption of {int(lens.max())} tokens does not fit the context of {context}")
    seq_start = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lens, out=seq_start[1:])
    M = int(seq_start[N])
    pos = np.arange(M, dtype=np.int64) - np.repeat(seq_start[:-1], lens)
    ids = a[np.repeat(np.arange(N), lens), pos].astype(np.int32)
    pos_seg = np.zeros(context + 1, dtype=np.int64)
    np.cumsum(np.bincount(pos, minlength=context), out=pos_seg[1:])
    tok_order, tok_seg = token_sort(torch.from_numpy(ids))
    i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32))  # noqa: E731
    return dict(ids=torch.from_numpy(ids), seq_start=i32(seq_start), eot_rows=i32(seq_start[1:] - 1), cls_rows=i32(seq_start[:-1]),
                max_len=int(lens.max()), tok_order=tok_order, tok_seg=tok_seg, pos_order=i32(np.argsort(pos, kind="stable")),
                pos_seg=i32(pos_seg))


def text_embed_bwd_packed(dx, ids, seq_start, demb, dpos, *, N, tok_sort, pos_sort):
    """demb[ids[r]] += dx[r], dpos[r - seq_start[seq(r)]] += dx[r] over the M packed rows as ordered sums (no atomic form):
    tok_sort = (tok_order, tok_seg), pos_sort = (pos_order, pos_seg) device tensors of pack_captions()."""
    lib = _lib.load()
    M = ids.numel()
    (to, ts), (po, ps) = tok_sort, pos_sort
    assert ids.dtype == torch.int32 and seq_start.dtype == torch.int32 and seq_start.numel() == N + 1 and dx.shape[0] >= M
    assert all(t.dtype == torch.int32 for t in (to, ts, po, ps))
    assert to.numel() == M and ts.numel() == M + 1 and po.numel() == M and ps.numel() == dpos.shape[0] + 1
    _chk(lib.tvts_text_embed_bwd_packed(_p(dx), _ld(dx), _p(ids), _p(seq_start), N, M, dx.shape[1], demb.shape[0], dpos.shape[0],
                                        _p(demb), _p(dpos), _p(to), _p(ts), _p(po), _p(ps), _stream()), "tvts_text_embed_bwd_packed")


def text_mean(t, mean, before, *, NT, B):
    lib = _lib.load()
    _chk(lib.tvts_text_mean(_p(t), NT, B, t.shape[1], _p(mean), _p(before), _stream()), "tvts_text_mean")


def text_mean_bwd(dmean, dt, *, NT, B):
    lib = _lib.load()
    _chk(lib.tvts_text_mean_bwd(_p(dmean), NT, B, dmean.shape[1], _p(dt), _stream()), "tvts_text_mean_bwd")


def sort_assemble(tok, text, type_embed, xs, *, B, S, off, Sv, NT):
    lib = _lib.load()
    _chk(lib.tvts_sort_assemble(_p(tok), _ld(tok), B, S, off, Sv, _p(text), NT, _p(type_embed), xs.shape[1], _p(xs),
                                _ld(xs), _stream()), "tvts_sort_assemble")


def sort_assemble_bwd(dxs, dvid, dout, dtype, *, B, S, off, Sv, NT):
    lib = _lib.load()
    E = dout.shape[1]
    ws = _tn_workspace(dout.device)  # ordered partials of the type-embedding gradient
    _chk(lib.tvts_sort_assemble_bwd(_p(dxs), _ld(dxs) if dxs is not None else 0, B, S, off, Sv, NT, _p(dvid), E,
                                    _p(dout), _ld(dout), _p(dtype), _p(ws), ws.numel(), _stream()), "tvts_sort_assemble_bwd")


def relu(x, out, dy=None):
    """out = relu(x), or with dy: out = dy * (x > 0)"""
    lib = _lib.load()
    _chk(lib.tvts_relu(_p(x), _p(dy), _p(out), x.numel(), _stream()), "tvts_relu")


def rows_gather(src, rows, dst, *, scatter_add=False):
    lib = _lib.load()
    _chk(lib.tvts_rows_gather(_p(src), _ld(src), _p(rows), rows.numel(), src.shape[1], _p(dst), _ld(dst),
                              int(scatter_add), _stream()), "tvts_rows_gather")


def rows_move(mode, rows, *, full_f32=None, full_bf16=None, packed_f32=None, packed_bf16=None):
    """mode "gather": packed[r] = full[rows[r]] (from full_f32 if given, else full_bf16); "scatter": full[rows[r]] = packed[r];
    "scatter_add": full_f32[rows[r]] += packed_f32[r], full_bf16[rows[r]] = bf16(sum).  rows int32, distinct."""
    lib = _lib.load()
    assert rows.dtype == torch.int32
    for t, dt in ((full_f32, torch.float32), (packed_f32, torch.float32), (full_bf16, torch.bfloat16), (packed_bf16, torch.bfloat16)):
        assert t is None or (t.dtype == dt and t.stride(1) == 1)
    ref = packed_f32 if packed_f32 is not None else packed_bf16
    W = ref.shape[1]
    ld = lambda t: _ld(t) if t is not None else 0  # noqa: E731
    _chk(lib.tvts_rows_move({"gather": 0, "scatter": 1, "scatter_add": 2}[mode], _p(rows), rows.numel(), W, _p(full_f32), ld(full_f32),
                            _p(full_bf16), ld(full_bf16), _p(packed_f32), ld(packed_f32), _p(packed_bf16), ld(packed_bf16), _stream()),
         "tvts_rows_move")


def zero_cols_bf16(x, cols):
    """x[:, :cols] = 0 (bf16, row-major)"""
    lib = _lib.load()
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    _chk(lib.tvts_zero_cols_bf16(_p(x), _ld(x), x.shape[0], int(cols), _stream()), "tvts_zero_cols_bf16")


def l2norm_rows(x, xn, inv, eps=1e-8):
    lib = _lib.load()
    _chk(lib.tvts_l2norm_rows(_p(x), x.shape[0], x.shape[1], eps, _p(xn), _p(inv), _stream()), "tvts_l2norm_rows")


def l2norm_rows_bwd(dxn, xn, inv, dx):
    lib = _lib.load()
    _chk(lib.tvts_l2norm_rows_bwd(_p(dxn), _p(xn), _p(inv), xn.shape[0], xn.shape[1], _p(dx), _stream()),
         "tvts_l2norm_rows_bwd")


def mc_logits(text, video, logits):
    """logits[b, c] = 100 * cos(video[b], text[c, b]): text fp32 [C, B, E], video fp32 [B, E], logits fp32 [B, C]"""
    lib = _lib.load()
    C, B, E = text.shape
    assert text.dtype == video.dtype == logits.dtype == torch.float32
    assert text.is_contiguous() and video.is_contiguous() and logits.is_contiguous()
    assert tuple(video.shape) == (B, E) and tuple(logits.shape) == (B, C)
    _chk(lib.tvts_mc_logits(_p(text), _p(video), C, B, E, _p(logits), _stream()), "tvts_mc_logits")


def infonce(x, lse, dx, loss):
    lib = _lib.load()
    _chk(lib.tvts_infonce(_p(x), x.shape[0], _p(lse), _p(dx), _p(loss), _stream()), "tvts_infonce")


def cross_entropy(logits, labels, scale, dlogits, loss):
    lib = _lib.load()
    assert labels.dtype == torch.int32
    _chk(lib.tvts_cross_entropy(_p(logits), _p(labels), logits.shape[0], logits.shape[1], scale, _p(dlogits), _p(loss),
                                _stream()), "tvts_cross_entropy")


def retrieval_ranks(sims, mode, valid=None):
    """ranks of the ground truth per query of a text x video similarity matrix; mode 't2v' | 'v2t';
    valid: optional uint8 [n_text], 0 where a caption is missing (the reference's query_masks)."""
    lib = _lib.load()
    assert sims.dtype == torch.float32 and sims.dim() == 2 and sims.stride(1) == 1
    nt, nv = sims.shape
    ranks = torch.empty(nt if mode == "t2v" else nv, dtype=torch.float32, device=sims.device)
    assert valid is None or (valid.dtype == torch.uint8 and valid.numel() == nt and valid.is_contiguous())
    _chk(lib.tvts_retrieval_ranks(_p(sims), sims.stride(0), nt, nv, 0 if mode == "t2v" else 1, _p(valid), _p(ranks), _stream()),
         "tvts_retrieval_ranks")
    return ranks


def v2v_ranks(sims, q0, labels, ranks=None, N=None):
    """label-matched video-to-video ranks (v1/downstream/run_class_zero.py:344-413): row i of sims fp32 [nq, >= N] = query video
    q0 + i against all N videos (its own entry is read as -1000), labels int32 [N] -> ranks fp32 [nq] = the number of
    other-label videos scoring above the best same-label one."""
    lib = _lib.load()
    assert sims.dtype == torch.float32 and sims.dim() == 2 and sims.stride(1) == 1
    assert labels.dtype == torch.int32 and labels.is_contiguous()
    N = labels.numel() if N is None else N
    nq = sims.shape[0]
    assert sims.shape[1] >= N and labels.numel() >= N
    if ranks is None:
        ranks = torch.empty(nq, dtype=torch.float32, device=sims.device)
    assert ranks.dtype == torch.float32 and ranks.is_contiguous() and ranks.numel() >= nq
    _chk(lib.tvts_v2v_ranks(_p(sims), sims.stride(0), nq, int(q0), N, _p(labels), _p(ranks), _stream()), "tvts_v2v_ranks")
    return ranks


def _adamw_bytes(chunk_group, ngroups):
    """30 B per element of every chunk that steps (group byte < ngroups): p, m, v read + written (24), g read (4), bf16 shadow
    written (2)"""
    assert chunk_group.dtype == torch.uint8
    return lambda: 30.0 * 1024 * float((chunk_group < ngroups).sum())


def adamw_hf(p, g, m, v, shadow, chunk_group, lr4, wd4, step, beta1=0.9, beta2=0.999, eps=1e-6, grad_scale=1.0,
             step_dev=None, hyper_dev=None):
    lib = _lib.load()
    lr = (ctypes.c_float * 4)(*lr4)
    wd = (ctypes.c_float * 4)(*wd4)
    with _hbm("adamw", _adamw_bytes(chunk_group, 255)):
        rc = (lib.tvts_adamw_hf(_p(p), _p(g), _p(m), _p(v), _p(shadow), _p(chunk_group), chunk_group.numel(),
                           ctypes.cast(lr, ctypes.c_void_p), ctypes.cast(wd, ctypes.c_void_p), step, _p(step_dev), _p(hyper_dev), beta1, beta2, eps,
                           grad_scale, _stream()))
    _chk(rc, "tvts_adamw_hf")


def adamw_hf_guarded(p, g, m, v, shadow, chunk_group, lr4, wd4, step, beta1=0.9, beta2=0.999, eps=1e-6, grad_scale=1.0,
                     step_dev=None, hyper_dev=None, norm_coef=None, skipped=None):
    """adamw_hf for the pretraining step with clipping and the overflow guard (tvts_adamw_hf_guarded).  norm_coef (device fp32 [2],
    what grad_sumsq left): g = stored g * grad_scale * norm_coef[1]; None, or a coefficient of 1.0: the bits of adamw_hf.  skipped
    (device int64, with step_dev and norm_coef): the guard as adamw_torch describes it; `step` is then ignored."""
    n = chunk_group.numel()
    assert chunk_group.dtype == torch.uint8 and all(t.dtype == torch.float32 and t.numel() >= n * 1024 for t in (p, g, m, v))
    assert shadow is None or (shadow.dtype == torch.bfloat16 and shadow.numel() >= n * 1024)
    assert hyper_dev is None or (hyper_dev.dtype == torch.float32 and hyper_dev.numel() >= 8)
    assert norm_coef is None or (norm_coef.dtype == torch.float32 and norm_coef.numel() >= 2)
    assert step_dev is None or (step_dev.dtype == torch.int32 and step_dev.numel() >= 1)
    if skipped is not None:
        if step_dev is None or norm_coef is None:
            raise ValueError("skipped (the guarded launch) needs step_dev and norm_coef")
        _guard_cells(step_dev, skipped, norm_coef)
    lr = (ctypes.c_float * 4)(*lr4)
    wd = (ctypes.c_float * 4)(*wd4)
    with _hbm("adamw", _adamw_bytes(chunk_group, 255)):
        rc = _lib.load().tvts_adamw_hf_guarded(_p(p), _p(g), _p(m), _p(v), _p(shadow), _p(chunk_group), n, ctypes.cast(lr, ctypes.c_void_p),
                                               ctypes.cast(wd, ctypes.c_void_p), int(step), _p(step_dev), _p(hyper_dev), beta1, beta2, eps,
                                               grad_scale, _p(norm_coef), _p(skipped), _stream())
    _chk(rc, "tvts_adamw_hf_guarded")


def ema_pair(decay):
    """(d32, o32) of timm's ModelEma rule ``ema * decay + (1. - decay) * p`` on fp32 tensors with a Python-float decay, as Python
    floats that hold fp32 values: d32 = fp32(decay), o32 = fp32(1.0 - decay) with the difference formed in DOUBLE and rounded once
    (fp32(1) - d32 is another number: 1.00016594e-4 instead of 9.99999975e-5 at decay 0.9999)"""
    decay = float(decay)
    if not (0.0 <= decay <= 1.0):
        raise ValueError(f"decay {decay!r}: expected a number in [0, 1]")
    return ctypes.c_float(decay).value, ctypes.c_float(1.0 - decay).value  # (the C cast: round to nearest even, once each)


def _torch_rule(label, per, streams, shadow, chunk_group, hyper_dev, step_dev, norm_coef, ema, ema_decay, skipped):
    """What adamw_torch and sgd_torch share: the buffer asserts, the ema / ema_decay pairing, the guard's cells and the traffic figure
    (`per` bytes per stepped element without the average, which adds 8; under the guard an upper bound: a skipped launch moves no
    parameter bytes) -> (the _hbm context of the launch, the entry point's trailing arguments ema, d32, o32, skipped, stream)"""
    n = chunk_group.numel()
    assert chunk_group.dtype == torch.uint8 and hyper_dev.dtype == torch.float32 and hyper_dev.numel() >= 128
    assert all(t.dtype == torch.float32 and t.numel() >= n * 1024 for t in streams) and (shadow is None or shadow.numel() >= n * 1024)
    if (ema is None) != (ema_decay is None):
        raise ValueError("ema_decay without ema" if ema is None else "ema needs ema_decay")
    d32, o32 = (0.0, 0.0) if ema is None else ema_pair(ema_decay)
    assert ema is None or (ema.dtype == torch.float32 and ema.is_contiguous() and ema.numel() >= n * 1024 and ema.device == streams[0].device)
    if skipped is not None:
        if step_dev is None or norm_coef is None:
            raise ValueError("skipped (the guarded launch) needs step_dev and norm_coef")
        _guard_cells(step_dev, skipped, norm_coef)
    per += 0.0 if ema is None else 8.0
    return _hbm(label, lambda: per * 1024 * float((chunk_group < 64).sum())), (_p(ema), d32, o32, _p(skipped), _stream())


def adamw_torch(p, g, m, v, shadow, chunk_group, hyper_dev, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, step_dev=None,
                norm_coef=None, ema=None, ema_decay=None, skipped=None):
    """one torch.optim.AdamW step over the flat buffers (tvts_adamw_torch, 30 B per element); hyper_dev: device fp32 lr[64] | wd[64].
    ema (fp32, the layout of p) with ema_decay: the same pass applies ModelEma's rule to the new p (38 B per element).  skipped
    (device int64, with step_dev and norm_coef): the launch under the overflow guard -- norm_coef[0] finite: step_dev[0] += 1, then
    the update with that device step count, bit for bit; not finite: p, m, v, the shadow and the average keep every bit, step_dev
    stays, skipped[0] += 1.  `step` is then ignored."""
    hbm, tail = _torch_rule("adamw", 30.0, (p, g, m, v), shadow, chunk_group, hyper_dev, step_dev, norm_coef, ema, ema_decay, skipped)
    with hbm:
        rc = _lib.load().tvts_adamw_torch(_p(p), _p(g), _p(m), _p(v), _p(shadow), _p(chunk_group), chunk_group.numel(), _p(hyper_dev),
                                          int(step), _p(step_dev), beta1, beta2, eps, grad_scale, _p(norm_coef), *tail)
    _chk(rc, "tvts_adamw_torch")


def sgd_torch(p, g, buf, shadow, chunk_group, hyper_dev, step, momentum=0.0, nesterov=False, grad_scale=1.0, step_dev=None,
              norm_coef=None, ema=None, ema_decay=None, skipped=None):
    """one torch.optim.SGD step (dampening 0) over the flat buffers, bit for bit (tvts_sgd_torch); hyper_dev: device fp32 lr[64] |
    wd[64].  buf: the momentum buffer (None with momentum 0: not touched); step == 1 (or step_dev[0] == 1) is the first update,
    which writes buf without reading it.  ema / ema_decay / skipped as adamw_torch; a skipped first call leaves step_dev at 0, so the
    next call is then the first update.  Bytes per stepped element: p 8, g 4, shadow 2, buf 8 (4 on the first update, 0 without
    momentum), the average 8."""
    mom = ctypes.c_float(float(momentum)).value != 0.0
    hbm, tail = _torch_rule("sgd", 22.0 if mom else 14.0, (p, g) + ((buf,) if buf is not None else ()), shadow, chunk_group, hyper_dev,
                            step_dev, norm_coef, ema, ema_decay, skipped)
    with hbm:
        rc = _lib.load().tvts_sgd_torch(_p(p), _p(g), _p(buf), _p(shadow), _p(chunk_group), chunk_group.numel(), _p(hyper_dev), int(step),
                                        _p(step_dev), float(momentum), 1 if nesterov else 0, grad_scale, _p(norm_coef), *tail)
    _chk(rc, "tvts_sgd_torch")


def _guard_cells(step_dev, skipped, norm_coef):
    assert step_dev.dtype == torch.int32 and step_dev.numel() >= 1 and skipped.dtype == torch.int64 and skipped.numel() >= 1
    assert norm_coef.dtype == torch.float32 and norm_coef.numel() >= 2


def ema_update(ema, p, chunk_group, decay):
    """ModelEma.update as a pass of its own: ema = fl(fl(ema * d32) + fl(o32 * p)) on every 1024-element chunk whose group byte is
    below 64; a chunk of another group (255 = frozen / padding) keeps every bit of ema.  12 B per element."""
    n = chunk_group.numel()
    d32, o32 = ema_pair(decay)
    assert chunk_group.dtype == torch.uint8 and ema.dtype == torch.float32 and p.dtype == torch.float32
    assert ema.is_contiguous() and p.is_contiguous() and ema.numel() >= n * 1024 and p.numel() >= n * 1024
    with _hbm("ema", lambda: 12.0 * 1024 * float((chunk_group < 64).sum())):
        rc = _lib.load().tvts_ema_update(_p(ema), _p(p), _p(chunk_group), n, d32, o32, _stream())
    _chk(rc, "tvts_ema_update")


def swap_f32_shadow(a, b, shadow):
    """a <-> b in place (fp32, equal sizes, a multiple of 4 elements) and shadow = bf16(new a); no temporary buffer"""
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and shadow.dtype == torch.bfloat16
    assert a.is_contiguous() and b.is_contiguous() and shadow.is_contiguous()
    assert a.numel() == b.numel() and shadow.numel() >= a.numel() and a.device == b.device == shadow.device
    with _hbm("ema", 18.0 * a.numel()):
        rc = _lib.load().tvts_swap_f32_shadow(_p(a), _p(b), _p(shadow), a.numel(), _stream())
    _chk(rc, "tvts_swap_f32_shadow")


# ---- v1 fine-tuning step (finetune.hip; its optimizer launch, adamw_torch, is above beside adamw_hf)
def drop_path_table(seed, p_sites, scale, *, site_base=0):
    """scale [nsites, B] fp32 = the stochastic-depth draw of one step: 1 / (1 - p) for a kept sample, 0 for a dropped one, exactly
    1.0 where p_sites[s] == 0.  seed: int64 device scalar; p_sites: fp32 device [nsites]."""
    assert seed.dtype == torch.int64 and p_sites.dtype == torch.float32 and scale.dtype == torch.float32
    assert scale.dim() == 2 and scale.is_contiguous() and p_sites.is_contiguous() and p_sites.numel() == scale.shape[0]
    _chk(_lib.load().tvts_drop_path_table(_p(seed), int(site_base), _p(p_sites), scale.shape[0], scale.shape[1], _p(scale), _stream()),
         "tvts_drop_path_table")


def drop_path_rows(y, scale, S, *, residual=None, out=None, out_bf16=None):
    """out[r] = residual[r] + scale[r // S] * y[r] (fp32 and / or bf16 out); without residual: out[r] = scale[r // S] * y[r], the
    backward of the branch.  scale: fp32 [rows // S] (one row of the step's table)."""
    assert y.dtype == torch.float32 and scale.dtype == torch.float32 and scale.is_contiguous() and y.shape[0] % S == 0
    assert scale.numel() >= y.shape[0] // S
    for t, dt in ((residual, torch.float32), (out, torch.float32), (out_bf16, torch.bfloat16)):
        assert t is None or (t.dtype == dt and t.shape == y.shape)
    with _hbm("drop_path", _nb((y, y.shape[0]), (residual, y.shape[0]), (out, y.shape[0]), (out_bf16, y.shape[0]))):
        rc = _lib.load().tvts_drop_path_rows(_p(y), _ld(y), y.shape[0], y.shape[1], int(S), _p(scale), _p(residual),
                                             _ld(residual) if residual is not None else 0, _p(out), _ld(out) if out is not None else 0,
                                             _p(out_bf16), _ld(out_bf16) if out_bf16 is not None else 0, _stream())
    _chk(rc, "tvts_drop_path_rows")


def soft_ce(logits, loss_acc, ws, *, soft_targets=None, labels=None, smoothing=0.0, scale=1.0, dlogits=None, hits=None):
    """loss_acc[0] += scale * CE(logits, targets) (soft targets fp32 [B, C], or int32 labels + smoothing); dlogits / hits optional.
    ws: fp32 scratch of >= 2 B elements."""
    B, C = logits.shape
    assert logits.dtype == torch.float32 and loss_acc.dtype == torch.float32 and ws.dtype == torch.float32 and ws.numel() >= 2 * B
    assert soft_targets is None or (soft_targets.dtype == torch.float32 and soft_targets.shape == logits.shape)
    assert labels is None or (labels.dtype == torch.int32 and labels.numel() == B and labels.is_contiguous())
    assert dlogits is None or (dlogits.dtype == torch.float32 and dlogits.shape == logits.shape)
    assert hits is None or hits.dtype == torch.int32
    _chk(_lib.load().tvts_soft_ce(_p(logits), _ld(logits), B, C, _p(soft_targets), _ld(soft_targets) if soft_targets is not None else 0,
                                  _p(labels), float(smoothing), float(scale), _p(loss_acc), _p(dlogits),
                                  _ld(dlogits) if dlogits is not None else 0, _p(hits), _p(ws), _stream()), "tvts_soft_ce")


def mix_targets(labels, mix, out, *, smoothing=0.0):
    """out fp32 [B, C] = the soft targets of a Mixup / CutMix step (mixup_target): labels int32 [B], mix the device table of
    mix_table(); feeds soft_ce(soft_targets=out)"""
    B, C = out.shape
    mi, mf = _mix_dev(mix, B)
    assert labels.dtype == torch.int32 and labels.numel() == B and labels.is_contiguous() and out.dtype == torch.float32
    _chk(_lib.load().tvts_mix_targets(_p(labels), _p(mi), _p(mf), B, C, float(smoothing), _p(out), _ld(out), _stream()),
         "tvts_mix_targets")


def class_ranks(x, labels, ranks=None):
    """ranks int32 [R] of the label's logit in every row of x fp32 [R, C] (row stride >= C): the number of classes that score
    higher, plus the equal ones with a lower index -- `ranks < k` is the top-k hit, `ranks == 0` is argmax == label.  labels int32
    [R] on the device; the caller has checked them on the host (a label outside [0, C) gets rank C)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    R, C = x.shape
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == R
    if ranks is None:
        ranks = torch.empty(R, dtype=torch.int32, device=x.device)
    assert ranks.dtype == torch.int32 and ranks.is_contiguous() and ranks.numel() >= R
    _chk(_lib.load().tvts_class_ranks(_p(x), x.stride(0), R, C, _p(labels), _p(ranks), _stream()), "tvts_class_ranks")
    return ranks


def view_sum(view_logits, seen, out, count):
    """out fp32 [N, C] = the sum of the seen views of view_logits fp32 [N, V, C] in the order v = 0 .. V - 1 (seen uint8 [N, V]),
    count int32 [N] = the number of seen views; a video without one gets a zero row"""
    N, V, C = view_logits.shape
    assert view_logits.dtype == torch.float32 and view_logits.is_contiguous()
    assert seen.dtype == torch.uint8 and seen.is_contiguous() and tuple(seen.shape) == (N, V)
    assert out.dtype == torch.float32 and tuple(out.shape) == (N, C) and out.stride(1) == 1
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() == N
    _chk(_lib.load().tvts_view_sum(_p(view_logits), _p(seen), N, V, C, _p(out), out.stride(0), _p(count), _stream()), "tvts_view_sum")


def view_store(logits, slot, labels, view_logits, seen, video_labels):
    """the rows of logits fp32 [B, C] into their view slots (slot int32 [B] = video * V + view) of view_logits fp32 [N, V, C]; a
    slot that is seen already, or named by an earlier row of the batch, keeps what it has.  labels int32 [B] -> video_labels [N]."""
    N, V, C = view_logits.shape
    B = logits.shape[0]
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[1] == C and logits.stride(1) == 1
    assert view_logits.dtype == torch.float32 and view_logits.is_contiguous()
    assert seen.dtype == torch.uint8 and seen.is_contiguous() and tuple(seen.shape) == (N, V)
    for t in (slot, labels):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B
    assert video_labels.dtype == torch.int32 and video_labels.is_contiguous() and video_labels.numel() == N
    _chk(_lib.load().tvts_view_store(_p(logits), logits.stride(0), B, C, _p(slot), _p(labels), N, V, _p(view_logits), _p(seen),
                                     _p(video_labels), _stream()), "tvts_view_store")


def grad_sumsq(g, chunk_group, partial, norm_coef, *, max_norm=0.0, grad_scale=1.0):
    """norm_coef[0] = the global norm of the gradient chunks whose group is not 255, norm_coef[1] = the clip coefficient
    min(1, max_norm / (norm + 1e-6)) (1 with max_norm <= 0); everything stays on the device."""
    n = chunk_group.numel()
    assert g.dtype == torch.float32 and g.is_contiguous() and g.numel() >= n * 1024 and chunk_group.dtype == torch.uint8
    assert partial.dtype == torch.float32 and partial.numel() >= n and norm_coef.dtype == torch.float32 and norm_coef.numel() >= 2
    _chk(_lib.load().tvts_grad_sumsq(_p(g), _p(chunk_group), n, _p(partial), float(max_norm or 0.0), float(grad_scale), _p(norm_coef),
                                     _stream()), "tvts_grad_sumsq")


def cast_f32_bf16(src, dst):
    lib = _lib.load()
    _chk(lib.tvts_cast_f32_bf16(_p(src), _p(dst), src.numel(), _stream()), "tvts_cast_f32_bf16")


def cast_bf16_f32(src, dst):
    lib = _lib.load()
    _chk(lib.tvts_cast_bf16_f32(_p(src), _p(dst), src.numel(), _stream()), "tvts_cast_bf16_f32")


def pad_rows_bf16(src, dst):
    """dst[r, :] = src[r, :] zero-extended to dst's width (bf16, row-major 2-D)."""
    lib = _lib.load()
    _chk(lib.tvts_pad_rows_bf16(_p(src), _ld(src), _p(dst), _ld(dst), src.shape[0], src.shape[1], dst.shape[1], _stream()),
         "tvts_pad_rows_bf16")


def add_rows_f32(dst, src):
    """dst[r, c] += src[r, c] for c < dst.shape[1] (fp32; src may be wider)."""
    lib = _lib.load()
    _chk(lib.tvts_add_rows_f32(_p(dst), _ld(dst), _p(src), _ld(src), dst.shape[0], dst.shape[1], _stream()), "tvts_add_rows_f32")


def transpose_batched(src, dst, tiles, ntiles):
    lib = _lib.load()
    with _hbm("weight_transpose", 4.0 * 64 * 64 * ntiles):
        rc = lib.tvts_transpose_bf16_batched(_p(src), _p(dst), _p(tiles), ntiles, _stream())
    _chk(rc, "tvts_transpose_bf16_batched")


def probe_tr16(inp, out):
    lib = _lib.load()
    _chk(lib.tvts_probe_tr16(_p(inp), _p(out), _stream()), "tvts_probe_tr16")


CLOCK_PROBE = None  # bench.py: dict(buf=int64 [n, 4] device tensor, i=0) while the instrumented step runs (see gemm_nt)


def zero_(t):
    """t[...] = 0 through the library (a zero-fill kernel on the current stream); t contiguous"""
    assert t.is_contiguous()
    _chk(_lib.load().tvts_zero_bytes(_p(t), t.numel() * t.element_size(), _stream()), "tvts_zero_bytes")
    return t


def device_clock_info(device=0):
    """-> (rate of the constant counter in kHz, CU count, the sheet's maximum shader clock in kHz)"""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _chk(_lib.load().tvts_device_clock_info(int(device), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "tvts_device_clock_info")
    return a.value, b.value, c.value


class Event:
    """HIP event on the launch stream (torch.cuda.Event would do too; this one goes through the C ABI)."""

    def __init__(self):
        self._e = ctypes.c_void_p()
        _chk(_lib.load().tvts_event_create(ctypes.byref(self._e)), "tvts_event_create")

    def record(self):
        _chk(_lib.load().tvts_event_record(self._e, _stream()), "tvts_event_record")

    def elapsed_ms(self, end: "Event") -> float:
        ms = ctypes.c_float()
        _chk(_lib.load().tvts_event_elapsed_ms(self._e, end._e, ctypes.byref(ms)), "tvts_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            _lib.load().tvts_event_destroy(self._e)
        except Exception:
            pass
