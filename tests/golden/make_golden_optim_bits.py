#!/usr/bin/env python3
"""Record tests/golden/optim_bits.npz: SHA-256 digests of what the flat-store optimizer launches leave behind (needs the GPU).

The per-element bounds of the AdamW tests and the equalities between variants would not see a change of operation order that moves
every variant alike; this fixture pins the bits themselves.  `record(K)` runs three consecutive steps of each of

    K.adamw_torch   host step | step_dev,  without | with ema
    K.sgd_torch     momentum 0.9 Nesterov | 0.9 plain | 0,  host step | step_dev,  without | with ema
    K.adamw_hf      host step | step_dev + hyper_dev

over four chunks with the group bytes [0, 1, 255, 1] (chunk 2 frozen), grad_scale 0.5 and, for the torch rules, a norm_coef cell
holding the clip coefficient 0.75, and after every step takes the digest of the bytes of p, of each state buffer the rule has, of
the bf16 shadow and of the average.  Digests only: the file stays a few kilobytes.  tests/test_optim_bits_gpu.py runs record() again
and compares.  The file is to be made from the tree BEFORE a change that must keep the bits (every call here has had the same Python
signature since the average was added), never from the code under test:

    python tests/golden/make_golden_optim_bits.py
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "optim_bits.npz")
CH = 1024
GROUPS = [0, 1, 255, 1]
STEPS = 3
DECAY = 0.9999
GRAD_SCALE = 0.5
GRAD_FACTOR = [1.0, -0.5, 2.0]  # the stored gradient of step k is g * GRAD_FACTOR[k] (exact in fp32)
HF_LR, HF_WD = [1e-2, 3e-3, 1e-3, 2e-3], [0.05, 0.0, 0.01, 0.02]


def state():
    """fp32 p, g, m, v, e over the four chunks from a fixed CPU generator (the construction of tests/test_v1_guard_gpu.py)"""
    gen = torch.Generator().manual_seed(2400)
    n = CH * len(GROUPS)
    return dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen) * 0.1, m=torch.randn(n, generator=gen) * 0.05,
                v=torch.rand(n, generator=gen) * 1e-2, e=torch.randn(n, generator=gen))


def hyper_table():
    h = torch.full((128,), 7.0)
    h[0], h[1], h[64], h[65] = 1e-2, 3e-3, 0.05, 0.0
    return h


def calls():
    """(name, kind, options) of every recorded call"""
    out = []
    for dev in (False, True):
        for ema in (False, True):
            tag = ("dev" if dev else "host") + ("_ema" if ema else "")
            out.append((f"adamw_torch_{tag}", "adamw", dict(dev=dev, ema=ema)))
            for mname, mu, nes in (("nesterov", 0.9, True), ("plain", 0.9, False), ("mom0", 0.0, False)):
                out.append((f"sgd_torch_{mname}_{tag}", "sgd", dict(dev=dev, ema=ema, momentum=mu, nesterov=nes)))
        out.append((f"adamw_hf_{'dev' if dev else 'host'}", "hf", dict(dev=dev, ema=False)))
    return out


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).digest()


def record(K, device="cuda:0"):
    """{"<call>/<step>/<buffer>": 32 digest bytes}, in the order the calls are made"""
    s = state()
    cg = torch.tensor(GROUPS, dtype=torch.uint8, device=device)
    hyper = hyper_table().to(device)
    hf_hyper = torch.tensor(HF_LR + HF_WD, dtype=torch.float32, device=device)
    nc = torch.tensor([1.0, 0.75], dtype=torch.float32, device=device)
    out = {}
    for name, kind, o in calls():
        t = {k: s[k].to(device) for k in ("p", "m", "v", "e")}
        t["sh"] = torch.full((s["p"].numel(),), -3.0, dtype=torch.bfloat16, device=device)
        keep = ["p", "sh"] + {"adamw": ["m", "v"], "hf": ["m", "v"], "sgd": ["m"] if o.get("momentum") else []}[kind] + (["e"] if o["ema"] else [])
        ema = dict(ema=t["e"], ema_decay=DECAY) if o["ema"] else {}
        for k in range(STEPS):
            g = (s["g"] * GRAD_FACTOR[k]).to(device)
            sd = torch.tensor([k + 1], dtype=torch.int32, device=device) if o["dev"] else None
            step = 0 if o["dev"] else k + 1
            if kind == "adamw":
                K.adamw_torch(t["p"], g, t["m"], t["v"], t["sh"], cg, hyper, step, grad_scale=GRAD_SCALE, step_dev=sd, norm_coef=nc, **ema)
            elif kind == "sgd":
                K.sgd_torch(t["p"], g, t["m"] if o["momentum"] else None, t["sh"], cg, hyper, step, momentum=o["momentum"],
                            nesterov=o["nesterov"], grad_scale=GRAD_SCALE, step_dev=sd, norm_coef=nc, **ema)
            else:
                K.adamw_hf(t["p"], g, t["m"], t["v"], t["sh"], cg, HF_LR, HF_WD, step, grad_scale=GRAD_SCALE, step_dev=sd,
                           hyper_dev=hf_hyper if o["dev"] else None)
            torch.cuda.synchronize()
            for b in keep:
                out[f"{name}/{k + 1}/{b}"] = digest(t[b])
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tvts_amd import hip
    rec = record(hip)
    for name in rec:  # every buffer moves in every step (equal digests ACROSS calls are expected: host step against step_dev)
        call, k, b = name.split("/")
        assert k == "1" or rec[name] != rec[f"{call}/{int(k) - 1}/{b}"], name
    np.savez_compressed(OUT, names=np.array(list(rec), dtype="S"), digests=np.frombuffer(b"".join(rec.values()), dtype=np.uint8).reshape(-1, 32))
    print(f"wrote {OUT}: {len(rec)} digests")


if __name__ == "__main__":
    main()
