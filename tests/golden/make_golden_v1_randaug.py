#!/usr/bin/env python3
"""Generate tests/golden/v1_randaug.npz by RUNNING THE REFERENCE's RandAugment under PIL (build container only).

v1/downstream/rand_augment.py and video_transforms.py (for ``create_random_augment``) are loaded read-only through the `_load` /
`_stub` shims of make_golden_v1.py; ``torchvision.transforms.Compose`` is stubbed by the three-line composer below, ``functional``
and ``random_erasing`` are stubbed empty (nothing run here reaches them).  No reference file is edited or copied; only data lands in
the fixture: seeded uint8 input frames, the frames the reference's operations returned, and -- recorded from OUTSIDE the reference
by wrapping its ``NAME_TO_OP`` entries -- the name of every operation function it called per view, with its argument and resample.

Two sections.
  op.*     every one of the fifteen operation functions called directly, at two arguments (the three without an argument once),
           on one frame of 19 x 27 and one of 40 x 70; the geometric ones with both signs and both resamples, posterize at 0 and
           8 bits, solarize at thresholds 0 and 256.
  chain.*  ``create_random_augment`` for three configurations over Bs = 2 clips x num_sample = 2 views x T = 2 frames, each under a
           seed of ``random`` and ``np.random``, with one ``random.random()`` and one ``np.random.uniform()`` drawn behind the run.
           The seeds are searched (the reference drawing, its operations replaced by a recorder) until the three chains together
           hold every operation function, a view with no active operation, a view with four, a view with one function twice, and
           both signs of a negated argument; the conditions are asserted on the real run.

    python tests/golden/make_golden_v1_randaug.py
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TVTS_REFERENCE_V1", "/root/reference/v1")
sys.path.insert(0, ROOT)

from tests import v1_randaug_ref as R  # noqa: E402
from tests.golden.make_golden_v1 import _load, _stub, save  # noqa: E402

SIZES = ((19, 27), (40, 70))
CHAINS = (("rand-m7-n4-mstd0.5-inc1", "bicubic"), ("rand-m9-n2-w0", "bilinear"), ("rand-m10-n3-inc0", "bicubic"))
BS, NS, T, CH, CW = 2, 2, 2, 24, 37
GEO = ("rotate", "shear_x", "shear_y", "translate_x_rel", "translate_y_rel")
# (function, argument, resample): 2 = PIL's BILINEAR, 3 = BICUBIC
OP_CASES = [("auto_contrast", None, 0), ("equalize", None, 0), ("invert", None, 0),
            ("rotate", 13.5, 3), ("rotate", -27.0, 2), ("rotate", 21.0, 2), ("rotate", -8.25, 3),
            ("posterize", 0, 0), ("posterize", 3, 0), ("posterize", 8, 0),
            ("solarize", 0, 0), ("solarize", 100, 0), ("solarize", 256, 0),
            ("solarize_add", 40, 0), ("solarize_add", 110, 0),
            ("color", 0.3, 0), ("color", 1.7, 0), ("contrast", 0.25, 0), ("contrast", 1.9, 0),
            ("brightness", 0.1, 0), ("brightness", 1.6, 0), ("sharpness", 0.1, 0), ("sharpness", 1.9, 0),
            ("shear_x", 0.21, 2), ("shear_x", -0.3, 3), ("shear_y", 0.3, 3), ("shear_y", -0.12, 2),
            ("translate_x_rel", 0.315, 3), ("translate_x_rel", -0.45, 2), ("translate_y_rel", 0.45, 2), ("translate_y_rel", -0.2, 3)]


class Compose:
    def __init__(self, ts): self.ts = ts
    def __call__(self, x):
        for t in self.ts: x = t(x)
        return x


def load_reference():
    tv = _stub("torchvision")
    tv.transforms = _stub("torchvision.transforms", Compose=Compose)
    tv.transforms.functional = _stub("torchvision.transforms.functional")
    _stub("functional")
    _stub("random_erasing", RandomErasing=None)
    d = os.path.join(REF, "downstream")
    ra = _load("rand_augment", os.path.join(d, "rand_augment.py"))
    vt = _load("video_transforms", os.path.join(d, "video_transforms.py"))
    return ra, vt


def run_chain(ra, vt, cfg, interp, seed, frames, dry):
    """the reference's transform over BS * NS views -> (views uint8 [B, T, H, W, 3], record per view, next random, next uniform);
    dry: the operations are replaced by the recorder alone (the seed search)"""
    from PIL import Image
    calls = []
    orig = dict(ra.NAME_TO_OP)

    def wrap(fn):
        def run(img, *args, **kwargs):
            calls.append((fn.__name__, args[0] if args else None, int(kwargs.get("resample", 0))))
            return img if dry else fn(img, *args, **kwargs)
        return run
    wrapped = {}
    for name, fn in orig.items():
        wrapped[name] = wrapped.get(name) or wrap(fn)
    try:
        ra.NAME_TO_OP.update(wrapped)
        random.seed(seed)
        np.random.seed(seed)
        views, rec = [], []
        for b in range(BS * NS):
            tf = vt.create_random_augment(input_size=(224, 224), auto_augment=cfg, interpolation=interp)
            del calls[:]
            out = tf([Image.fromarray(f) for f in frames[b // NS]])
            assert len(calls) % T == 0 and all(calls[i] == calls[i - i % T] for i in range(len(calls)))  # one draw for all frames
            rec.append([[n, None if a is None else float(a), r if n in GEO else 0] for n, a, r in calls[::T]])
            views.append(np.stack([np.asarray(im) for im in out]))
        return np.stack(views), rec, random.random(), float(np.random.uniform())
    finally:
        ra.NAME_TO_OP.update(orig)


def facts(recs):
    """what the tests rely on, over the records of the chains so far -> set of strings"""
    have = set()
    for rec in recs:
        for view in rec:
            names = [n for n, _, _ in view]
            have.update(names)
            have.add("views with %d" % len(view)) if len(view) in (0, 4) else None
            if len(set(names)) < len(names):
                have.add("twice")
            for n, a, _ in view:
                if n in GEO:
                    have.add("negative" if a < 0 else "positive")
    return have


WANT = {fn for fn, _, _ in OP_CASES} | {"views with 0", "views with 4", "twice", "negative", "positive"}


def main():
    ra, vt = load_reference()
    from PIL import Image
    out = {}
    # ---- per op
    frames = [R.case_frames(9100 + k, 1, h, w)[0] for k, (h, w) in enumerate(SIZES)]
    res = [[], []]
    for fn, arg, resample in OP_CASES:
        f = {v.__name__: v for v in ra.NAME_TO_OP.values()}[fn]
        for k, fr in enumerate(frames):
            args = () if arg is None else (arg,)
            got = np.asarray(f(Image.fromarray(fr), *args, fillcolor=(128, 128, 128), resample=resample or 2))
            assert got.shape == fr.shape and got.dtype == np.uint8
            mine = R.apply_named(fr, fn, arg, resample)
            assert np.array_equal(mine, got), (fn, arg, resample, int((mine != got).sum()))
            res[k].append(got)
    out.update({"op.fn": np.array([c[0] for c in OP_CASES]), "op.arg": np.array([np.nan if c[1] is None else c[1] for c in OP_CASES]),
                "op.resample": np.array([c[2] for c in OP_CASES]), "op.frame_a": frames[0], "op.frame_b": frames[1],
                "op.out_a": np.stack(res[0]), "op.out_b": np.stack(res[1])})
    # ---- chains: a greedy seed search on the reference's own draw, then the real run
    recs = []
    for k, (cfg, interp) in enumerate(CHAINS):
        src = R.case_frames(9200 + k, BS * T, CH, CW).reshape(BS, T, CH, CW, 3)
        best, best_n = None, -1
        for seed in range(1000 * k, 1000 * k + 1000):
            _, rec, _, _ = run_chain(ra, vt, cfg, interp, seed, src, dry=True)
            n = len(facts(recs + [rec]) & WANT)
            if n > best_n:
                best, best_n = seed, n
        views, rec, nxt_r, nxt_u = run_chain(ra, vt, cfg, interp, best, src, dry=False)
        recs.append(rec)
        print(f"chain {k} {cfg} {interp}: seed {best}, {best_n} of {len(WANT)} facts\n  " + "\n  ".join(map(str, rec)))
        out.update({f"chain.{k}.cfg": cfg, f"chain.{k}.interp": interp, f"chain.{k}.seed": best, f"chain.{k}.frames": src,
                    f"chain.{k}.views": views, f"chain.{k}.rec": json.dumps(rec), f"chain.{k}.next_random": nxt_r,
                    f"chain.{k}.next_uniform": nxt_u})
    missing = WANT - facts(recs)
    assert not missing, missing
    out.update({"chain.n": len(CHAINS), "chain.shape": np.array([BS, NS, T, CH, CW])})
    save("v1_randaug", **out)


if __name__ == "__main__":
    main()
