"""RandAugment on the device (tvts_randaug_hist / tvts_randaug_apply, hip.randaug_u8, FinetuneStep.step(..., aug=plan with ra));
run with -m gpu.  The gate is bit equality: zero differing bytes against the reference's own frames under PIL
(tests/golden/v1_randaug.npz) and, where the fixture has no frame, against tests/v1_randaug_ref.py, which
tests/test_v1_randaug_cpu.py pins to that fixture and to PIL.  No PIL and no reference tree is needed here."""
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import v1_downstream_synth as S  # noqa: E402
import v1_randaug_ref as R  # noqa: E402
from tvts_amd.downstream import finetune_v1 as F  # noqa: E402

DEV = "cuda:0"
SENT = 0xA5  # what the view regions of the work tensor are pre-filled with
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "v1_randaug.npz")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def op_cases(gold):
    return [(str(fn), None if np.isnan(arg) else float(arg), int(rs))
            for fn, arg, rs in zip(gold["op.fn"], gold["op.arg"], gold["op.resample"])]


def plan_of(views, H, W, L, ns):
    """views: per view a list of (function name, argument, resample) -> RAPlan"""
    out = []
    for ops in views:
        rows = [F.ra_row(fn, arg, rs, H, W) for fn, arg, rs in ops]
        out.append(([r for r in rows if r[0][0] != F.RA_NONE], ops))
    return F.ra_plan(out, L, ns)


def run(K, frames, plan):
    """frames uint8 [Bs, T, H, W, 3] -> (the work tensor on the host, the clip every view ended in, the table)"""
    Bs, B = frames.shape[0], plan.ra_i.shape[0]
    work = torch.full((Bs + 2 * B,) + tuple(frames.shape[1:]), SENT, dtype=torch.uint8, device=DEV)
    work[:Bs] = torch.from_numpy(np.array(frames)).to(DEV)
    table = K.RandaugTable(plan.ra_i, plan.ra_d, Bs=Bs, num_sample=plan.num_sample, device=DEV)
    rows = K.randaug_u8(work, table)
    torch.cuda.synchronize()
    return work.cpu().numpy(), rows, table


def check_untouched(work, frames, ra_i, Bs):
    """the source clips are as uploaded, and a clip of the view regions holds the sentinel unless layer j < k_b wrote it"""
    B = ra_i.shape[0]
    assert np.array_equal(work[:Bs], frames), "a source clip was written"
    written = {Bs + (j & 1) * B + b for b in range(B) for j in range(int((ra_i[b, :, 0] != 0).sum()))}
    for r in range(Bs, Bs + 2 * B):
        if r not in written:
            assert (work[r] == SENT).all(), f"clip {r} of the work tensor was written by a layer that had no op for its view"


@pytest.mark.parametrize("size", ["a", "b"])
def test_every_op_equals_the_reference_frames(K, gold, size):
    """all op cases of the fixture as the views of one clip, one layer: 19 x 27 (81-byte rows, inside one tile) and 40 x 70 (wider
    and taller than a tile)"""
    fr, want = gold["op.frame_" + size], gold["op.out_" + size]
    cases = op_cases(gold)
    plan = plan_of([[c] for c in cases], fr.shape[0], fr.shape[1], 1, len(cases))
    work, rows, _ = run(K, fr[None, None], plan)
    bad = {}
    for b, c in enumerate(cases):
        n = int((work[rows[b], 0] != want[b]).sum())
        print(f"{c}: {n} differing bytes")
        if n:
            bad[c] = n
    assert not bad, bad
    check_untouched(work, fr[None, None], plan.ra_i, 1)


STAT_OPS = [("auto_contrast", None, 0), ("equalize", None, 0), ("contrast", 0.4, 0), ("contrast", 1.7, 0), ("sharpness", 0.3, 0),
            ("sharpness", 1.9, 0), ("color", 1.6, 0), ("rotate", 17.0, 3), ("shear_x", -0.3, 2)]


def degenerate_frames(name):
    rng = np.random.RandomState(5)
    if name == "constant":
        fr = np.empty((2, 19, 27, 3), dtype=np.uint8)
        fr[0], fr[1] = (7, 200, 90), (0, 255, 128)
        return fr
    if name == "8x8":   # 64 pixels: equalize has step == 0; sharpness a 6 x 6 interior
        return rng.randint(0, 256, size=(2, 8, 8, 3)).astype(np.uint8)
    return rng.randint(0, 256, size=(2, 3, 3, 3)).astype(np.uint8)  # sharpness: one interior pixel


@pytest.mark.parametrize("name", ["constant", "8x8", "3x3"])
def test_degenerate_statistics(K, name):
    fr = degenerate_frames(name)[None]  # one clip of two frames
    plan = plan_of([[c] for c in STAT_OPS], fr.shape[2], fr.shape[3], 1, len(STAT_OPS))
    work, rows, _ = run(K, fr, plan)
    for b, c in enumerate(STAT_OPS):
        for t in range(fr.shape[1]):
            want = R.apply_named(fr[0, t], *c)
            n = int((work[rows[b], t] != want).sum())
            assert n == 0, (name, c, t, n)
    if name == "constant":
        for b in (0, 1):
            assert np.array_equal(work[rows[b]], fr[0]), STAT_OPS[b]  # one nonzero bin per channel: the identity, exactly


def chain(gold, k):
    Bs, ns, T, H, W = (int(v) for v in gold["chain.shape"])
    rec = [[(n, a, r or 0) for n, a, r in v] for v in json.loads(str(gold[f"chain.{k}.rec"]))]
    interp = 2 if str(gold[f"chain.{k}.interp"]) == "bilinear" else 3
    rec = [[(n, a, interp) for n, a, _ in v] for v in rec]
    L = max(4, max(len(v) for v in rec))
    return gold[f"chain.{k}.frames"], gold[f"chain.{k}.views"], plan_of(rec, H, W, L, ns)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_chains_equal_the_reference_and_leave_the_rest_untouched(K, gold, k):
    frames, views, plan = chain(gold, k)
    work, rows, table = run(K, frames, plan)
    for b in range(len(views)):
        n = int((work[rows[b]] != views[b]).sum())
        assert n == 0, (k, b, plan.ops[b], n)
    check_untouched(work, frames, plan.ra_i, frames.shape[0])
    again, rows2, _ = run(K, frames, plan)
    assert np.array_equal(work, again) and np.array_equal(rows, rows2), "two identical calls left different bytes"


def test_entry_points_refuse_bad_arguments(K):
    from tvts_amd import _lib
    lib = _lib.load()
    w = torch.zeros((3, 1, 4, 4, 3), dtype=torch.uint8, device=DEV)
    ri, rd = torch.zeros((1, 2, 4), dtype=torch.int32, device=DEV), torch.zeros((1, 2, 8), dtype=torch.float64, device=DEV)
    h = torch.zeros((1, 1, 4, 256), dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    good = dict(work=p(w), Bs=1, B=1, ns=1, T=1, H0=4, W0=4, layer=0, L=2, ra_i=p(ri))
    assert lib.tvts_randaug_hist(*good.values(), p(h), None) == 0
    assert lib.tvts_randaug_apply(*good.values(), p(rd), None, None) == 0
    for key, val in (("work", None), ("ra_i", None), ("Bs", 0), ("B", 2), ("ns", 0), ("T", 0), ("H0", 2), ("W0", 2), ("layer", 2),
                     ("layer", -1), ("L", 9), ("L", 0)):
        args = dict(good, **{key: val})
        assert lib.tvts_randaug_hist(*args.values(), p(h), None) == -22, (key, val)
        assert lib.tvts_randaug_apply(*args.values(), p(rd), p(h), None) == -22, (key, val)
    assert lib.tvts_randaug_hist(*good.values(), None, None) == -22
    assert lib.tvts_randaug_apply(*good.values(), None, p(h), None) == -22
    torch.cuda.synchronize()
    assert not w.any()


# ---------------------------------------------------------------------------------------------- the gather and the step
def drawn_aug(plan_ra, Bs, ns, H, W, img, seed=21):
    """a seeded crop / flip / erase draw for the chain's views, carrying the RandAugment plan, and the same rows over B
    pre-augmented source clips (view b reads clip b)"""
    py_state, np_state = random.getstate(), np.random.get_state()
    try:
        random.seed(seed)
        np.random.seed(seed)
        aug_i = F.Augment(img, hflip=0.5, reprob=0.5, remode="pixel", num_sample=ns, noise_seed=seed).draw(Bs, H, W).aug_i
    finally:
        random.setstate(py_state)
        np.random.set_state(np_state)
    pre = aug_i.copy()
    pre[:, 0] = np.arange(len(pre))
    return F.AugPlan(aug_i, plan_ra), F.AugPlan(pre)


def test_gather_through_randaug_is_the_gather_on_the_augmented_views(K, gold):
    frames, views, ra = chain(gold, 0)
    kw = S.TINY
    img, patch, tb = kw["img_size"], kw["patch_size"], kw["tubelet_size"]
    Bs, B, T, H, W = frames.shape[0], len(views), frames.shape[1], frames.shape[2], frames.shape[3]
    plan, pre = drawn_aug(ra, Bs, ra.num_sample, H, W, img)
    n, kc = (img // patch) ** 2, 3 * tb * patch * patch
    keep = torch.arange(n, dtype=torch.int32).repeat(B, T // tb, 1).contiguous().to(DEV)
    mix = K.mix_table(np.array([[B - 1 - b, 1 + b % 2, 3, 40, 5, 50] for b in range(B)]), np.array([[0.7, 0.3]] * B, dtype=np.float32),
                      B=B, img=img, device=DEV)
    work, rows, _ = run(K, frames, ra)
    aug_i = np.array(plan.aug_i)
    aug_i[:, 0] = rows
    outs = []
    for src, tab in ((work, aug_i), (views, pre.aug_i)):
        fr = torch.from_numpy(np.array(src)).to(DEV)
        out = torch.zeros((B * (T // tb) * n, kc), dtype=torch.bfloat16, device=DEV)
        K.patch_gather_tube_u8_aug(fr, keep, out, K.aug_table(tab, Bs=fr.shape[0], H0=H, W0=W, img=img, device=DEV), mix, B=B,
                                   tubes=T // tb, tubelet=tb, n=n, img=img, patch=patch)
        outs.append(out.view(torch.int16).cpu())
    assert torch.equal(outs[0], outs[1]), int((outs[0] != outs[1]).sum())


def test_step_with_randaug_is_the_step_on_the_augmented_views(K, gold):
    """FinetuneStep.step(source clips, aug = plan with ra, mix) against a twin's step fed the reference's augmented views as B source
    clips: loss, logits and the whole flat gradient bit for bit; a plan without ra afterwards still takes the plain path"""
    from test_v1_aug_gpu import run_step, same_bits
    from test_v1_finetune_gpu import F as FX, build
    import v1_mixup_ref as M
    frames, views, ra = chain(gold, 0)
    img, C = S.TINY["img_size"], FX["classes"]
    Bs, B, H, W = frames.shape[0], len(views), frames.shape[2], frames.shape[3]
    plan, pre = drawn_aug(ra, Bs, ra.num_sample, H, W, img)
    np_state = np.random.get_state()
    np.random.seed(9)
    mix = F.Mixup(num_classes=C, mode="elem", label_smoothing=0.1, **M.DEFAULT).draw(B, img)
    np.random.set_state(np_state)
    labels = torch.randint(0, C, (Bs,), generator=torch.Generator().manual_seed(64)).repeat_interleave(ra.num_sample)
    m, twin = build(rate=0.0), build(rate=0.0)
    for what, mplan in (("randaug", None), ("randaug + mix", mix)):
        got = run_step(m, torch.from_numpy(frames), labels, aug=plan, mix=mplan)
        want = run_step(twin, torch.from_numpy(views), labels, aug=pre, mix=mplan)
        same_bits(got, want, what)
    plain = F.AugPlan(plan.aug_i)
    same_bits(run_step(m, torch.from_numpy(frames), labels, aug=plain), run_step(twin, torch.from_numpy(frames), labels, aug=plain),
              "a plan without ra")
