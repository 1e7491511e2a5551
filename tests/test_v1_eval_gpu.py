"""The device side of the v1 evaluation (tvts_amd/downstream/evaluate_v1.py; run with -m gpu): the test-view gather, the label
ranks, the per-video view sum, and validation_one_epoch / final_test / ViewMerger end to end on the tiny model.

Every kernel result here is an exact quantity and is compared bit for bit: the gather against tvts_patch_gather_tube_u8 on the
host-sliced clips and against bf16 of the reference's recorded clips (tests/golden/v1_eval.npz; tests/test_v1_eval_cpu.py shows by
sha256 that tests/v1_eval_ref.normalise(slice_view(...)) IS the recorded fp32 clip), the ranks against their numpy definition, the
view sums against a numpy fp32 loop in the stated order.  The only bounded figure is the validation loss: the ce_check bound of
tests/kernel_bounds.py (restated in ce_loss_bound below and pinned to ce_check itself), averaged over the batches."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
import v1_downstream_synth as S  # noqa: E402
import v1_eval_ref as R  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
EINVAL = -22
IMG, TB, T, TSRC = 32, 2, 4, 8
TUBES = T // TB


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


@pytest.fixture(scope="module")
def E(K):
    from tvts_amd.downstream import evaluate_v1
    return evaluate_v1


@pytest.fixture(scope="module")
def fx(golden):
    return golden("v1_eval")


@pytest.fixture(scope="module")
def clips():
    """seeded uint8 source clips {(H0, W0): [2, TSRC, H0, W0, 3]}, made once and never written: the two fixture sizes (clip 0 of
    each IS the recorded one) and a square one without room"""
    out = {}
    for (h, w), seed in zip(R.SIZES + ((IMG, IMG),), R.FRAME_SEEDS + (9103,)):
        a = np.stack([R.source_clip(seed, h, w), R.source_clip(seed + 50, h, w)])
        a.setflags(write=False)
        out[(h, w)] = a
    return out


# ---------------------------------------------------------------------------------------------- helpers
def full_keep(b, patch, tubes=TUBES, img=IMG):
    return torch.arange((img // patch) ** 2, dtype=torch.int32).repeat(b, tubes, 1).contiguous()


def kc(patch):
    return 3 * TB * patch * patch


def gather_view(K, frames, view_i, patch, keep=None, cols=8, check=True, img=IMG):
    """one launch of the view gather into a guarded output -> (out view [B * tubes * n, Kc] bf16, its buffer)"""
    fr = torch.from_numpy(np.array(frames)).to(DEV)
    view_i = np.asarray(view_i, dtype=np.int64)
    b = len(view_i)
    keep = full_keep(b, patch) if keep is None else keep
    n = keep.shape[2]
    if check:
        table = K.view_table(view_i, Bs=fr.shape[0], Tsrc=fr.shape[1], H0=fr.shape[2], W0=fr.shape[3], T=T, img=img, device=DEV)
    else:
        table = torch.from_numpy(view_i.astype(np.int32)).to(DEV)
    buf, out = KB.guarded(b * TUBES * n, kc(patch), BF16, DEV, rows=3, cols=cols)
    K.patch_gather_tube_u8_view(fr, keep.to(DEV), out, table, B=b, tubes=TUBES, tubelet=TB, n=n, img=img, patch=patch)
    torch.cuda.synchronize()
    KB.check_guards(buf, b * TUBES * n, kc(patch), "view gather")
    return out, buf


def gather_sliced(K, frames, view_i, patch, keep=None, img=IMG):
    """tvts_patch_gather_tube_u8 (the parent's kernel) on the host-sliced uint8 clips of the same views"""
    view_i = np.asarray(view_i)
    sl = np.stack([R.slice_view(frames[int(r[0])], r, T, img) for r in view_i])
    b = len(view_i)
    keep = full_keep(b, patch) if keep is None else keep
    n = keep.shape[2]
    out = torch.empty(b * TUBES * n, kc(patch), dtype=BF16, device=DEV)
    K.patch_gather_tube_u8(torch.from_numpy(sl).to(DEV), keep.to(DEV), out, B=b, tubes=TUBES, tubelet=TB, n=n, img=img, patch=patch)
    torch.cuda.synchronize()
    return out


def fold(out, b, patch, img=IMG):
    """bf16 rows [B * tubes * ppf, 3 * tb * patch^2] of a full keep -> clip [B, 3, T, img, img] (bf16, on the host)"""
    g = img // patch
    o = out.detach().cpu().contiguous().view(b, TUBES, g, g, 3, TB, patch, patch)
    return o.permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(b, 3, TUBES * TB, img, img).contiguous()


SIX = {  # B = 6 views over Bs = 2 clips; the offsets reach 0 and H0 - img / W0 - img, t0 = 1 ends on frame TSRC - 1
    (32, 48): [[0, 0, 2, 0, 0], [1, 1, 2, 0, 16], [0, 1, 2, 0, 8], [1, 0, 2, 0, 3], [1, 4, 1, 0, 16], [0, 1, 2, 0, 0]],
    (48, 32): [[1, 0, 2, 0, 0], [0, 1, 2, 16, 0], [0, 0, 2, 8, 0], [1, 1, 2, 5, 0], [0, 4, 1, 16, 0], [1, 1, 2, 16, 0]],
    (32, 32): [[0, 0, 2, 0, 0], [1, 1, 2, 0, 0], [1, 0, 1, 0, 0], [0, 4, 1, 0, 0], [0, 1, 2, 0, 0], [1, 1, 2, 0, 0]],
}


def rows8(rows):
    return [list(r) + [0, 0, 0] for r in rows]


# ================================================================================================ 1. the view gather
@pytest.mark.parametrize("patch", [16, 8])
@pytest.mark.parametrize("size", list(SIX))
def test_gather_equals_the_u8_gather_on_host_sliced_clips(K, clips, size, patch):
    view_i = rows8(SIX[size])
    got, _ = gather_view(K, clips[size], view_i, patch)
    want = gather_sliced(K, clips[size], view_i, patch)
    assert not torch.isnan(got.float()).any()
    KB.assert_equal_bits(got.contiguous(), want, f"view gather {size} patch {patch}")


@pytest.mark.parametrize("patch", [16, 8])
def test_gather_equals_the_reference_clips(K, E, fx, clips, patch):
    """the fixture's views, planned by TestViews: bf16 of the clip the reference's __getitem__ returned, byte for byte"""
    for k, size in enumerate(R.SIZES):
        plan = E.TestViews(IMG, IMG, R.SEG, R.CROP).plan(1, TSRC, *size)
        src = clips[size][:1]
        want = []
        for j, row in enumerate(plan.view_i):
            clip = R.normalise(R.slice_view(src[0], row, plan.T, IMG))
            assert R.sha(clip) == str(fx[f"sha_{k}"][j])  # the recorded clip itself
            want.append(torch.from_numpy(clip).to(BF16))
        got, _ = gather_view(K, src, plan.view_i, patch)
        KB.assert_equal_bits(fold(got, len(plan), patch), torch.stack(want), f"fixture views {size} patch {patch}")


def test_gather_single_sample_keep_subset_and_wide_rows(K, clips):
    fr = clips[(32, 48)]
    for patch in (16, 8):
        ppf = (IMG // patch) ** 2
        one = rows8([[1, 1, 2, 0, 16]])
        got, _ = gather_view(K, fr, one, patch)                                           # B = 1
        KB.assert_equal_bits(got.contiguous(), gather_sliced(K, fr, one, patch), f"B = 1 patch {patch}")
        keep = torch.tensor([[[ppf - 1], [1]]], dtype=torch.int32)                        # n = 1, another patch per tube
        got, _ = gather_view(K, fr, one, patch, keep=keep, cols=24)                       # and a wider leading dimension
        KB.assert_equal_bits(got.contiguous(), gather_sliced(K, fr, one, patch, keep=keep), f"n = 1 patch {patch}")
        view_i = rows8(SIX[(32, 48)])
        keep = torch.stack([torch.randperm(ppf, generator=torch.Generator().manual_seed(7 + i))[:3] for i in range(6 * TUBES)])
        keep = keep.view(6, TUBES, 3).to(torch.int32).contiguous()
        got, _ = gather_view(K, fr, view_i, patch, keep=keep, cols=16)
        KB.assert_equal_bits(got.contiguous(), gather_sliced(K, fr, view_i, patch, keep=keep), f"keep subset patch {patch}")


def test_gather_leaves_a_row_without_source_unwritten(K, clips):
    fr, patch = clips[(48, 32)], 8
    view_i = np.array(rows8(SIX[(48, 32)]))
    view_i[2, 0], view_i[4, 0] = -1, 2          # outside [0, Bs) on both sides; (the host check refuses them)
    with pytest.raises(ValueError):
        K.view_table(view_i, Bs=2, Tsrc=TSRC, H0=48, W0=32, T=T, img=IMG, device=DEV)
    got, _ = gather_view(K, fr, view_i, patch, check=False)
    rows = TUBES * (IMG // patch) ** 2
    ok = np.array(rows8(SIX[(48, 32)]))
    want = gather_sliced(K, fr, ok, patch)
    for b in range(6):
        mine = got[b * rows:(b + 1) * rows]
        if b in (2, 4):
            assert torch.isnan(mine.float()).all(), b
        else:
            KB.assert_equal_bits(mine.contiguous(), want[b * rows:(b + 1) * rows].contiguous(), f"sample {b}")


def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def test_gather_einval_for_each_refused_argument(K, clips):
    lib = K._lib.load()
    H0, W0, patch, b = 32, 48, 8, 6
    fr = torch.from_numpy(np.array(clips[(H0, W0)])).to(DEV)
    keep = full_keep(b, patch).to(DEV)
    table = K.view_table(rows8(SIX[(H0, W0)]), Bs=2, Tsrc=TSRC, H0=H0, W0=W0, T=T, img=IMG, device=DEV)
    n, kcw = keep.shape[2], kc(patch)
    buf, out = KB.guarded(b * TUBES * n, kcw, BF16, DEV, rows=3, cols=8)
    m3, s3 = (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(frames=_ptr(fr), Bs=2, Tsrc=TSRC, H0=H0, W0=W0, view_i=_ptr(table), keep=_ptr(keep), B=b, tubes=TUBES, tubelet=TB, n=n,
                img=IMG, patch=patch, mean3=m3, std3=s3, out=_ptr(buf), ldo=kcw + 8)
    bad = [("frames", None), ("view_i", None), ("keep", None), ("out", None), ("mean3", None), ("std3", None), ("Bs", 0), ("Bs", -1),
           ("Tsrc", 0), ("Tsrc", -2), ("H0", 0), ("W0", 0), ("H0", IMG - 1), ("W0", IMG - 1), ("B", 0), ("tubes", 0), ("tubelet", 0),
           ("tubelet", -1), ("n", 0), ("patch", 0), ("img", 0), ("img", IMG + 4), ("patch", 4), ("ldo", kcw + 4), ("ldo", kcw - 8),
           ("out", _ptr(buf, 8))]
    for key, val in bad:
        args = dict(base)
        args[key] = val
        assert lib.tvts_patch_gather_tube_u8_view(*args.values(), st) == EINVAL, (key, val)
    torch.cuda.synchronize()
    assert torch.isnan(buf.float()).all()        # nothing was launched
    assert lib.tvts_patch_gather_tube_u8_view(*base.values(), st) == 0
    torch.cuda.synchronize()
    KB.check_guards(buf, b * TUBES * n, kcw, "accepted call")
    KB.assert_equal_bits(out.contiguous(), gather_sliced(K, clips[(H0, W0)], rows8(SIX[(H0, W0)]), patch), "accepted call")


def test_engine_view_none_is_the_old_launch_and_view_refuses_company(K):
    """EngineV1._vit_embed_v1: without a view table the uint8 path calls what it called before (same kernel, same arguments); with
    one it refuses a crop, a mix or an aug beside it and anything but uint8 frames"""
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    m = VisionTransformer(num_classes=5, **S.TINY)
    eng, calls = m.engine, []
    frames = torch.randint(0, 256, (2, 4, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    orig = {n: getattr(K, n) for n in ("patch_gather_tube_u8", "patch_gather_tube_u8_view")}
    try:
        for n in orig:
            setattr(K, n, (lambda n: lambda *a, **k: (calls.append(n), orig[n](*a, **k))[1])(n))
        m(frames)
        assert calls == ["patch_gather_tube_u8"]
        del calls[:]
        m.forward_views(frames, rows8([[0, 0, 1, 0, 0], [1, 0, 1, 0, 0]]), 4)
        assert calls == ["patch_gather_tube_u8_view"]
    finally:
        for n in orig:
            setattr(K, n, orig[n])
    keep = torch.arange(16, dtype=torch.int32, device=DEV).repeat(2, 2, 1).contiguous()
    table = K.view_table(rows8([[0, 0, 1, 0, 0], [1, 0, 1, 0, 0]]), Bs=2, Tsrc=4, H0=64, W0=64, T=4, img=64, device=DEV)
    with pytest.raises(ValueError):
        eng.encode_video(frames.to(DEV), keep, 2, 2, crop=torch.zeros(2, 2, dtype=torch.int32, device=DEV), project=False, view=table)
    with pytest.raises(ValueError):
        eng.encode_video(torch.zeros(2, 3, 4, 64, 64, device=DEV), keep, 2, 2, channel_major=True, project=False, view=table)
    with pytest.raises(ValueError):
        m.forward_views(frames, rows8([[0, 1, 1, 0, 0]]), 4)          # the last frame would be frame 4 of 4
    with pytest.raises(ValueError):
        m.forward_views(frames, rows8([[0, 0, 1, 0, 0]]), 3)          # no multiple of the tubelet


# ================================================================================================ 2. tvts_class_ranks
def rank_case(C, Rn, seed):
    """logits quantised to halves (ties everywhere at large C) with planted rows -> (x fp32 [Rn, C], labels)"""
    rs = np.random.RandomState(seed)
    x = (np.round(rs.standard_normal((Rn, C)) * 4) / 2).astype(np.float32)
    labels = rs.randint(0, C, Rn)
    labels[0] = 0                                                  # row 0: label 0 in a quantised row
    if Rn > 1:                                                     # row 1: an all-equal row, label C - 1: every other class ties in front
        x[1], labels[1] = np.float32(1.25), C - 1
    if Rn > 2:                                                     # row 2: -inf entries (the label's among them when it is even)
        x[2, ::2] = -np.inf
    if Rn > 3 and C > 2:                                           # row 3: ties at the label's value on both sides of the label
        lab = C // 2
        x[3], labels[3] = np.float32(-3.0), lab
        x[3, [0, lab - 1, lab, min(lab + 1, C - 1), C - 1]] = np.float32(7.5)
    if Rn > 4:                                                     # row 4: NaN entries outrank nothing
        x[4, rs.rand(C) < 0.3] = np.nan
        x[4, labels[4]] = np.float32(0.0)
    if Rn > 5:                                                     # row 5: all equal, label 0
        x[5], labels[5] = np.float32(-2.0), 0
    labels[6::3] = 0
    labels[7::3] = C - 1
    return x, labels.astype(np.int32)


@pytest.mark.parametrize("Rn", [1, 3, 65])
@pytest.mark.parametrize("C", [1, 5, 11, 174, 1000])
def test_class_ranks_are_exact(K, C, Rn):
    x, labels = rank_case(C, Rn, 100 * C + Rn)
    want = R.class_ranks_np(x, labels)
    if Rn > 1:
        assert want[1] == C - 1
    if Rn > 3 and C > 2:
        assert want[3] == len({0, C // 2 - 1})                     # the equal entries in front of the label count, those behind do not
    if Rn > 5:
        assert want[5] == 0
    for pad in (0, 5):                                             # dense, and a strided view of a wider buffer
        wide = torch.full((Rn, C + pad), float("inf"), dtype=F32, device=DEV)
        wide[:, :C] = torch.from_numpy(x).to(DEV)
        buf = torch.full((Rn + 2,), -7, dtype=torch.int32, device=DEV)
        K.class_ranks(wide[:, :C], torch.from_numpy(labels).to(DEV), buf[:Rn])
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[Rn:] == -7).all()
        assert np.array_equal(got[:Rn], want), (C, Rn, pad, np.nonzero(got[:Rn] != want)[0][:5])
    assert ((want == 0) == (np.nanargmax(np.where(np.isnan(x), -np.inf, x), axis=1) == labels)).all()


def test_class_ranks_refusals_and_stray_labels(K):
    lib = K._lib.load()
    x = torch.zeros(3, 8, dtype=F32, device=DEV)
    lab = torch.tensor([0, 9, -1], dtype=torch.int32, device=DEV)
    out = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args in ((None, 8, 3, 8, _ptr(lab), _ptr(out)), (_ptr(x), 8, 3, 8, None, _ptr(out)), (_ptr(x), 8, 3, 8, _ptr(lab), None),
                 (_ptr(x), 8, 0, 8, _ptr(lab), _ptr(out)), (_ptr(x), 8, 3, 0, _ptr(lab), _ptr(out)), (_ptr(x), 7, 3, 8, _ptr(lab), _ptr(out))):
        assert lib.tvts_class_ranks(*args, st) == EINVAL, args
    torch.cuda.synchronize()
    assert (out == -7).all()
    K.class_ranks(x, lab, out)                                     # a label outside [0, C): rank C, nothing read
    torch.cuda.synchronize()
    assert out.tolist() == [0, 8, 8]


# ================================================================================================ 3. tvts_view_sum
@pytest.mark.parametrize("N", [1, 7])
@pytest.mark.parametrize("V", [1, 6])
def test_view_sum_is_the_ordered_fp32_sum(K, N, V):
    C = 11
    rs = np.random.RandomState(10 * N + V)
    vl = (rs.standard_normal((N, V, C)) * 10.0 ** rs.randint(-3, 4, (N, V, C))).astype(np.float32)  # the order of the adds shows
    seen = (rs.rand(N, V) < 0.7).astype(np.uint8) * np.uint8(3)    # any nonzero byte is "seen"
    seen[0] = 3
    if N > 1:
        seen[3] = 0                                                # a video without a view
        seen[5, V - 1] = 0
    want, cnt = R.view_sum_np(vl, seen)
    runs = []
    for _ in range(2):
        buf, out = KB.guarded(N, C, F32, DEV, rows=2, cols=3)
        count = torch.full((N + 1,), -7, dtype=torch.int32, device=DEV)
        K.view_sum(torch.from_numpy(vl).to(DEV), torch.from_numpy(seen).to(DEV), out, count[:N])
        torch.cuda.synchronize()
        KB.check_guards(buf, N, C, "view sum")
        assert count[N] == -7 and count[:N].cpu().numpy().tolist() == cnt.tolist()
        runs.append(out.contiguous())
    KB.assert_equal_bits(runs[0].cpu(), torch.from_numpy(want), f"view sum N {N} V {V}")
    KB.assert_equal_bits(runs[0], runs[1], "two runs")
    if N > 1:
        assert not runs[0][3].any() and cnt[3] == 0
    if V > 1:  # the case separates the stated order from another one
        rev, _ = R.view_sum_np(vl[:, ::-1], seen[:, ::-1])
        assert not np.array_equal(rev, want)


# ================================================================================================ 4. merged accuracy against compute_video
@pytest.mark.parametrize("cuts", [(), (17,), (13, 39)])
def test_merger_reproduces_the_reference_merge(K, E, fx, cuts):
    """the fixture's lines fed in one, two or three batches -- the repeated line (line 18; its first line is line 15) arrives inside
    its first line's batch or in a later one -- plus a video that never gets a view"""
    labels, lines = R.eval_lines(int(fx["merge_seed"]))
    N = R.N_VIDEOS + 1
    m = E.ViewMerger(N, R.SEG * R.CROP, R.N_CLASSES, DEV, num_crop=R.CROP)
    edges = [0, *cuts, len(lines)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        part = lines[lo:hi]
        logits = torch.from_numpy(np.stack([x for *_, x in part])).to(DEV)
        lab = torch.from_numpy(np.array([labels[v] for v, *_ in part], dtype=np.int32)).to(DEV)
        m.add(logits, lab, [R.video_id(v) for v, *_ in part], [ck for _, ck, _, _ in part], [cp for _, _, cp, _ in part])
    top1, top5 = m.result()
    assert (top1, top5) == (float(fx["merge_top"][0]), float(fx["merge_top"][1]))
    seen = m.seen.cpu().numpy()
    assert seen[:R.N_VIDEOS].sum(axis=1).tolist() == [6 - (v == R.SHORT_VIDEO) for v in range(R.N_VIDEOS)] and not seen[R.N_VIDEOS].any()
    first = next(x for v, ck, cp, x in lines if v == R.DUP_VIDEO and (ck, cp) == (1, 0))
    KB.assert_equal_bits(m.view_logits[R.DUP_VIDEO, 1 * R.CROP + 0].cpu(), torch.from_numpy(first), "the repeated line is skipped")
    assert m.labels[:R.N_VIDEOS].cpu().numpy().tolist() == labels.tolist()
    # per video, none left out: the fixture's margins (tests/test_v1_eval_cpu.py) put every comparison beyond the fp32 sums' error
    total, count = torch.empty(N, R.N_CLASSES, dtype=F32, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)
    K.view_sum(m.view_logits, m.seen, total, count)
    ranks = K.class_ranks(total, m.labels).cpu().numpy()[:R.N_VIDEOS]
    assert ((ranks < 1) * 1.0).tolist() == fx["merge_top1"].tolist() and ((ranks < 5) * 1.0).tolist() == fx["merge_top5"].tolist()
    with pytest.raises(ValueError):
        m.add(logits[:1], lab[:1], ["x"], [2], [0])
    with pytest.raises(ValueError):
        m.add(logits[:1], lab[:1], ["x"], [0], [3])
    with pytest.raises(IndexError):
        m.add(logits[:2], lab[:2], ["new1", "new2"], [0, 0], [0, 0])


# ================================================================================================ 5. end to end, tiny model
KW = S.TINY
EIMG, ET, ETSRC = KW["img_size"], 4, 8


def build(C):
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    m = VisionTransformer(num_classes=C, **KW)
    m.load_state_dict(S.synth_state(KW, 61, C), strict=True)
    return m


def source_batches(C):
    """two batches of uint8 source clips [Bs, 8, 64, 86, 3] (2 and 1 clips) with labels and ids"""
    rs = np.random.RandomState(700 + C)
    out = []
    for i, bs in enumerate((2, 1)):
        fr = torch.from_numpy(rs.randint(0, 256, (bs, ETSRC, EIMG, 86, 3)).astype(np.uint8))
        out.append((fr, torch.from_numpy(rs.randint(0, C, bs)), ["clip%d_%d" % (i, j) for j in range(bs)]))
    return out


@pytest.mark.parametrize("C", [5, 11])
def test_final_test_views_equal_forward_on_sliced_views(K, E, C, tmp_path):
    m = build(C)
    views = E.TestViews(EIMG, EIMG, 2, 3)
    batches = source_batches(C)
    # the labels of the run: the model's own view-0 prediction for the first clip, something else for the others
    want, labels = [], []
    for fr, _, _ in batches:
        plan = views.plan(fr.shape[0], ETSRC, EIMG, 86)
        sl = np.stack([R.slice_view(fr[int(r[0])].numpy(), r, plan.T, EIMG) for r in plan.view_i])
        want.append(m(torch.from_numpy(sl)))                       # uint8 [B, T, img, img, 3]: centre crop = identity
    mean0 = torch.cat(want)[:6].double().mean(0)
    labels = [int(mean0.argmax()), int(torch.cat(want)[6:12].double().mean(0).argmin()), int(torch.cat(want)[12:].double().mean(0).argsort()[-2])]
    batches = [(batches[0][0], torch.tensor(labels[:2]), batches[0][2]), (batches[1][0], torch.tensor(labels[2:]), batches[1][2])]
    merger = E.ViewMerger(3, views.per_video, C, DEV, num_crop=3)
    path = os.path.join(tmp_path, "0.txt")
    stats = E.final_test(batches, m, None, path, views=views, merger=merger)
    got = merger.view_logits.view(18, C)
    KB.assert_equal_bits(got, torch.cat(want), f"final_test view logits, C = {C}")
    # the file parses with the host merge and gives the merger's result; its lines carry the logits exactly
    assert E.merge(str(tmp_path), 1) == merger.result()
    lines = open(path).read().splitlines()
    assert len(lines) == 19 and lines[1].startswith("clip0_0 [") and lines[1].endswith("] %d 0 0" % labels[0])
    assert lines[18].startswith("clip1_0 [") and lines[18].endswith("] %d 1 2" % labels[2])
    row = np.array([float(v) for v in lines[7].split("[")[1].split("]")[0].split(",")], dtype=np.float32)
    assert np.array_equal(row, got[6].cpu().numpy())
    # the meters over the 18 views: batches of 12 and 6
    lg, lab = torch.cat(want).cpu().numpy(), np.repeat(labels, 6)
    ranks = R.class_ranks_np(lg, lab)
    for k, name in ((1, "acc1"), (5, "acc5")):
        assert stats[name] == E._meter_avg([int((ranks[:12] < k).sum()), int((ranks[12:] < k).sum())], [12, 6]), name
    assert lines[0] == "{}, {}".format(*(float(np.float32((ranks[12:] < k).sum()) * np.float32(100.0 / 6)) for k in (1, 5)))
    top1 = np.mean([(np.argmax(lg[6 * v:6 * v + 6].astype(np.float64).mean(0)) == labels[v]) * 1.0 for v in range(3)]) * 100
    assert merger.result()[0] == top1 and top1 > 0
    # file=None and no merger: the same meters
    assert E.final_test(batches, m, None, None, views=views) == stats
    # the reference's batch layout (views=None): already-cropped clips with their (chunk, split)
    plan = views.plan(2, ETSRC, EIMG, 86)
    fr = batches[0][0]
    sl = torch.from_numpy(np.stack([R.slice_view(fr[int(r[0])].numpy(), r, plan.T, EIMG) for r in plan.view_i]))
    m2 = E.ViewMerger(2, 6, C, DEV, num_crop=3)
    ref_batch = [(sl, torch.tensor(np.repeat(labels[:2], 6)), [batches[0][2][v] for v in plan.video], torch.from_numpy(plan.chunk),
                  torch.from_numpy(plan.split))]
    E.final_test(ref_batch, m, None, None, merger=m2)
    KB.assert_equal_bits(m2.view_logits.view(12, C), got[:12].contiguous(), "views=None")


def ce_loss_bound(logits, labels):
    """(float64 mean CE, its bound) as kernel_bounds.ce_check forms them for scale 1, loss0 0"""
    Rn, C = logits.shape
    x64 = logits.double()
    lse = torch.logsumexp(x64, 1)
    d = KB.lse_bound(lse, x64.max(1).values, C)
    xl = x64.gather(1, labels.long()[:, None])[:, 0]
    ref = float((lse - xl).sum()) / Rn
    return ref, float(KB.sum_bound(ref, Rn, init=0.0, c=5)) + float(d.sum()) / Rn


@pytest.mark.parametrize("C", [5, 11])
def test_validation_one_epoch_meters(K, E, C):
    m = build(C)
    g = torch.Generator().manual_seed(900 + C)
    vids = [S.synth_clip(KW, 4, ET, 901), torch.randint(0, 256, (4, ET, 70, 75, 3), dtype=torch.uint8, generator=g), S.synth_clip(KW, 1, ET, 902)]
    seen, orig = [], m.forward

    def rec(x):
        out = orig(x)
        seen.append(out.clone())
        return out
    pre = [orig(v) for v in vids]
    # labels from the model's own logits: a top-1 hit, a top-5-only hit (third place), the last place, in turn
    labels, i = [], 0
    for lg in pre:
        order = lg.argsort(dim=1, descending=True).cpu()
        lab = []
        for r in range(lg.shape[0]):
            lab.append(int(order[r, (0, 2, C - 1)[i % 3]]))
            i += 1
        labels.append(torch.tensor(lab))
    m.forward = rec
    try:
        stats = E.validation_one_epoch([(v, t, "ignored") for v, t in zip(vids, labels)], m, DEV)
    finally:
        del m.forward
    assert sorted(stats) == ["acc1", "acc5", "loss"] and len(seen) == 3
    for a, b in zip(seen, pre):
        KB.assert_equal_bits(a, b, "the logits of the run")
    h1, h5 = [], []
    for lg, lab in zip(seen, labels):
        ranks = R.class_ranks_np(lg.cpu().numpy(), lab.numpy())
        h1.append(int((ranks < 1).sum()))
        h5.append(int((ranks < 5).sum()))
    print(f"C = {C}: hits@1 {h1} hits@5 {h5} acc1 {stats['acc1']!r} acc5 {stats['acc5']!r} loss {stats['loss']!r}")
    assert stats["acc1"] == E._meter_avg(h1, [4, 4, 1]) and stats["acc5"] == E._meter_avg(h5, [4, 4, 1])
    assert abs(stats["acc1"] - 100.0 * sum(h1) / 9) < 1e-5 and abs(stats["acc5"] - 100.0 * sum(h5) / 9) < 1e-5
    assert sum(h1) == 3 and (sum(h5) == 9 if C == 5 else sum(h5) == 6)
    parts = [ce_loss_bound(lg, lab.to(DEV)) for lg, lab in zip(seen, labels)]
    ref = sum(p[0] for p in parts) / 3                               # update(loss=...) counts every batch once
    bound = sum(p[1] for p in parts) / 3 + 1e-12
    weighted = sum(p[0] * n for p, n in zip(parts, (4, 4, 1))) / 9
    print(f"loss {stats['loss']!r} ref {ref!r} bound {bound:.3g} (weighted mean {weighted!r})")
    assert abs(ref - weighted) > 1000 * bound                        # the short last batch tells the two averages apart
    assert abs(stats["loss"] - ref) <= bound
    # ce_loss_bound is ce_check's bound: ce_check accepts a loss just inside it and refuses one just outside
    r0, b0 = parts[0]
    KB.ce_check(seen[0], labels[0].to(DEV).to(torch.int32), 1.0, loss=r0 + 0.999 * b0, what="pin")
    with pytest.raises(AssertionError):
        KB.ce_check(seen[0], labels[0].to(DEV).to(torch.int32), 1.0, loss=r0 + 1.001 * b0, what="pin")
    with pytest.raises(IndexError):
        E.validation_one_epoch([(vids[2], torch.tensor([C]))], m)
    with pytest.raises(ValueError):
        E.validation_one_epoch([], m)
