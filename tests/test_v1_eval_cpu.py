"""The host side of the v1 evaluation (tvts_amd/downstream/evaluate_v1.py) against tests/golden/v1_eval.npz, which records the
reference's own test-view slicing (SSVideoClsDataset.__getitem__, mode 'test') and its compute_video / merge: the view plan, the
restatement of the slicing the GPU tests compare the gather with, the host merge, and every refusal.  No GPU."""
import os

import numpy as np
import pytest
import torch

import kernel_bounds as KB
import v1_eval_ref as R
from tvts_amd import hip as K
from tvts_amd.downstream import evaluate_v1 as E


@pytest.fixture(scope="module")
def fx(golden):
    return golden("v1_eval")


def views():
    return E.TestViews(input_size=R.SHORT, short_side_size=R.SHORT, test_num_segment=R.SEG, test_num_crop=R.CROP)


def test_fixture_is_what_the_tests_regenerate(fx):
    assert [tuple(v) for v in fx["views"].tolist()] == R.VIEWS and [tuple(s) for s in fx["sizes"].tolist()] == list(R.SIZES)
    assert tuple(fx["frame_seeds"].tolist()) == R.FRAME_SEEDS and int(fx["short"]) == R.SHORT and int(fx["tsrc"]) == R.TSRC


def test_plan_reproduces_the_recorded_views(fx):
    for k, (H0, W0) in enumerate(R.SIZES):
        plan = views().plan(1, R.TSRC, H0, W0)
        assert len(plan) == len(R.VIEWS) and plan.T == R.TSRC // 2
        assert list(zip(plan.chunk.tolist(), plan.split.tolist())) == R.VIEWS and not plan.video.any()
        assert plan.view_i[:, 1].tolist() == fx[f"t0_{k}"].tolist()
        assert plan.view_i[:, 3].tolist() == fx[f"top_{k}"].tolist()
        assert plan.view_i[:, 4].tolist() == fx[f"left_{k}"].tolist()
        assert (plan.view_i[:, 2] == 2).all() and not plan.view_i[:, 5:].any() and not plan.view_i[:, 0].any()
        K.check_view_plan(plan.view_i, Bs=1, Tsrc=R.TSRC, H0=H0, W0=W0, T=plan.T, img=R.SHORT)


def test_plan_orders_clip_major_and_takes_single_views():
    v = views()
    plan = v.plan(3, R.TSRC, 32, 48)
    assert plan.video.tolist() == [b for b in range(3) for _ in R.VIEWS] and plan.view_i[:, 0].tolist() == plan.video.tolist()
    assert list(zip(plan.chunk.tolist(), plan.split.tolist())) == R.VIEWS * 3
    one = v.plan(3, R.TSRC, 32, 48, chunk_nb=[1, 0, 1], split_nb=torch.tensor([2, 1, 0]))
    assert one.view_i[:, :5].tolist() == [[0, 1, 2, 0, 16], [1, 0, 2, 0, 8], [2, 1, 2, 0, 0]]
    # ssv2.py:151-154 with a step that is no integer: int() truncates
    big = E.TestViews(224, 224, 2, 3).plan(1, 32, 224, 299)
    assert big.view_i[:3, 4].tolist() == [0, int(1 * 37.5), int(2 * 37.5)] and big.T == 16 and not big.view_i[:, 3].any()
    tall = E.TestViews(224, 224, 2, 3).plan(1, 32, 298, 224)
    assert tall.view_i[:3, 3].tolist() == [0, 37, 74] and not tall.view_i[:, 4].any()
    sq = E.TestViews(224, 224, 2, 3).plan(1, 32, 224, 224)  # H0 == W0: the height branch, offset 0
    assert not sq.view_i[:, 3:].any()


def test_slicing_by_the_plan_gives_the_recorded_clips(fx):
    """the restatement the GPU tests hold the gather to IS the reference's returned clip: same sha256 over the whole fp32 clip"""
    for k, ((H0, W0), seed) in enumerate(zip(R.SIZES, R.FRAME_SEEDS)):
        buf = R.source_clip(seed, H0, W0)
        plan = views().plan(1, R.TSRC, H0, W0)
        for j, row in enumerate(plan.view_i):
            clip = R.normalise(R.slice_view(buf, row, plan.T, R.SHORT))
            assert np.array_equal(R.sample(clip), fx[f"sample_{k}"][j]), (k, j)
            assert R.sha(clip) == str(fx[f"sha_{k}"][j]), (k, j)


def test_merge_fixture_margins(fx):
    """every video's label mean is further from every other class mean than two fp32 sums of its views can move (sum_bound): the
    device's fp32 sums must rank every video of the fixture as the reference's float64 means do, none may be left out"""
    labels, lines = R.eval_lines(int(fx["merge_seed"]))
    assert labels.tolist() == fx["merge_labels"].tolist()
    feats = R.kept_views(lines)
    assert sorted(feats) == list(range(R.N_VIDEOS))
    assert len(feats[R.SHORT_VIDEO]) == R.SEG * R.CROP - 1 and len(feats[R.DUP_VIDEO]) == R.SEG * R.CROP
    assert sum(1 for ln in lines if ln[0] == R.DUP_VIDEO) == R.SEG * R.CROP + 1
    for v in range(R.N_VIDEOS):
        x = np.stack([d for _, d in feats[v]]).astype(np.float64)
        mean = x.mean(axis=0)
        margin = np.abs(np.delete(mean, labels[v]) - mean[labels[v]]).min()
        bound = 2.0 * float(KB.sum_bound(float(np.abs(x).sum(axis=0).max()), len(x))) / len(x)
        assert margin > bound and abs(margin - float(fx["merge_margin"][v])) < 1e-12, (v, margin, bound)
    assert 0 < fx["merge_top1"].mean() < 1 and 0 < fx["merge_top5"].mean() < 1


def test_host_merge_reproduces_the_reference(fx, tmp_path):
    labels, lines = R.eval_lines(int(fx["merge_seed"]))
    # two "ranks": the lines split over two files, the repeated line in the second one
    cut = len(lines) // 2
    R.write_file(os.path.join(tmp_path, "0.txt"), labels, lines[:cut])
    R.write_file(os.path.join(tmp_path, "1.txt"), labels, lines[cut:])
    top1, top5 = E.merge(str(tmp_path), 2)
    assert top1 == float(fx["merge_top"][0]) and top5 == float(fx["merge_top"][1])
    feats = R.kept_views(lines)
    for v in range(R.N_VIDEOS):
        pred, t1, t5 = E.compute_video([d.astype(np.float64) for _, d in feats[v]], labels[v])
        assert (pred, t1, t5) == (int(fx["merge_pred"][v]), float(fx["merge_top1"][v]), float(fx["merge_top5"][v])), v
    assert E.compute_video([], 0) is None
    # the restated definitions of the two kernels agree with it on the fixture
    vl = np.zeros((R.N_VIDEOS, R.SEG * R.CROP, R.N_CLASSES), dtype=np.float32)
    seen = np.zeros(vl.shape[:2], dtype=np.uint8)
    for v in feats:
        for slot, d in feats[v]:
            vl[v, slot], seen[v, slot] = d, 1
    total, count = R.view_sum_np(vl, seen)
    ranks = R.class_ranks_np(total, labels)
    assert count.tolist() == [len(feats[v]) for v in range(R.N_VIDEOS)]
    assert ((ranks < 1) * 1.0).tolist() == fx["merge_top1"].tolist() and ((ranks < 5) * 1.0).tolist() == fx["merge_top5"].tolist()


def test_meter_average_is_the_reference_s():
    """acc: fp32 percentage per batch, weighted by batch size; three batches of 4, 4, 1"""
    got = E._meter_avg([3, 1, 1], [4, 4, 1])
    want = (float(np.float32(3) * np.float32(25.0)) * 4 + float(np.float32(1) * np.float32(25.0)) * 4 + 100.0) / 9
    assert got == want and abs(got - 100 * 5 / 9) < 1e-9


def test_refusals():
    with pytest.raises(ValueError, match="test_num_crop"):
        E.TestViews(32, 32, 2, 1)
    with pytest.raises(ValueError, match="short_side_size"):
        E.TestViews(32, 40, 2, 3)
    v = views()
    with pytest.raises(ValueError, match="short side"):
        v.plan(1, R.TSRC, 40, 48)
    with pytest.raises(ValueError, match="test_num_segment"):
        v.plan(1, 7, 32, 48)                      # odd frame count: chunk 0 has 4 frames, chunk 1 has 3
    with pytest.raises(ValueError, match="test_num_segment"):
        E.TestViews(32, 32, 3, 3).plan(1, 8, 32, 48)  # chunk 2 is shorter than chunk 0
    with pytest.raises(ValueError, match="test_num_segment"):
        v.plan(1, 1, 32, 48)                      # chunk 1 of a one-frame clip is empty
    with pytest.raises(ValueError):
        v.plan(2, R.TSRC, 32, 48, chunk_nb=[0, 2], split_nb=[0, 0])
    with pytest.raises(ValueError):
        v.plan(2, R.TSRC, 32, 48, chunk_nb=[0, 1], split_nb=[0, 3])
    with pytest.raises(ValueError):
        v.plan(2, R.TSRC, 32, 48, chunk_nb=[0, 1])
    assert E.TestViews(32, 32, 1, 3).plan(1, 7, 32, 48).T == 4  # one segment: nothing to be ragged against


def test_view_table_host_check():
    kw = dict(Bs=2, Tsrc=8, H0=32, W0=48, T=4, img=32)
    good = np.array([[0, 0, 2, 0, 0, 0, 0, 0], [1, 1, 2, 0, 16, 0, 0, 0]], dtype=np.int64)
    out = K.check_view_plan(good, **kw)
    assert out.dtype == np.int32 and out.flags["C_CONTIGUOUS"] and out.tolist() == good.tolist()
    K.check_view_plan([[0, 4, 1, 0, 0, 0, 0, 0]], **kw)  # the last frame is frame Tsrc - 1
    for col, val in ((0, -1), (0, 2), (1, -1), (1, 2), (2, 0), (2, 3), (3, -1), (3, 1), (4, -1), (4, 17), (5, 1), (7, -1)):
        bad = good.copy()
        bad[1, col] = val
        with pytest.raises(ValueError):
            K.check_view_plan(bad, **kw)
    with pytest.raises(ValueError):
        K.check_view_plan(good[:, :6], **kw)
    with pytest.raises(ValueError):
        K.check_view_plan(good.astype(np.float32), **kw)
    with pytest.raises(ValueError):
        K.check_view_plan(good, **dict(kw, H0=31))
    with pytest.raises(ValueError):
        K.check_view_plan(good, **dict(kw, T=5))
