"""The host half of the v2 step's ragged uint8 input (DESIGN.md 8j "v2 ragged"): the plan builder and its check, the refusals of
prepare_batch, the host restatement against the reference's own outputs, split_batch over a list and the dataset side.  No GPU is
needed: nothing is launched (the entry point's -22 refusals return before any launch)."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ragged_ref as RR  # noqa: E402

from tvts_amd import _lib  # noqa: E402
from tvts_amd import arch as A  # noqa: E402
from tvts_amd import hip as K  # noqa: E402
from tvts_amd.data_loader import transforms as TR  # noqa: E402
from tvts_amd.data_loader.v2_input import U8VideoTransform, collate_u8_v2, failed_clip  # noqa: E402
from tvts_amd.engine import Engine  # noqa: E402
from tvts_amd.step import split_batch  # noqa: E402

TAGS = ("wide", "tall", "same")


def u8(*s):
    return torch.zeros(*s, dtype=torch.uint8)


def table_at(plan, loc):
    n_in, n_out = (int(v) for v in plan["tables"][loc:loc + 2])
    return n_in, n_out, plan["tables"][loc + 2:loc + 2 + n_out].tolist()


# ---------------------------------------------------------------------------------------------- the plan builder
def test_gather_plan_is_pillows_tables_shared_per_axis_pair():
    # landscape, portrait (its transposed pairs), an unresized axis pair (short side == size: left alone), an upscaled square
    sizes, frames = [(57, 90), (90, 57), (48, 70), (30, 30)], [3, 1, 2, 3]
    plan = K.gather_plan(sizes, frames, None, size=48, img=40, T=3)
    desc, tables = plan["desc"], plan["tables"]
    assert desc.dtype == np.int64 and desc.shape == (4, 8) and tables.dtype == np.int32 and tables.ndim == 1
    end = 0
    for b, ((hs, ws), fr) in enumerate(zip(sizes, frames)):
        off, dh, dw, top, left, yt, xt, dfr = desc[b].tolist()
        nh, nw = TR.resize_sizes(hs, ws, 48)
        assert (off, dh, dw, dfr) == (end, hs, ws, fr)
        assert table_at(plan, yt) == (hs, nh, TR.pil_nearest_table(hs, nh)) and table_at(plan, xt) == (ws, nw, TR.pil_nearest_table(ws, nw))
        assert (top, left) == (TR.centre_crop_offset(nh - 40), TR.centre_crop_offset(nw - 40))
        end += fr * hs * ws * 3  # a short clip occupies its own frames only
    assert plan["nbytes"] == end and plan["offsets"].tolist() == desc[:, 0].tolist()
    assert TR.resize_sizes(48, 70, 48) == (48, 70) and table_at(plan, int(desc[2, 5]))[2] == list(range(48))  # identity, no special case
    assert table_at(plan, int(desc[2, 6])) == (70, 70, list(range(70)))
    # 57 x 90 and 90 x 57 share both tables; the square's two axes share one; six distinct (n_in, n_out) in all
    assert desc[0, 5] == desc[1, 6] and desc[0, 6] == desc[1, 5] and desc[3, 5] == desc[3, 6]
    pairs = {(57, 48), (90, 75), (48, 48), (70, 70), (30, 48)}
    assert tables.size == sum(2 + n_out for _, n_out in pairs)
    # size=None: no Resize, identity tables of the source sides; explicit crops and offsets are taken as given
    p2 = K.gather_plan([(41, 50), (50, 41)], [2, 2], [(1, 10), (0, 0)], size=None, img=40, T=2, offsets=[3, 3 + 2 * 41 * 50 * 3 + 1])
    assert p2["desc"][:, 3:5].tolist() == [[1, 10], [0, 0]] and p2["desc"][:, 0].tolist() == [3, 12304]
    assert p2["nbytes"] == 12304 + 2 * 50 * 41 * 3
    assert table_at(p2, int(p2["desc"][0, 5])) == (41, 41, list(range(41))) and p2["desc"][0, 6] == p2["desc"][1, 5]
    K.check_gather_plan(p2["desc"], p2["tables"], T=2, img=40, src_bytes=p2["nbytes"])


# ---------------------------------------------------------------------------------------------- refusals
def test_check_gather_plan_refuses_one_broken_plan_per_rule():
    plan = K.gather_plan([(57, 90), (90, 57)], [2, 1], [(4, 17), (35, 2)], size=48, img=40, T=2)
    ok = lambda desc=plan["desc"], tables=plan["tables"], nbytes=plan["nbytes"], T=2: K.check_gather_plan(  # noqa: E731
        desc, tables, T=T, img=40, src_bytes=nbytes)
    ok()
    yt0, xt0 = int(plan["desc"][0, 5]), int(plan["desc"][0, 6])
    for col, val, msg in ((0, -1, "leaves the buffer"), (0, plan["nbytes"], "leaves the buffer"), (1, 58, "leaves the buffer|side of 58"),
                          (5, -1, "names a table"), (5, len(plan["tables"]) - 1, "names a table"), (5, 3, "is not pil_nearest_table"),
                          (6, yt0, "side of 90, its table resamples 57"), (3, 9, "crop outside"), (3, -1, "crop outside"),
                          (4, 36, "crop outside"), (4, -1, "crop outside"), (7, 0, "frames"), (7, 3, "frames"), (7, -1, "frames")):
        d = plan["desc"].copy()
        d[0, col] = val
        with pytest.raises(ValueError, match=msg):
            ok(desc=d)
    t = plan["tables"].copy()
    t[xt0 + 2 + 5] += 1  # one wrong source index
    with pytest.raises(ValueError, match="is not pil_nearest_table"):
        ok(tables=t)
    with pytest.raises(ValueError, match="leaves the buffer"):
        ok(nbytes=plan["nbytes"] - 1)
    with pytest.raises(ValueError, match="frames"):
        ok(T=1)
    small = K.gather_plan([(57, 90)], [1], None, size=48, img=40, T=1)  # a valid plan for img 40 resizes to 48 x 75: below img 64
    with pytest.raises(ValueError, match="below the crop"):
        K.check_gather_plan(small["desc"], small["tables"], T=1, img=64, src_bytes=small["nbytes"])
    with pytest.raises(ValueError, match="below the crop"):
        K.gather_plan([(57, 90)], [1], None, size=30, img=40, T=1)
    with pytest.raises(ValueError, match="integer desc"):
        K.check_gather_plan(plan["desc"].astype(np.float32), plan["tables"], T=2, img=40, src_bytes=plan["nbytes"])
    # check_resize_plan is the v1 plan's and stays what it was: a gather plan's last column (frames) is nonzero there
    with pytest.raises(ValueError):
        K.check_resize_plan(plan["desc"], plan["tables"], T=2, img=40, src_bytes=plan["nbytes"])


def _engine(**over):
    eng = Engine.__new__(Engine)  # (the host half of prepare_batch reads the architecture alone)
    eng.arch = A.small_arch(image=40, patch=8, **over)
    return eng


def test_prepare_batch_refusals_without_a_gpu():
    eng = _engine(num_frames=4)
    base = dict(text=torch.ones(2, 4, dtype=torch.int64), keep_ind=torch.zeros(2, 3, dtype=torch.int64))
    for video, extra, msg in (
            ([u8(2, 57, 90, 3), u8(2, 57, 90, 3).float()], dict(resize=48), r"uint8 tensor \[T, Hs, Ws, 3\]"),   # not uint8
            ([u8(2, 3, 57, 90), u8(2, 57, 90, 3)], dict(resize=48), r"uint8 tensor \[T, Hs, Ws, 3\]"),           # channel-major
            ([u8(2, 57, 90, 3), u8(57, 90, 3)], dict(resize=48), r"uint8 tensor \[T, Hs, Ws, 3\]"),              # no frame axis
            ([u8(2, 57, 90, 3), np.zeros((2, 57, 90, 3), np.uint8)], dict(resize=48), r"uint8 tensor \[T, Hs, Ws, 3\]"),
            ([], dict(resize=48), "empty list"),
            ([u8(2, 57, 90, 3), u8(0, 57, 90, 3)], dict(resize=48), "clip 1 has no frames"),
            ([u8(2, 57, 90, 3), u8(3, 57, 90, 3)], dict(resize=48, num_frames=2), "clip 1 has 3 frames, more than"),
            ([u8(5, 57, 90, 3), u8(3, 57, 90, 3)], dict(resize=48), "temporal embedding has 4 rows"),
            ([u8(2, 57, 90, 3), u8(1, 57, 90, 3)], dict(resize=48, num_frames=5), "temporal embedding has 4 rows"),
            ([u8(2, 57, 90, 3), u8(2, 90, 57, 3)], dict(resize=30), "below the crop"),                           # resized side below img
            ([u8(2, 57, 90, 3), u8(2, 39, 90, 3)], {}, "below the crop"),                                        # the same, no Resize
            ([u8(2, 57, 90, 3), u8(2, 90, 57, 3)], dict(resize=48, crop=torch.tensor([[9, 0], [0, 0]])), "crop outside"),
            ([u8(2, 57, 90, 3), u8(2, 90, 57, 3)], dict(resize=48, crop=torch.tensor([[0, 0], [0, 9]])), "crop outside"),
            ([u8(2, 57, 90, 3), u8(2, 90, 57, 3)], dict(resize=48, crop=torch.tensor([[0, -1], [0, 0]])), "crop outside"),
            ([u8(2, 57, 90, 3), u8(2, 90, 57, 3)], dict(crop=torch.tensor([[17, 50], [51, 17]])), "crop outside"),  # clip 1: top 51 > 90 - 40
            ([u8(2, 57, 90, 3), u8(2, 90, 57, 3)], dict(resize=48, crop=torch.tensor([[0, 0]])), r"crop \(1, 2\)")):
        with pytest.raises(ValueError, match=msg):
            Engine.prepare_batch(eng, dict(base, video=video, **extra))  # (an engine without a device: every refusal is the host's)
    clips, plan, B, T = eng._ragged_batch(dict(video=(u8(2, 57, 90, 3), u8(1, 90, 57, 3)), resize=48, num_frames=3))
    assert (B, T) == (2, 3) and plan["desc"][:, 7].tolist() == [2, 1] and plan["nbytes"] == 3 * 57 * 90 * 3


def test_entry_point_refuses_bad_arguments():
    lib = _lib.load()
    assert "tvts_patch_gather_u8_ragged" in _lib.parse_header()
    src = open(_lib.HEADER_PATH).read()
    assert "base_dataset.py:116-130" in src and "functional.py:47-78" in src and "check_gather_plan" in src
    buf = lambda n=64: ctypes.cast(ctypes.create_string_buffer(n), ctypes.c_void_p)  # noqa: E731
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    call = lambda src=buf(), desc=buf(), tables=buf(), keep=buf(), B=2, T=2, n=3, img=64, patch=16, mean=f3, std=f3, out=buf(), ldo=768: \
        lib.tvts_patch_gather_u8_ragged(src, desc, tables, keep, B, T, n, img, patch, mean, std, out, ldo, None)  # noqa: E731
    for kw in (dict(src=None), dict(desc=None), dict(tables=None), dict(keep=None), dict(out=None), dict(mean=None), dict(std=None),
               dict(B=0), dict(B=-1), dict(T=0), dict(n=0), dict(patch=0), dict(patch=-16), dict(img=0), dict(img=-64), dict(img=60),
               dict(ldo=772), dict(ldo=760), dict(patch=14, img=56, ldo=584)):
        assert call(**kw) == -22, kw


# ---------------------------------------------------------------------------------------------- the restatement is the reference's
def test_restatement_equals_the_reference_fixture(golden):
    """Resize(48) nearest + CenterCrop(40) / the crop (3, 5) + ClipToTensor + Normalize of every fixture clip, and the zero frames
    behind a short clip: the reference of the GPU tests, against the arrays the reference's own chain wrote"""
    f = golden("transform_resize")
    img, size, crop = int(f["image"]), int(f["size"]), [int(v) for v in f["crop_yx"]]
    clips = [torch.tensor(f["frames_" + t]) for t in TAGS]
    for crops, key in ((None, "out_"), ([crop] * 3, "out_crop_")):
        got = RR.restate(clips, crops, size, img, 3)
        for b, t in enumerate(TAGS):
            assert torch.equal(got[b], torch.tensor(f[key + t])), key + t
    short = RR.restate([clips[0][:1], clips[1][:2], clips[2]], None, size, img, 4)
    assert torch.equal(short[0, :1], torch.tensor(f["out_wide"])[:1]) and torch.equal(short[1, :2], torch.tensor(f["out_tall"])[:2])
    for z in (short[0, 1:], short[1, 2:], short[2, 3:]):  # final = zeros; final[:n] = imgs -- +0 in every bit
        assert z.numel() and not z.view(torch.int32).any()
    for b, t in enumerate(TAGS):
        assert list(RR.resized_hw(*clips[b].shape[1:3], size)) == list(f["resized_hw_" + t])


# ---------------------------------------------------------------------------------------------- split_batch
def test_split_batch_slices_a_list_by_clip_and_carries_num_frames():
    clips = [torch.full((fr, 41 + b, 50, 3), b, dtype=torch.uint8) for b, fr in enumerate((3, 2, 1, 1))]
    text = torch.arange(2 * 4 * 5).reshape(8, 5)  # transcript-major: row t * B + b
    data = dict(video=clips, text=text, crop=torch.arange(8).reshape(4, 2), resize=48, mask_seed=3, meta="m")
    chunks = split_batch(data, 2)
    for k, c in enumerate(chunks):
        assert isinstance(c["video"], list) and len(c["video"]) == 2
        assert all(c["video"][j] is clips[2 * k + j] for j in range(2))
        assert c["num_frames"] == 3 and c["resize"] == 48 and c["meta"] == "m" and c["sample_offset"] == 2 * k
        assert torch.equal(c["crop"], data["crop"][2 * k:2 * k + 2])
        assert torch.equal(c["text"], text.reshape(2, 4, 5)[:, 2 * k:2 * k + 2].reshape(4, 5))
    assert [c["num_frames"] for c in split_batch(dict(data, num_frames=4), 4)] == [4] * 4  # a given T is carried as it is
    assert split_batch(dict(data, video=tuple(clips)), 1)[0]["video"] == clips
    # each chunk is planned on its own, with the whole batch's T: the second chunk holds short clips only
    eng = _engine()
    plans = [eng._ragged_batch(dict(c, crop=None)) for c in chunks]
    assert [p[3] for p in plans] == [3, 3] and plans[1][1]["desc"][:, 7].tolist() == [1, 1] and plans[1][1]["desc"][0, 0] == 0
    with pytest.raises(ValueError, match="does not divide"):
        split_batch(data, 3)
    with pytest.raises(ValueError, match="empty list"):
        split_batch(dict(data, video=[]), 1)
    with pytest.raises(ValueError, match="uint8 clips"):
        split_batch(dict(data, video=[clips[0], 3, clips[1], clips[2]]), 2)
    # tensors: what it was (no num_frames appears)
    t = split_batch(dict(video=torch.zeros(4, 2, 3, 8, 8), text=text), 2)
    assert "num_frames" not in t[0] and tuple(t[1]["video"].shape) == (2, 2, 3, 8, 8)


# ---------------------------------------------------------------------------------------------- the dataset side
def test_v2_input_draws_the_reference_crops_and_collates():
    tf = {m: U8VideoTransform(m, crop_size=40) for m in ("train", "test")}
    assert tf["train"].resize == 48
    shapes = [(3, 57, 90), (2, 101, 64), (3, 48, 70), (1, 40, 40)]
    g = torch.Generator().manual_seed(5)
    raw = [torch.randint(0, 256, (3, t, h, w), generator=g).float() for t, h, w in shapes]  # [C, T, H, W] byte values, as the reader's
    raw[3] = failed_clip(40).permute(3, 0, 1, 2).float()
    random.seed(11)
    samples = [dict(tf["train"](c), idx=torch.tensor(i)) for i, c in enumerate(raw)]
    random.seed(11)
    for s, (t, h, w) in zip(samples, shapes):
        nh, nw = TR.resize_sizes(h, w, 48)
        x1 = random.randint(0, nw - 40)  # video_transform.py:228-229: x1 first, then y1
        y1 = random.randint(0, nh - 40)
        assert tuple(s["crop"]) == (y1, x1) and s["resize"] == 48 and tuple(s["video"].shape) == (t, h, w, 3)
    c = tf["test"](raw[0])
    assert tuple(c["crop"]) == (TR.centre_crop_offset(48 - 40), TR.centre_crop_offset(75 - 40)) == (4, 18)
    fc = failed_clip(40)
    assert fc.dtype == torch.uint8 and tuple(fc.shape) == (1, 40, 40, 3) and not fc.any()
    with pytest.raises(ValueError):
        failed_clip(0)
    data = collate_u8_v2(samples, dict(num_frames=3, input_res=40))
    assert isinstance(data["video"], list) and data["num_frames"] == 3 and data["resize"] == 48
    assert data["crop"].dtype == torch.int32 and tuple(data["crop"].shape) == (4, 2) and torch.equal(data["idx"], torch.arange(4))
    same = collate_u8_v2([samples[0]] * 2, dict(num_frames=3))
    assert torch.is_tensor(same["video"]) and tuple(same["video"].shape) == (2, 3, 57, 90, 3) and same["num_frames"] == 3
    short = collate_u8_v2([samples[1]] * 2, dict(num_frames=3))  # equal shapes but short: a list, so that the batch is padded
    assert isinstance(short["video"], list) and len(short["video"]) == 2 and tuple(short["video"][0].shape) == (2, 101, 64, 3)
    with pytest.raises(ValueError, match="num_frames"):
        collate_u8_v2(samples, dict(num_frames=2))
    # the collated batch is one the engine's host half takes, the failed clip as one black frame behind its own Resize
    clips, plan, B, T = _engine()._ragged_batch(data)
    assert (B, T) == (4, 3) and plan["desc"][:, 7].tolist() == [3, 2, 3, 1] and plan["desc"][3, 1:3].tolist() == [40, 40]
    assert table_at(plan, int(plan["desc"][3, 5]))[:2] == (40, 48)
    want = RR.restate(clips, data["crop"].tolist(), 48, 40, 3)
    assert not want[3, 1:].view(torch.int32).any() and float(want[3, 0].max()) < 0  # black behind Normalize, then zero frames
