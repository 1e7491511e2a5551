"""CPU-side checks of the v1 pretraining step's uint8 input: the host tap tables against Pillow itself and against the fixture the
reference's transform left (tests/golden/v1_input.npz), the crop draw of U8VideoTransform, the packing of ragged clips, the refusals
of prepare_batch that need no GPU, and the -22 refusals of tvts_resize_crop_u8 (no GPU is present here: nothing is launched)."""
import ctypes
import random

import numpy as np
import pytest
import torch

from tvts_amd import _lib
from tvts_amd import arch as A
from tvts_amd import hip as K
from tvts_amd.data_loader import transforms as TR
from tvts_amd.data_loader.v1_input import U8VideoTransform, collate_u8, pack_clips
from tvts_amd.engine_v1 import EngineV1
from v1_input_ref import resample_u8

PAIRS = [(9, 5), (64, 36), (30, 60), (19, 20), (80, 36), (426, 476), (640, 476), (5, 7), (38, 38)]


def _clips(golden):
    f = golden("v1_input")
    return f, [dict(src=f[f"src.{i}"], crop=f[f"crop.{i}"], u8=f[f"u8.{i}"], f32=f[f"f32.{i}"], mode=str(f["mode"][i]))
               for i in range(int(f["n"]))]


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_bilinear_coeffs_are_pillows_taps(n_in, n_out):
    """every tap read back from Pillow by a one-hot line.  A uint8 probe cannot carry 22 bits, so the line is a 32-bit integer
    image (mode 'I'): Pillow resamples it with the SAME normalised double weights of precompute_coeffs, before their fixed-point
    conversion, and rounds half up -- a source pixel of 2^22 at x comes back as int(0.5 + w[x] * 2^22) in every output, the tap."""
    Image = pytest.importorskip("PIL.Image")
    rows = TR.pil_bilinear_coeffs(n_in, n_out)
    assert len(rows) == n_out
    got = np.zeros((n_out, n_in), dtype=np.int64)
    for i, (first, k) in enumerate(rows):
        assert first >= 0 and len(k) >= 1 and first + len(k) <= n_in and min(k) >= 0
        got[i, first:first + len(k)] = k
    one = 1 << TR.PIL_PRECISION_BITS
    for x in range(n_in):
        line = np.zeros((1, n_in), dtype=np.int32)
        line[0, x] = one
        back = np.asarray(Image.fromarray(line).resize((n_out, 1), Image.BILINEAR))[0]
        assert np.array_equal(back.astype(np.int64), got[:, x]), (x, back, got[:, x])
    assert abs(int(got.sum(1).max()) - one) <= max(len(k) for _, k in rows) and TR.pil_bilinear_coeffs(n_in, n_out) is rows  # cached


@pytest.mark.parametrize("hs,ws,nh,nw", [(7, 9, 4, 5), (36, 64, 20, 36), (64, 36, 36, 20), (20, 30, 40, 60), (19, 19, 20, 20),
                                         (45, 80, 20, 36), (240, 426, 268, 476), (360, 640, 268, 476), (1, 5, 3, 7), (38, 51, 38, 51)])
def test_two_pass_restatement_equals_pillow(hs, ws, nh, nw):
    Image = pytest.importorskip("PIL.Image")
    src = np.random.RandomState(hs * 1000 + ws).randint(0, 256, size=(hs, ws, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(src).resize((nw, nh), Image.BILINEAR))
    assert np.array_equal(resample_u8(src, nh, nw), want)


def test_restatement_equals_the_reference_fixture(golden):
    """runs where Pillow is absent: Resize(38) + the recorded crop of every fixture clip"""
    f, clips = _clips(golden)
    size, c = int(f["resize"]), int(f["crop_size"])
    for i, cl in enumerate(clips):
        hs, ws = cl["src"].shape[1:3]
        nh, nw = TR.resize_sizes(hs, ws, size)
        top, left = (int(v) for v in cl["crop"])
        got = resample_u8(cl["src"], nh, nw)[:, top:top + c, left:left + c]
        assert np.array_equal(got, cl["u8"]), i
    assert TR.resize_sizes(38, 51, 38) == (38, 51)  # the clip the reference returns untouched: identity taps
    for i, (first, k) in enumerate(TR.pil_bilinear_coeffs(38, 38)):
        assert [(first + j, v) for j, v in enumerate(k) if v] == [(i, 1 << 22)]


def test_u8_transform_draws_the_reference_crops(golden):
    f, clips = _clips(golden)
    random.seed(int(f["seed"]))
    tf = {m: U8VideoTransform(m, crop_size=int(f["crop_size"])) for m in ("train", "test")}
    for i, cl in enumerate(clips):
        s = tf[cl["mode"]](torch.from_numpy(cl["src"]).permute(3, 0, 1, 2))
        assert s["resize"] == int(f["resize"]) and tuple(s["crop"]) == tuple(int(v) for v in cl["crop"]), (i, s["crop"], cl["crop"])
        assert s["video"].dtype == torch.uint8 and np.array_equal(s["video"].numpy(), cl["src"])
    with pytest.raises(ValueError):
        tf["train"](torch.zeros(4, 3, 20, 20))
    for d in range(9):
        assert TR.centre_crop_offset(d) == int(round(d / 2.)) == (d >> 1) + ((d & 1) & (d >> 1))


def _engine(**over):
    eng = EngineV1.__new__(EngineV1)  # (the host half of prepare_batch reads the architecture alone)
    eng.arch = A.small_arch_v1(image=32, **over)
    return eng


def test_collate_packs_ragged_clips_at_the_descriptor_offsets(golden):
    f, clips = _clips(golden)
    samples = [dict(video=torch.from_numpy(cl["src"]), crop=tuple(int(v) for v in cl["crop"]), resize=int(f["resize"]), idx=torch.tensor(i))
               for i, cl in enumerate(clips)]
    data = collate_u8(samples)
    assert isinstance(data["video"], list) and data["crop"].dtype == torch.int32 and tuple(data["crop"].shape) == (5, 2)
    assert torch.equal(data["idx"], torch.arange(5)) and data["resize"] == 38
    u8 = _engine()._u8_batch(data)
    plan = u8["plan"]
    assert u8["B"] == 5 and u8["T"] == 4 and plan["desc"].dtype == np.int64 and plan["tables"].dtype == np.int32
    buf = pack_clips(u8["clips"], plan["offsets"], torch.full((plan["nbytes"] + 5,), 0xEE, dtype=torch.uint8))
    assert bool((buf[plan["nbytes"]:] == 0xEE).all())
    end = 0
    for b, cl in enumerate(clips):
        off, hs, ws, top, left, yt, xt, zero = plan["desc"][b].tolist()
        assert (hs, ws) == cl["src"].shape[1:3] and (top, left) == tuple(int(v) for v in cl["crop"]) and zero == 0 and off == end
        assert np.array_equal(buf[off:off + cl["src"].size].numpy(), cl["src"].reshape(-1))
        for loc, n_in in ((yt, hs), (xt, ws)):
            n_out = int(plan["tables"][loc + 1])
            assert int(plan["tables"][loc]) == n_in and np.array_equal(plan["tables"][loc:loc + K.resize_table(n_in, n_out).size],
                                                                       K.resize_table(n_in, n_out))
        end = off + cl["src"].size
    assert plan["nbytes"] == end
    # 45 x 80 and 80 x 45 share their two tables; 38 -> 38 is shared by the rows of clip 3 and nothing else
    assert plan["desc"][0, 5] == plan["desc"][1, 6] and plan["desc"][0, 6] == plan["desc"][1, 5]
    assert K.check_resize_plan(plan["desc"], plan["tables"], T=4, img=32, src_bytes=plan["nbytes"]) == plan["tmp_rows"]
    same = collate_u8(samples[:1] * 3)
    assert torch.is_tensor(same["video"]) and tuple(same["video"].shape) == (3, 4, 45, 80, 3)


def test_resize_plan_check_refuses_bad_plans():
    plan = K.resize_plan([(45, 80), (80, 45)], [(4, 17), (32, 2)], size=38, img=32, T=2)
    ok = lambda desc=plan["desc"], tables=plan["tables"], nbytes=plan["nbytes"]: K.check_resize_plan(  # noqa: E731
        desc, tables, T=2, img=32, src_bytes=nbytes)
    assert ok() == plan["tmp_rows"] and 32 <= plan["tmp_rows"] <= 45
    for col, val in ((0, -1), (0, plan["nbytes"]), (3, 7), (3, -1), (4, 36), (5, 3), (5, len(plan["tables"])), (6, int(plan["desc"][0, 5])),
                     (7, 1), (1, 44)):
        d = plan["desc"].copy()
        d[0, col] = val
        with pytest.raises(ValueError):
            ok(desc=d)
    t = plan["tables"].copy()
    t[-1] += 1
    with pytest.raises(ValueError):
        ok(tables=t)
    with pytest.raises(ValueError):
        ok(nbytes=plan["nbytes"] - 1)
    with pytest.raises(ValueError, match="below the crop"):
        K.resize_plan([(45, 80)], None, size=30, img=32, T=2)
    centre = K.resize_plan([(45, 80)], None, size=38, img=32, T=2)["desc"][0]
    assert (centre[3], centre[4]) == (3, TR.centre_crop_offset(67 - 32))


def test_prepare_batch_refusals_without_a_gpu():
    eng = _engine()
    text = dict(input_ids=torch.ones(2, 4, dtype=torch.int64), attention_mask=torch.ones(2, 4, dtype=torch.int64))
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    base = dict(text=text, keep_ind=torch.zeros(2, 4, 2, dtype=torch.int64))
    for video, extra, msg in (
            ([u8(4, 45, 80, 3), u8(3, 45, 80, 3)], dict(resize=38), "frames"),                 # a clip shorter than T
            (u8(2, 4, 45, 80, 3), dict(resize=30), "below the crop"),                           # resized side below img
            (u8(2, 4, 31, 80, 3), {}, "below the crop"),                                        # the same without a resize
            (u8(2, 4, 45, 80, 3), dict(resize=38, crop=torch.tensor([[7, 0], [0, 0]])), "crop outside"),
            (u8(2, 4, 45, 80, 3), dict(resize=38, crop=torch.tensor([[0, 0], [0, 36]])), "crop outside"),
            (u8(2, 4, 38, 67, 3), dict(crop=torch.tensor([[0, 0], [-1, 0]])), "crop outside"),
            (u8(2, 4, 38, 67, 3), dict(crop=torch.tensor([[0, 36], [0, 0]])), "crop outside"),
            (u8(2, 4, 3, 38, 67), {}, r"\[B, T, H, W, 3\]"),                                    # channel-major uint8
            ([u8(4, 3, 45, 80)] * 2, dict(resize=38), r"\[B, T, H, W, 3\]"),
            ([u8(4, 45, 80, 3)] * 2, {}, "resize")):                                            # a list without a resize
        with pytest.raises(ValueError, match=msg):
            EngineV1.prepare_batch(eng, dict(base, video=video, **extra))
    with pytest.raises(KeyError, match="mask_seed"):
        EngineV1.prepare_batch(eng, dict(text=text, video=u8(2, 4, 38, 67, 3)))
    assert eng._u8_batch(dict(video=torch.zeros(2, 4, 3, 32, 32))) is None  # fp32 clips: the path of before


def _buf(n=64):
    return ctypes.cast(ctypes.create_string_buffer(n), ctypes.c_void_p)


def test_resize_entry_point_refuses_bad_arguments():
    lib = _lib.load()
    assert "tvts_resize_crop_u8" in _lib.parse_header()
    src = open(_lib.HEADER_PATH).read()
    assert "videoaug.py:8-22" in src and "functional.py:56-59" in src
    call = lambda src=_buf(), desc=_buf(), tables=_buf(), B=2, T=2, img=32, rows=40, tmp=_buf(), nb=2 * 2 * 40 * 32 * 3, out=_buf(), ldo=96: \
        lib.tvts_resize_crop_u8(src, desc, tables, B, T, img, rows, tmp, nb, out, ldo, None)  # noqa: E731
    for kw in (dict(src=None), dict(desc=None), dict(tables=None), dict(tmp=None), dict(out=None), dict(B=0), dict(B=-1), dict(T=0),
               dict(img=0), dict(img=-32), dict(rows=0), dict(nb=2 * 2 * 40 * 32 * 3 - 1), dict(nb=0), dict(ldo=95), dict(B=65536)):
        assert call(**kw) == -22, kw
