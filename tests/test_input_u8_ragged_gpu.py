"""The v2 step's ragged uint8 input on the device (run with -m gpu; DESIGN.md 8j "v2 ragged"): tvts_patch_gather_u8_ragged against the
reference's own outputs (tests/golden/transform_resize.npz) and against tvts_patch_gather_u8_resized run clip by clip, bit for bit; the
zero frames behind short clips; the model, the training step, the micro-batched step, the encoder and GraphReplay on lists of
clips against the fp32 clips of the host restatement (tests/ragged_ref.py, held to the fixture by the CPU test).  Every plan goes
through check_gather_plan before its launch; src and out sit between guard regions that must come back untouched."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ragged_ref as RR  # noqa: E402
from test_model_gpu import check_grads  # noqa: E402
from test_train_guard_gpu import bits, make, same_bits, same_state, snapshot  # noqa: E402

from oracle import tvts_oracle as O  # noqa: E402  (checker only)

DEV = "cuda:0"
TAGS = ("wide", "tall", "same")
GUARD, SRC_FILL, OUT_FILL = 509, 0xA5, 9.0  # (an odd guard: the packed buffer itself starts at an odd address)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return True


def run_ragged(clips, frames, crops, keep, *, size, img, patch, T, gaps=None):
    """one launch over the clips (clip b cut to frames[b] pictures, gaps[b] pad bytes in front of it) -> bf16 rows [B * T * n, ldo]
    on the host.  The plan is checked on the host first; src and out lie between guard regions, asserted untouched."""
    from tvts_amd import hip as K
    B, n = len(clips), keep.shape[1]
    clips = [c[:fr] for c, fr in zip(clips, frames)]
    offs, total = RR.pack(clips, gaps or [0] * B)
    plan = K.gather_plan([tuple(c.shape[1:3]) for c in clips], frames, crops, size=size, img=img, T=T, offsets=offs)
    assert plan["nbytes"] == total
    K.check_gather_plan(plan["desc"], plan["tables"], T=T, img=img, src_bytes=total)
    host = torch.full((GUARD + total + GUARD,), SRC_FILL, dtype=torch.uint8)
    for c, off in zip(clips, offs):
        host[GUARD + off:GUARD + off + c.numel()] = c.reshape(-1)
    buf = host.to(DEV)
    Kc = 3 * patch * patch
    ldo = -(-Kc // 64) * 64
    rows = B * T * n
    big = torch.full((rows + 16, ldo), OUT_FILL, dtype=torch.bfloat16, device=DEV)
    K.patch_gather_u8_ragged(buf[GUARD:GUARD + total], torch.from_numpy(plan["desc"]).to(DEV), torch.from_numpy(plan["tables"]).to(DEV),
                             keep.to(torch.int32).to(DEV).contiguous(), big[8:8 + rows], B=B, T=T, n=n, img=img, patch=patch)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), host), "the packed buffer or its guards were written"
    got = big.cpu()
    assert bool((got[:8] == OUT_FILL).all()) and bool((got[8 + rows:] == OUT_FILL).all()), "rows outside the output were written"
    return got[8:8 + rows]


# ---------------------------------------------------------------------------------------------- the kernel
def test_ragged_gather_equals_the_reference_fixture(gpu, golden):
    """wide, tall and same as ONE ragged batch in one launch, 1-3 pad bytes between the clips"""
    f = golden("transform_resize")
    img, size, patch = int(f["image"]), int(f["size"]), 8
    clips = [torch.tensor(f["frames_" + t]) for t in TAGS]
    g = img // patch
    keep = torch.arange(g * g, dtype=torch.int32).unsqueeze(0).expand(3, -1).contiguous()
    crop = [int(v) for v in f["crop_yx"]]
    assert crop == [3, 5]
    for crops, key in ((None, "out_"), ([crop] * 3, "out_crop_")):
        rows = run_ragged(clips, [3, 3, 3], crops, keep, size=size, img=img, patch=patch, T=3, gaps=[1, 3, 3])
        ref = RR.im2col_rows(torch.stack([torch.tensor(f[key + t]) for t in TAGS]), keep, patch)  # the reference's outputs
        per = 3 * g * g
        for b, t in enumerate(TAGS):
            assert torch.equal(rows[b * per:(b + 1) * per].float(), ref[b * per:(b + 1) * per]), key + t


def _four_clips(size, T, seed):
    """landscape, portrait, one upscaled, one already at `size` (left alone by the Resize)"""
    g = torch.Generator().manual_seed(seed)
    shapes = [(size + 14, size + 45), (size + 54, size + 9), (size - 26, size - 16), (size, size + 24)]
    return [torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8) for h, w in shapes], g


def _crops(clips, size, img, g):
    """random crops; clip 0 at the top-left corner, clip 1 at the bottom-right one"""
    out = []
    for b, c in enumerate(clips):
        nh, nw = RR.resized_hw(int(c.shape[1]), int(c.shape[2]), size)
        out.append((0, 0) if b == 0 else (nh - img, nw - img) if b == 1 else
                   (int(torch.randint(0, nh - img + 1, (1,), generator=g)), int(torch.randint(0, nw - img + 1, (1,), generator=g))))
    return out


@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("patch,img,size", [(16, 64, 76), (14, 56, 67)])
def test_ragged_gather_equals_the_resized_gather_clip_by_clip(gpu, patch, img, size, T):
    from tvts_amd import hip as K
    from tvts_amd.data_loader.transforms import resize_tables
    clips, g = _four_clips(size, T, seed=patch + T)
    crops = _crops(clips, size, img, g)
    gsz, n = img // patch, 5
    keep = torch.stack([torch.randperm(gsz * gsz, generator=g)[:n] for _ in range(4)]).to(torch.int32)
    rows = run_ragged(clips, [T] * 4, crops, keep, size=size, img=img, patch=patch, T=T, gaps=[3, 1, 2, 1])
    Kc, ldo = 3 * patch * patch, rows.shape[1]
    assert (Kc, ldo) == ((768, 768) if patch == 16 else (588, 640))
    for b, c in enumerate(clips):
        one = torch.full((T * n, ldo), OUT_FILL, dtype=torch.bfloat16, device=DEV)
        K.patch_gather_u8(c.unsqueeze(0).to(DEV), keep[b:b + 1].to(DEV), one, B=1, T=T, n=n, img=img, patch=patch,
                          crop=torch.tensor([crops[b]], dtype=torch.int32, device=DEV),
                          resize=resize_tables(int(c.shape[1]), int(c.shape[2]), size, DEV))
        same_bits(rows[b * T * n:(b + 1) * T * n], one, f"clip {b}")
    assert not bits(rows[:, Kc:].contiguous()).any() if ldo > Kc else True  # columns K .. ldo: +0
    # and the values are the restatement's (the reference of the model tests below)
    ref = RR.im2col_rows(RR.restate(clips, crops, size, img, T), keep, patch)
    assert torch.equal(rows[:, :Kc].float(), ref)


def test_short_clips_are_followed_by_zero_rows(gpu):
    from tvts_amd.data_loader.v2_input import failed_clip
    patch, img, size, T, n = 16, 64, 76, 3, 5
    clips, g = _four_clips(size, T, seed=9)
    clips[3] = failed_clip(img).expand(T, -1, -1, -1).contiguous()  # the failed decode: one black img x img frame, upscaled by Resize
    frames = [T, T - 1, 1, 1]
    crops = _crops(clips, size, img, g)
    keep = torch.stack([torch.randperm(16, generator=g)[:n] for _ in range(4)]).to(torch.int32)
    kw = dict(size=size, img=img, patch=patch, T=T)
    full = run_ragged(clips, [T] * 4, crops, keep, gaps=[2, 3, 1, 1], **kw)
    short = run_ragged(clips, frames, crops, keep, gaps=[2, 3, 1, 1], **kw)
    for b, fr in enumerate(frames):
        lo = b * T * n
        same_bits(short[lo:lo + fr * n], full[lo:lo + fr * n], f"clip {b}: its own frames")
        tail = short[lo + fr * n:lo + T * n]
        assert tail.numel() == (T - fr) * n * short.shape[1] and not bits(tail.contiguous()).any(), f"clip {b}: zero frames"
    assert bits(full[3 * T * n:]).any() and float(full[3 * T * n:, :768].float().max()) < 0  # black behind Normalize is not zero


def test_entry_point_refusals(gpu):
    from tvts_amd import _lib
    lib = _lib.load()
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    src, desc, tables, keep, out = z(64), z(2, 8, dt=torch.int64), z(64, dt=torch.int32), z(2, 3, dt=torch.int32), z(12, 768, dt=torch.bfloat16)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda src=p(src), desc=p(desc), tables=p(tables), keep=p(keep), B=2, T=2, n=3, img=64, patch=16, mean=f3, std=f3, out=p(out), \
        ldo=768: lib.tvts_patch_gather_u8_ragged(src, desc, tables, keep, B, T, n, img, patch, mean, std, out, ldo, None)  # noqa: E731
    for kw in (dict(src=None), dict(desc=None), dict(tables=None), dict(keep=None), dict(out=None), dict(mean=None), dict(std=None),
               dict(B=0), dict(T=0), dict(n=0), dict(patch=0), dict(img=0), dict(B=-2), dict(img=-64), dict(img=72), dict(ldo=772),
               dict(ldo=760), dict(patch=14, img=56, ldo=584)):
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert not out.any()  # nothing was launched


# ---------------------------------------------------------------------------------------------- model, step, encoder
ARGS = types.SimpleNamespace(local_rank=0, rank=0, world_size=1)
SIZE = 76


@pytest.fixture(scope="module")
def ragged(gpu):
    """four decoder-sized clips for small_arch (image 64): lengths (2, 2, 1, 1), the last the failed-decode form; the batch with a
    random crop and with the centre crop, each beside the fp32 clips of the host restatement (computed once, read only)"""
    from tvts_amd import arch as A
    from tvts_amd.data_loader.v2_input import failed_clip
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    P = O.synth_params(oarch, seed=31)
    b = O.synth_batch(oarch, B=4, T=2, seed=44, caption_len=8)
    clips, g = _four_clips(SIZE, 2, seed=21)
    clips = [clips[1], clips[0], clips[2][:1], failed_clip(a["image"])]  # (both clips of the second half are short)
    crops = _crops(clips, SIZE, a["image"], g)
    crop_t = torch.tensor(crops)
    fp_crop, fp_centre = RR.restate(clips, crops, SIZE, a["image"], 2), RR.restate(clips, None, SIZE, a["image"], 2)
    assert not fp_crop[2:, 1].contiguous().view(torch.int32).any() and fp_crop[:2].abs().min() > 0
    return dict(a=a, oarch=oarch, P=P, clips=clips, crops=crops,
                u8_crop=dict(b, video=clips, crop=crop_t, resize=SIZE), u8_centre=dict(b, video=clips, resize=SIZE),
                fp_crop=dict(b, video=fp_crop), fp_centre=dict(b, video=fp_centre))


def _model(r):
    from tvts_amd.model._common import TVTSv2Base
    m = TVTSv2Base(ARGS, arch=r["a"])
    m.load_state_dict(r["P"], strict=True)
    return m


def test_forward_on_a_ragged_list_equals_forward_on_the_restated_clips(ragged):
    m = _model(ragged)
    outs = {}
    with torch.no_grad():
        for kind in ("crop", "centre"):
            te8, ve8, pr8 = m(ragged["u8_" + kind])
            te, ve, pr = m(ragged["fp_" + kind])
            assert torch.equal(te8, te) and torch.equal(ve8, ve) and torch.equal(pr8, pr), kind
            outs[kind] = ve8
    assert not torch.equal(outs["crop"], outs["centre"])
    pb = m.engine.prepare_batch(ragged["u8_crop"])
    assert pb["video"].dtype == torch.uint8 and pb["video"].dim() == 1 and pb["crop"] is None and pb["resize"] is None
    assert pb["gather"]["desc"].dtype == torch.int64 and tuple(pb["gather"]["desc"].shape) == (4, 8) and (pb["B"], pb["T"]) == (4, 2)
    assert pb["video"].numel() == sum(c.numel() for c in ragged["clips"]) and pb["gather"]["tables"].dtype == torch.int32
    assert "gather" not in m.engine.prepare_batch(ragged["fp_crop"])  # (the other wire formats prepare what they prepared)


def test_training_step_on_a_ragged_list_has_the_bits_of_the_fp32_step(ragged):
    a, P = ragged["a"], ragged["P"]
    m8, opt8, r8 = make(a, P)
    m, opt, r = make(a, P)
    for kind in ("crop", "centre"):
        o8, o = r8.step(ragged["u8_" + kind]), r.step(ragged["fp_" + kind])
        same_bits(o8["loss1"], o["loss1"], kind + ": loss1")
        same_bits(o8["loss2"], o["loss2"], kind + ": loss2")
        torch.cuda.synchronize()
        same_bits(m8.store.grad, m.store.grad, kind + ": the flat gradient")
        same_state(m8, snapshot(m), kind + ": after the update")
    assert opt8.global_step == opt.global_step == 2 and bool(m.store.grad.abs().sum() > 0)


def test_micro_batches_on_a_ragged_list(ragged):
    """n = 2 beside n = 1 on the same list at the gates of tests/test_micro_batch_gpu.py: gradient norm within 1e-2, worst tensor
    cosine above 0.995 (check_grads).  The second chunk holds short clips only: it agrees on T through num_frames."""
    a, P = ragged["a"], ragged["P"]
    m1, opt1, r1 = make(a, P)
    m2, opt2, r2 = make(a, P, micro_batches=2)
    o1, o2 = r1.step(ragged["u8_crop"]), r2.step(ragged["u8_crop"])
    torch.cuda.synchronize()
    names = [k for k in P if m1.engine.requires_grad[k]]
    ref = {k: m1.store.g(k).detach().cpu().clone() for k in names}
    d1, d2 = abs(float(o1["loss1"]) - float(o2["loss1"])), abs(float(o1["loss2"]) - float(o2["loss2"]))
    tot, tot_ref, worst = check_grads(m2.store, ref)
    print(f"\n   [ragged, n = 2 vs n = 1] |d loss1| {d1:.2e} |d loss2| {d2:.2e} (gate 1e-2); gradient norm {tot / tot_ref - 1:+.2e} "
          f"(gate 1e-2), worst tensor cosine {worst[0][0]:.5f} {worst[0][1]} (gate 0.995)")
    assert d1 < 1e-2 and d2 < 1e-2


def test_encode_video_on_lists_and_on_tensors_with_crop_and_resize(ragged):
    a = ragged["a"]
    m = _model(ragged)
    clips, crops = ragged["clips"], ragged["crops"]
    keep = torch.tensor([[0, 5, 3, 10, 15, 6]])
    for crop, fp in ((torch.tensor(crops), ragged["fp_crop"]["video"]), (None, ragged["fp_centre"]["video"])):
        want = m.encode_video(fp, keep)
        assert torch.equal(m.encode_video(clips, keep, crop=crop, resize=SIZE), want)
        assert torch.equal(m.encode_video(clips, keep, crop=crop, resize=SIZE, num_frames=2), want)
    # num_frames beyond the longest clip: one more zero frame per clip
    pad = torch.cat([ragged["fp_centre"]["video"], torch.zeros(4, 1, 3, a["image"], a["image"])], 1)
    assert torch.equal(m.encode_video(clips, keep, resize=SIZE, num_frames=3), m.encode_video(pad, keep))
    # a uniform tensor with crop / resize goes through the existing kernels
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (3, 2, 90, 121, 3), generator=g, dtype=torch.uint8)
    nh, nw = RR.resized_hw(90, 121, SIZE)
    ucrop = torch.tensor([[0, 0], [nh - a["image"], nw - a["image"]], [5, 17]])
    for size, crop in ((SIZE, ucrop), (SIZE, None), (None, ucrop)):
        want = m.encode_video(RR.restate(list(frames), None if crop is None else crop.tolist(), size, a["image"], 2), keep)
        assert torch.equal(m.encode_video(frames, keep, crop=crop, resize=size), want), (size, crop)
    assert torch.equal(m.encode_video(frames, keep), m.encode_video(RR.restate(list(frames), None, None, a["image"], 2), keep))
    with pytest.raises(ValueError, match="crop outside"):
        m.encode_video(frames, keep, crop=ucrop + torch.tensor([[0, 0], [1, 0], [0, 0]]), resize=SIZE)
    with pytest.raises(ValueError, match="below the crop"):
        m.encode_video(frames, keep, resize=60)
    with pytest.raises(ValueError, match="more than"):
        m.encode_video(clips, keep, resize=SIZE, num_frames=1)


def test_graph_replay_steps_ragged_batches_eagerly(ragged, monkeypatch):
    from tvts_amd.step import GraphReplay
    monkeypatch.setenv("TVTS_TRAINER_GRAPH", "1")
    a, P = ragged["a"], ragged["P"]
    m, opt, r = make(a, P)
    me, opte, re_ = make(a, P)
    rep = GraphReplay(r)
    if not rep.usable:
        pytest.skip("graph capture is not usable in this run")
    for kind in ("crop", "centre", "crop"):
        o, oe = rep.step(ragged["u8_" + kind]), re_.step(ragged["u8_" + kind], device_step=True)
        same_bits(o["loss1"], oe["loss1"], "loss1")
        same_bits(o["loss2"], oe["loss2"], "loss2")
    assert rep.eager == 3 and rep.captures == 0 and rep.replays == 0
    same_state(m, snapshot(me), "GraphReplay over ragged batches against the runner")
    assert opt.global_step == 3
