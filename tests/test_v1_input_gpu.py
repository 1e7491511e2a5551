"""The v1 pretraining step's uint8 input on the device (run with -m gpu): tvts_resize_crop_u8 against the bytes the reference's own
Resize + crop left in tests/golden/v1_input.npz, the im2col rows behind it against the fp32 gather on the fixture's fp32 clips, the
whole step in every wire format against the fp32-fed step bit for bit, the device-drawn tube masks, and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
from oracle import tvts_v1_oracle as V  # noqa: E402  (synthetic weights and captions only)
from test_v1_gpu import build, engine_step  # noqa: E402
from tvts_amd import arch as A  # noqa: E402
from tvts_amd.data_loader import transforms as TR  # noqa: E402
from tvts_amd.data_loader.v1_input import collate_u8  # noqa: E402
from v1_input_ref import resample_u8  # noqa: E402

DEV = "cuda:0"
IMG, SIZE, T = 32, 38, 4


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


@pytest.fixture(scope="module")
def fx(golden):
    f = golden("v1_input")
    assert int(f["crop_size"]) == IMG and int(f["resize"]) == SIZE and int(f["T"]) == T
    n = int(f["n"])
    d = dict(src=[torch.from_numpy(f[f"src.{i}"]) for i in range(n)], crop=[tuple(int(v) for v in f[f"crop.{i}"]) for i in range(n)],
             u8=torch.from_numpy(np.stack([f[f"u8.{i}"] for i in range(n)])), f32=torch.from_numpy(np.stack([f[f"f32.{i}"] for i in range(n)])))
    d["new"] = [TR.resize_sizes(int(s.shape[1]), int(s.shape[2]), SIZE) for s in d["src"]]
    return d


_RESIZED = {}


def resized(fx, b):
    """the whole resized clip b by the numpy restatement (tests/test_v1_input_cpu.py holds it to Pillow and to the fixture), once"""
    if b not in _RESIZED:
        _RESIZED[b] = torch.from_numpy(resample_u8(fx["src"][b].numpy(), *fx["new"][b]))
    return _RESIZED[b]


def run_kernel(K, clips, crops, frames):
    """one launch over the ragged batch, byte offsets 1, 2, 3 (mod 4) past the previous clip; output and tmp guarded -> uint8 [B, T, 32, 32, 3]"""
    B = len(clips)
    offsets, at = [], 0
    for b, c in enumerate(clips):
        at += 1 + b % 3
        if at % 4 == 0:
            at += 1
        offsets.append(at)
        at += frames * c.shape[1] * c.shape[2] * 3
    assert all(o % 4 for o in offsets)
    plan = K.resize_plan([(c.shape[1], c.shape[2]) for c in clips], crops, size=SIZE, img=IMG, T=frames, offsets=offsets)
    src = torch.full((plan["nbytes"] + 16,), 0xAB, dtype=torch.uint8)
    for c, o in zip(clips, offsets):
        src[o:o + frames * c[0].numel()] = c[:frames].reshape(-1)
    n_tmp = B * frames * plan["tmp_rows"] * IMG * 3
    tmp = torch.full((n_tmp + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    buf, out = KB.guarded(B * frames * IMG, 3 * IMG, torch.uint8, DEV)
    K.resize_crop_u8(src.to(DEV), torch.from_numpy(plan["desc"]).to(DEV), torch.from_numpy(plan["tables"]).to(DEV), tmp[:n_tmp], out,
                     B=B, T=frames, img=IMG, tmp_rows=plan["tmp_rows"])
    torch.cuda.synchronize()
    KB.check_guards(buf, B * frames * IMG, 3 * IMG, "resize_crop_u8")
    assert bool((tmp[n_tmp:] == 0xFF).all()), "bytes past tmp were written"
    return out.cpu().reshape(B, frames, IMG, IMG, 3)


@pytest.mark.parametrize("case", ["fixture", "origin", "far corner", "two frames"])
def test_kernel_against_the_fixture(K, fx, case):
    B = len(fx["src"])
    if case in ("fixture", "two frames"):
        crops, want = fx["crop"], fx["u8"]
    else:
        crops = [(0, 0)] * B if case == "origin" else [(nh - IMG, nw - IMG) for nh, nw in fx["new"]]
        want = torch.stack([resized(fx, b)[:, t:t + IMG, l:l + IMG] for b, (t, l) in enumerate(crops)])
    frames = 2 if case == "two frames" else T
    got = run_kernel(K, fx["src"], crops, frames)
    KB.assert_equal_bits(got.reshape(B * frames * IMG, -1), want[:, :frames].reshape(B * frames * IMG, -1).contiguous(), f"resize + crop ({case})")
    if case == "far corner":  # the last source pixel and the last tap are read: the last output of either axis ends at n_in
        for (hs, ws), (nh, nw) in zip([(s.shape[1], s.shape[2]) for s in fx["src"]], fx["new"]):
            for n_in, n_out in ((hs, nh), (ws, nw)):
                first, k = TR.pil_bilinear_coeffs(n_in, n_out)[-1]
                assert first + len(k) == n_in


@pytest.mark.parametrize("keep_kind", ["full", "shuffled partial"])
def test_im2col_bytes_equal_the_fp32_gather(K, fx, keep_kind):
    """kernel + patch_gather_tube_u8 == patch_gather_tube on the fixture's fp32 clip, byte for byte"""
    B, p, tb = len(fx["src"]), 16, 2
    tubes, ppf = T // tb, (IMG // p) ** 2
    n = ppf if keep_kind == "full" else ppf - 1
    g = torch.Generator().manual_seed(41)
    keep = torch.stack([torch.stack([torch.randperm(ppf, generator=g)[:n] if n < ppf else torch.arange(ppf) for _ in range(tubes)])
                        for _ in range(B)]).to(torch.int32).to(DEV)
    frames = run_kernel(K, fx["src"], fx["crop"], T).to(DEV)
    Kc, M = 3 * tb * p * p, B * tubes * n
    kw = dict(B=B, tubes=tubes, tubelet=tb, n=n, img=IMG, patch=p)
    buf_a, a = KB.guarded(M, Kc, torch.bfloat16, DEV)
    buf_b, b = KB.guarded(M, Kc, torch.bfloat16, DEV)
    K.patch_gather_tube_u8(frames, keep, a, **kw)
    K.patch_gather_tube(fx["f32"].to(DEV), keep, b, **kw)
    torch.cuda.synchronize()
    KB.check_guards(buf_a, M, Kc, "tube_u8")
    KB.assert_equal_bits(a.contiguous(), b.contiguous(), f"im2col rows ({keep_kind} keep)")


# ------------------------------------------------------------------------------------------------ the step
def archs(**over):
    a = A.small_arch_v1(image=IMG, **over)
    return a, V.tiny_arch(**{k: a[k] for k in V.tiny_arch() if k in a and k != "name"})


def step_bits(m, batch, seed0, training):
    m.engine.drop_seed.copy_(seed0)
    m.engine.training = training
    l1, l2, te, ve, pred = engine_step(m, batch)
    return dict(l1=l1, l2=l2, te=te, ve=ve, pred=pred.clone(), grad=m.store.grad.clone())


def same_bits(got, want, what):
    assert got["l1"] == want["l1"] and got["l2"] == want["l2"], (what, got["l1"], want["l1"], got["l2"], want["l2"])
    for k in ("te", "ve", "pred"):
        KB.assert_equal_bits(got[k].reshape(got[k].shape[0], -1), want[k].reshape(want[k].shape[0], -1), f"{what}: {k}")
    assert torch.equal(got["grad"].view(torch.int32), want["grad"].view(torch.int32)), f"{what}: the whole flat gradient"
    assert float(want["grad"].abs().max()) > 0.0


def wire_formats(fx):
    """{name: the video keys of the batch dict} for the fixture's five clips -- every format must give the fp32 step on fx['f32']"""
    canvas = torch.randint(0, 256, (5, T, 69, 71, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    for b, (t, l) in enumerate(fx["crop"]):
        canvas[b, :, t:t + IMG, l:l + IMG] = fx["u8"][b]
    crop = torch.tensor(fx["crop"], dtype=torch.int64)
    return {"pre-cropped": dict(video=fx["u8"].clone()),
            "resized + crop": dict(video=canvas, crop=crop),
            "source list + resize": dict(video=[s.clone() for s in fx["src"]], crop=crop, resize=SIZE)}


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train + dropout"])
def test_step_bits_in_every_wire_format(K, fx, training):
    a, oa = archs()
    P = V.synth_params(oa, seed=5)
    base = V.synth_batch(oa, B=5, T=T, seed=6, n_trans=4, caption_len=13)
    m = build(a, P, dropout=0.1)
    m.train(training)
    seed0 = m.engine.drop_seed.clone()
    want = step_bits(m, dict(base, video=fx["f32"].clone()), seed0, training)
    for name, vid in wire_formats(fx).items():
        data = {k: v for k, v in base.items() if k != "video"}
        data.update(vid)
        same_bits(step_bits(m, data, seed0, training), want, name)
    # one tensor [B, T, Hs, Ws, 3] at source size: clip 0 with its frames rolled (B = 4 clips of one size, one crop)
    rolls = dict(video=torch.stack([fx["src"][0].roll(b, 0) for b in range(4)]), crop=torch.tensor([fx["crop"][0]] * 4), resize=SIZE)
    base4 = V.synth_batch(oa, B=4, T=T, seed=7, n_trans=4, caption_len=13)
    want4 = step_bits(m, dict(base4, video=torch.stack([fx["f32"][0].roll(b, 0) for b in range(4)])), seed0, training)
    same_bits(step_bits(m, dict(base4, **rolls), seed0, training), want4, "source tensor + resize")
    # the module's forward hands the dict through untouched
    if not training:
        with torch.no_grad():
            m.engine.drop_seed.copy_(seed0)
            te, ve, pred = m(dict(base, video=fx["f32"].clone()))
            m.engine.drop_seed.copy_(seed0)
            data = {k: v for k, v in base.items() if k != "video"}
            te2, ve2, pred2 = m(dict(data, **collate_u8([dict(video=s, crop=c, resize=SIZE) for s, c in zip(fx["src"], fx["crop"])])))
        for x, y in ((te, te2), (ve, ve2), (pred, pred2)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_step_bits_with_text_unpadded(K, fx):
    a, oa = archs()
    P = V.synth_params(oa, seed=5)
    base = V.synth_batch(oa, B=5, T=T, seed=6, n_trans=4, caption_len=13)
    m = build(dict(a, text_unpadded=True), P, dropout=0.1)
    assert m.engine.text_unpadded
    seed0 = m.engine.drop_seed.clone()
    want = step_bits(m, dict(base, video=fx["f32"].clone()), seed0, True)
    for name in ("resized + crop", "source list + resize"):
        data = {k: v for k, v in base.items() if k != "video"}
        data.update(wire_formats(fx)[name])
        same_bits(step_bits(m, data, seed0, True), want, name + " (text_unpadded)")


# ------------------------------------------------------------------------------------------------ device-drawn tube masks
def test_mask_seed_rows(K, fx):
    a, oa = archs(num_frames=16)
    n_temp, ppf, nk = 8, 4, 2
    assert a["num_frames"] // a["tubelet"] == n_temp and A.patches_per_frame(a) == ppf and A.n_keep(a) == nk
    m = build(a, V.synth_params(oa, seed=5))
    text = V.synth_batch(oa, B=4, T=T, seed=6, n_trans=4, caption_len=9)["text"]
    seed, off = 0x1234567, 11
    clip8 = torch.randint(0, 256, (4, 16, IMG, IMG, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    whole = m.engine.prepare_batch(dict(text=text, video=clip8, mask_seed=seed, sample_offset=off))["keep"]
    rows = K.tube_mask(seed, off * n_temp, 4 * n_temp, ppf, nk, device=DEV).view(4, n_temp, nk)
    assert whole.dtype == torch.int32 and tuple(whole.shape) == (4, n_temp, nk) and torch.equal(whole, rows)
    w = whole.cpu()
    assert int(w.min()) >= 0 and int(w.max()) < ppf and all(len(set(r.tolist())) == nk for r in w.reshape(-1, nk))
    assert len({tuple(r.tolist()) for r in w.reshape(-1, nk)}) > 1
    # two half batches with sample_offset give the rows of the whole batch
    half_text = lambda lo: {k: v.reshape(4, 4, -1)[:, lo:lo + 2].reshape(8, -1) for k, v in text.items()}  # noqa: E731
    halves = [m.engine.prepare_batch(dict(text=half_text(lo), video=clip8[lo:lo + 2], mask_seed=seed, sample_offset=off + lo))["keep"]
              for lo in (0, 2)]
    assert torch.equal(torch.cat(halves), whole)
    # a 2-tube clip gets the first two rows of its 8
    short = m.engine.prepare_batch(dict(text=text, video=clip8[:, :4].contiguous(), mask_seed=seed, sample_offset=off))["keep"]
    assert tuple(short.shape) == (4, 2, nk) and short.is_contiguous() and torch.equal(short, whole[:, :2])
    # no sample_offset: clip 0 of the batch is global clip 0
    assert torch.equal(m.engine.prepare_batch(dict(text=text, video=clip8, mask_seed=seed))["keep"],
                       K.tube_mask(seed, 0, 4 * n_temp, ppf, nk, device=DEV).view(4, n_temp, nk))


def test_refusals(K, fx):
    a, oa = archs()
    m = build(a, V.synth_params(oa, seed=5))
    base = {k: v for k, v in V.synth_batch(oa, B=2, T=T, seed=6, n_trans=4, caption_len=9).items() if k != "video"}
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    for video, extra, msg in (
            ([u8(4, 45, 80, 3), u8(2, 45, 80, 3)], dict(resize=SIZE), "frames"),
            (u8(2, 4, 45, 80, 3), dict(resize=30), "below the crop"),
            (u8(2, 4, 31, 80, 3), {}, "below the crop"),
            (u8(2, 4, 45, 80, 3), dict(resize=SIZE, crop=torch.tensor([[0, 0], [7, 0]])), "crop outside"),
            (u8(2, 4, 38, 67, 3), dict(crop=torch.tensor([[0, 36], [0, 0]])), "crop outside"),
            (u8(2, 4, 3, 38, 67), {}, r"\[B, T, H, W, 3\]")):
        with pytest.raises(ValueError, match=msg):
            m.engine.prepare_batch(dict(base, video=video, **extra))
    nokeep = {k: v for k, v in base.items() if k != "keep_ind"}
    with pytest.raises(KeyError, match="mask_seed"):
        m.engine.prepare_batch(dict(nokeep, video=u8(2, 4, 32, 32, 3)))
    with pytest.raises(KeyError, match="mask_seed"):
        m.engine.prepare_batch(dict(nokeep, video=torch.zeros(2, 4, 3, 32, 32)))
    # a temporary buffer below the size rule is refused by the entry point (the other -22 cases: tests/test_v1_input_cpu.py)
    plan = K.resize_plan([(45, 80)], [(4, 17)], size=SIZE, img=IMG, T=2)
    with pytest.raises(K.HipError, match="-22"):
        K.resize_crop_u8(torch.zeros(plan["nbytes"], dtype=torch.uint8, device=DEV), torch.from_numpy(plan["desc"]).to(DEV),
                         torch.from_numpy(plan["tables"]).to(DEV), torch.zeros(2 * plan["tmp_rows"] * IMG * 3 - 1, dtype=torch.uint8, device=DEV),
                         torch.zeros(1, 2, IMG, IMG, 3, dtype=torch.uint8, device=DEV), B=1, T=2, img=IMG, tmp_rows=plan["tmp_rows"])
