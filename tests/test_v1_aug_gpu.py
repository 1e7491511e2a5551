"""Random-resized crop, flip and random erasing fused into the uint8 tubelet gather of the v1 fine-tuning step (run with -m gpu).

The expected values come from tests/v1_aug_ref.py (taps in fp32 as torch forms them, everything behind them in float64; the
restatement is pinned to the reference's own run by tests/test_v1_aug_cpu.py).  Per-element gate of every kernel test: with e the
float64 value and d the fp32 allowance of the element, bf16(e - d) <= out <= bf16(e + d) -- bf16 rounding is monotonic, so this
admits one value almost everywhere; no relative tolerance is put on a bf16 result.  d = 2e-6 for an unmixed picture element (values
up to 2.64, fp32 ulp 2.4e-7, three roundings in the normalisation -- the first two amplified by 1 / std <= 4.5 -- and seven in the
blend), 2e-5 for a noise element (logf / cosf at a few ulp under sqrt(-2 ln u) <= 6.66, and the fp32 rounding of u1, u2 and 2 pi),
and for a mode-1 mix lam * d_own + (1 - lam) * d_partner + 1e-6 (two products and a sum more: 3e-6 on picture elements).
Identity crops, erase-free elements of an erased sample, mode-0 mixes and repeated launches are compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import v1_aug_ref as A  # noqa: E402
import v1_downstream_synth as S  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
EINVAL = -22
IMG, PATCH, TB, T = 32, 8, 2, 4
H0, W0, BS, NS = 37, 53, 2, 2
B = BS * NS
TUBES, PPF, KC = T // TB, (IMG // PATCH) ** 2, 3 * TB * PATCH * PATCH
D_PIC, D_NOISE, D_MIX = 2e-6, 2e-5, 1e-6
NAN_BITS = 0x7FC1  # a NaN pattern no kernel produces: what the outputs are pre-filled with


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


@pytest.fixture(scope="module")
def frames():
    """the seeded uint8 source frames [BS, T, H0, W0, 3], made once and never written"""
    f = A.case_frames(4242, BS, H0, W0, frames=T)
    f.setflags(write=False)
    return f


# ---------------------------------------------------------------------------------------------- helpers
def row(src, crop, flip=0, emode=0, box=(0, 0, 0, 0), key=0):
    key &= (1 << 64) - 1
    lo, hi = np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint32).view(np.int32)
    return [src, *crop, flip, emode, *box, int(lo), int(hi), 0, 0, 0]


def full_keep(b=B, tubes=TUBES, ppf=PPF):
    return torch.arange(ppf, dtype=torch.int32).repeat(b, tubes, 1).contiguous()


def launch(K, frames, aug_i, keep=None, mix=None, img=IMG, patch=PATCH, tb=TB, pad=0, check=True):
    """one launch of the new gather -> (out view [B * tubes * n, Kc] bf16 on the device, its NaN-pre-filled buffer)"""
    fr = torch.from_numpy(np.array(frames)).to(DEV)
    aug_i = np.asarray(aug_i, dtype=np.int64)
    b, tubes = len(aug_i), fr.shape[1] // tb
    keep = full_keep(b, tubes, (img // patch) ** 2) if keep is None else keep
    n, kc = keep.shape[2], 3 * tb * patch * patch
    buf = torch.full((b * tubes * n + 2, kc + pad), NAN_BITS, dtype=torch.int16, device=DEV).view(BF16)
    out = buf[:b * tubes * n, :kc]
    if check:
        table = K.aug_table(aug_i, Bs=fr.shape[0], H0=fr.shape[2], W0=fr.shape[3], img=img, device=DEV)
    else:
        table = torch.from_numpy(aug_i.astype(np.int32)).to(DEV)
    mt = None if mix is None else K.mix_table(mix[0], mix[1], B=b, img=img, device=DEV)
    K.patch_gather_tube_u8_aug(fr, keep.to(DEV), out, table, mt, B=b, tubes=tubes, tubelet=tb, n=n, img=img, patch=patch)
    torch.cuda.synchronize()
    g = buf.view(torch.int16)
    assert (g[b * tubes * n:] == NAN_BITS).all() and (g[:, kc:] == NAN_BITS).all(), "the kernel wrote outside its rows"
    return out, buf


def fold(out, keep, img=IMG, patch=PATCH, tb=TB):
    """bf16 rows [B * tubes * n, 3 * tb * patch^2] -> float64 clip [B, 3, T, img, img] on the host, NaN where no kept patch landed"""
    b, tubes, n = keep.shape
    o = out.detach().to(torch.float64).cpu().numpy().reshape(b, tubes, n, 3, tb, patch, patch)
    clip = np.full((b, 3, tubes * tb, img, img), np.nan)
    g = img // patch
    for bi in range(b):
        for tu in range(tubes):
            for i in range(n):
                gy, gx = divmod(int(keep[bi, tu, i]), g)
                clip[bi, :, tu * tb:(tu + 1) * tb, gy * patch:(gy + 1) * patch, gx * patch:(gx + 1) * patch] = o[bi, tu, i]
    return clip


def bits(out):
    return out.detach().contiguous().view(torch.int16).cpu()


def to_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), as float64: ONE rounding, taken from the double itself"""
    x = np.asarray(x, dtype=np.float64)
    mag = np.abs(x)
    down = (mag.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).astype(np.int64)
    best = None
    for step in (-1, 0, 1, 2):
        cb = np.maximum(down + step * 0x10000, 0).astype(np.uint32)
        cv = cb.view(np.float32).astype(np.float64)
        err = np.abs(cv - mag)
        if best is None:
            best, best_err, best_b = cv, err, cb
        else:
            take = (err < best_err) | ((err == best_err) & ((cb >> np.uint32(16)) & np.uint32(1) == 0) & (cb != best_b))
            best, best_err, best_b = np.where(take, cv, best), np.where(take, err, best_err), np.where(take, cb, best_b)
    return np.copysign(best, x)


def gate(got, e, d, what, where=None):
    """bf16(e - d) <= got <= bf16(e + d) at every element of `where` (default: everywhere; an unwritten element is NaN and fails)"""
    where = np.ones(got.shape, dtype=bool) if where is None else where
    lo, hi = to_bf16(e - d), to_bf16(e + d)
    bad = where & ~((got >= lo) & (got <= hi))
    one = where & (lo == hi)
    print(f"{what}: {int(where.sum())} elements compared, {int(one.sum())} of them with a single admitted value")
    assert where.any() and not np.isnan(got[where]).any(), what
    if bad.any():
        idx = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(where.sum())} outside the gate, first at {idx}: got {got[idx]!r}, "
                             f"e {e[idx]!r}, admitted [{lo[idx]!r}, {hi[idx]!r}]")


def expected(frames, aug_i, img=IMG):
    """-> (e float64 [B, 3, T, img, img], d the allowance per element, box masks [B, img, img])"""
    aug_i = np.asarray(aug_i)
    e = A.aug_clip(frames, aug_i, img=img)
    masks = np.stack([A.box_mask(r, img) for r in aug_i])
    noisy = masks & (aug_i[:, 6] >= 2)[:, None, None]
    d = np.where(noisy[:, None, None], D_NOISE, D_PIC) * np.ones_like(e)
    return e, d, masks


def mixed(e, d, mix_i, mix_f):
    """the mix table over float64 clips and their allowances (mode 1 with the fp32 lam / 1 - lam the kernel is handed)"""
    oe, od = e.copy(), d.copy()
    for b, (partner, mode, yl, yh, xl, xh) in enumerate(np.asarray(mix_i).tolist()):
        lam, oml = float(np.float32(mix_f[b][0])), float(np.float32(mix_f[b][1]))
        if mode == 1:
            oe[b], od[b] = e[b] * lam + e[partner] * oml, d[b] * lam + d[partner] * oml + D_MIX
        elif mode == 2:
            oe[b][..., yl:yh, xl:xh], od[b][..., yl:yh, xl:xh] = e[partner][..., yl:yh, xl:xh], d[partner][..., yl:yh, xl:xh]
        elif mode == 3:
            oe[b][:, yl:yh, xl:xh, :], od[b][:, yl:yh, xl:xh, :] = e[partner][:, yl:yh, xl:xh, :], d[partner][:, yl:yh, xl:xh, :]
    return oe, od


# ================================================================================================ 1. identity crop
def test_identity_crop_is_the_plain_u8_gather(K, frames):
    """h == w == img, no flip, no erase: the bits of tvts_patch_gather_tube_u8 with crop = (top, left), at the frame's corners (the
    far one reads the last pixel of the frame) and in between; the two views of a clip take different crops"""
    crops = [(0, 0), (H0 - IMG, W0 - IMG), (3, 7), (H0 - IMG, 0)]
    aug_i = [row(b // NS, (*crops[b], IMG, IMG), key=99 + b) for b in range(B)]
    out, _ = launch(K, frames, aug_i)
    plain = torch.full((B * TUBES * PPF, KC), NAN_BITS, dtype=torch.int16, device=DEV).view(BF16)
    fr_b = torch.from_numpy(np.array(frames[[r[0] for r in aug_i]])).to(DEV)
    K.patch_gather_tube_u8(fr_b, full_keep().to(DEV), plain, B=B, tubes=TUBES, tubelet=TB, n=PPF, img=IMG, patch=PATCH,
                           crop=torch.tensor(crops, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    print(f"identity crop: {out.numel()} elements compared bit for bit")
    assert torch.equal(bits(out), bits(plain))


# ================================================================================================ 2. resize and flip
# name -> (source frame size, crop of the first view, crop of the second view); crops are (top, left, h, w)
RESIZE = {
    "upscale_9x11": ((H0, W0), (5, 7, 9, 11), (20, 30, 11, 9)),
    "downscale_whole_frame": ((H0, W0), (0, 0, H0, W0), (1, 2, 36, 50)),
    "one_row_one_column": ((H0, W0), (36, 0, 1, W0), (0, 52, H0, 1)),
    "one_pixel": ((H0, W0), (17, 23, 1, 1), (H0 - 1, W0 - 1, 1, 1)),
    "source_smaller_than_img": ((20, 24), (0, 0, 20, 24), (3, 2, 15, 20)),
    "interior_far_edge": ((H0, W0), (6, 9, 20, 30), (2, 3, 33, 40)),       # a clamp to the FRAME's edge would read differing pixels
    "ends_at_the_last_pixel": ((H0, W0), (H0 - 7, W0 - 13, 7, 13), (H0 - 33, W0 - 47, 33, 47)),
}


@pytest.mark.parametrize("name", list(RESIZE))
def test_resize_and_flip(K, frames, name):
    """every sample against the float64 restatement; view k of clip s takes crop k, once unflipped and once flipped across the two
    clips (so the two samples of one source differ in crop and flip), and the last clip's views end at its last pixel"""
    (h0, w0), c1, c2 = RESIZE[name]
    fr = frames if (h0, w0) == (H0, W0) else A.case_frames(77, BS, h0, w0, frames=T)
    aug_i = [row(0, c1, 0), row(0, c2, 1), row(1, c1, 1), row(1, c2, 0)]
    out, _ = launch(K, fr, aug_i)
    e, d, _ = expected(fr, aug_i)
    gate(fold(out, full_keep()), e, d, name)
    if name == "interior_far_edge":   # the pixels just outside the far edge differ from the edge's own (else the case shows nothing)
        t, l, h, w = c1
        assert (fr[:, :, t + h, l:l + w] != fr[:, :, t + h - 1, l:l + w]).any() and (fr[:, :, t:t + h, l + w] != fr[:, :, t:t + h, l + w - 1]).any()


# ================================================================================================ 3. keep, ldo, unwritten rows
ERASED = [row(0, (5, 7, 9, 11), 0, 3, (3, 3, 18, 10), key=1 << 40), row(0, (0, 0, H0, W0), 1, 2, (5, 6, 17, 9), key=12345),
          row(1, (6, 9, 20, 30), 1, 3, (8, 16, 8, 8), key=0xDEADBEEFCAFE), row(1, (2, 3, 33, 40), 0, 1, (1, 13, 30, 1), key=7)]


def test_keep_permutation_moves_patches_not_values(K, frames):
    """n = 11 of the 16 patches per (sample, tube) in a seeded order: every kept patch holds the bits it has under the full keep
    list -- noise included: a pixel's noise follows its output coordinate, not the row or thread that holds it"""
    g = torch.Generator().manual_seed(5)
    keep = torch.stack([torch.randperm(PPF, generator=g)[:11] for _ in range(B * TUBES)]).to(torch.int32).view(B, TUBES, 11).contiguous()
    part, _ = launch(K, frames, ERASED, keep=keep)
    whole, _ = launch(K, frames, ERASED)
    a, b = fold(part, keep), fold(whole, full_keep())
    kept = ~np.isnan(a)
    assert kept.sum() == B * TUBES * 11 * KC and np.array_equal(a[kept], b[kept])
    e, d, _ = expected(frames, ERASED)
    gate(a, e, d, "keep permutation, n = 11", where=kept)


def test_wide_ldo_and_a_sample_without_a_source(K, frames):
    """ldo = K + 24 over an output pre-filled with a NaN pattern: the columns beyond K keep their bits (checked in launch), and so
    do all rows of a sample whose src is Bs -- the table is device data, the kernel leaves such a sample alone and reads nothing"""
    aug_i = [list(r) for r in ERASED]
    aug_i[2][0] = BS
    out, buf = launch(K, frames, aug_i, pad=24, check=False)
    rows = TUBES * PPF
    raw = bits(out)
    assert (raw[2 * rows:3 * rows] == NAN_BITS).all() and not (raw[:2 * rows] == NAN_BITS).any() and not (raw[3 * rows:] == NAN_BITS).any()
    ok, _ = launch(K, frames, ERASED, pad=24)
    keepers = [r for r in range(B * rows) if not 2 * rows <= r < 3 * rows]
    assert torch.equal(raw[keepers], bits(ok)[keepers])
    # under a mix, a sample whose PARTNER has no source is left alone too
    mi = np.array([[1, 1, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [3, 1, 0, 0, 0, 0], [2, 1, 0, 0, 0, 0]], dtype=np.int32)
    mf = np.full((B, 2), 0.5, dtype=np.float32)
    out, _ = launch(K, frames, aug_i, mix=(mi, mf), check=False)
    raw = bits(out)
    assert (raw[2 * rows:] == NAN_BITS).all() and not (raw[:2 * rows] == NAN_BITS).any()


# ================================================================================================ 4. erase
# boxes (etop, eleft, eh, ew): cut inside an 8-pixel group on both sides; spanning patch borders in y and x; one pixel wide;
# exactly one patch
BOXES = [(2, 3, 5, 10), (5, 6, 17, 13), (1, 13, 30, 1), (8, 16, 8, 8)]
CROPS = [(5, 7, 9, 11), (0, 0, H0, W0), (6, 9, 20, 30), (2, 3, IMG, IMG)]


@pytest.mark.parametrize("emode", [1, 2, 3])
def test_erase_modes(K, frames, emode):
    aug_i = [row(b // NS, CROPS[b], b % 2, emode, BOXES[b], key=0xABCDEF0123 * (b + 1)) for b in range(B)]
    clean = [row(b // NS, CROPS[b], b % 2) for b in range(B)]
    out, _ = launch(K, frames, aug_i)
    again, _ = launch(K, frames, aug_i)
    assert torch.equal(bits(out), bits(again))                          # two launches: the same bits
    got, base = fold(out, full_keep()), fold(launch(K, frames, clean)[0], full_keep())
    e, d, masks = expected(frames, aug_i)
    inside = np.broadcast_to(masks[:, None, None], got.shape)
    assert inside.sum() == 3 * T * sum(b[2] * b[3] for b in BOXES)
    assert np.array_equal(got[~inside], base[~inside])                  # outside the box: the unerased value, bit for bit
    gate(got, e, d, f"erase mode {emode}, inside the boxes", where=inside)
    if emode == 1:
        assert not got[inside].any() and not np.signbit(got[inside]).any()
    else:
        assert (got[inside] != base[inside]).mean() > 0.99
    if emode == 2:   # one value per (frame, channel)
        for b in range(B):
            v = got[b][:, :, masks[b]]
            assert (v == v[..., :1]).all() and len(np.unique(v[..., 0])) > 1


# ================================================================================================ 5. mix
MIX_BOX = {1: (0, 0, 0, 0), 2: (3, 27, 5, 22), 3: (1, 3, 6, 25)}   # mode 3: the frames [1, 3), the rows [6, 25)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_mix_takes_the_partner_through_its_own_row(K, frames, mode):
    """partners 1, 2, 3, 0: sample 0's partner shares its source clip, the others differ in source, and all differ in crop, flip
    and erase (ERASED); sample 3 stays unmixed (mode 0) with cells that would show"""
    mi = np.array([[1, mode, *MIX_BOX[mode]], [2, mode, *MIX_BOX[mode]], [3, mode, *MIX_BOX[mode]], [0, 0, 0, IMG, 0, IMG]], dtype=np.int32)
    mf = np.array([[0.3, 0.7], [0.625, 0.375], [0.9, 0.1], [0.5, 0.5]], dtype=np.float32)
    out, _ = launch(K, frames, ERASED, mix=(mi, mf))
    e, d, _ = expected(frames, ERASED)
    me, md = mixed(e, d, mi, mf)
    got = fold(out, full_keep())
    gate(got, me, md, f"mix mode {mode}")
    alone = fold(launch(K, frames, ERASED)[0], full_keep())
    assert np.array_equal(got[3], alone[3]) and not np.array_equal(got[0], alone[0])
    if mode >= 2:    # a select: every element is the own or the partner's unmixed value, bit for bit
        for b in range(3):
            assert ((got[b] == alone[b]) | (got[b] == alone[mi[b, 0]])).all()


def test_mix_mode_zero_is_the_launch_without_a_table(K, frames):
    mi = np.array([[1, 0, 2, 9, 3, 11], [0, 0, 0, IMG, 0, IMG], [3, 0, 0, 0, 0, 0], [2, 0, 5, 6, 7, 8]], dtype=np.int32)
    mf = np.array([[0.5, 0.5], [0.0, 1.0], [1.0, 0.0], [0.25, 0.75]], dtype=np.float32)
    a, _ = launch(K, frames, ERASED, mix=(mi, mf))
    b, _ = launch(K, frames, ERASED)
    print(f"mix mode 0: {a.numel()} elements compared bit for bit")
    assert torch.equal(bits(a), bits(b))


# ================================================================================================ 6. refusals
def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def test_einval_for_each_refused_argument(K, frames):
    """null pointers, exactly one of the two mix pointers, non-positive sizes, the shape / ldo / alignment conditions: TVTS_EINVAL
    and nothing launched (the output keeps its fill); H0, W0 below img are NOT refused"""
    lib = K._lib.load()
    fr = torch.from_numpy(np.array(frames)).to(DEV)
    keep = full_keep().to(DEV)
    aug = K.aug_table(np.array(ERASED), Bs=BS, H0=H0, W0=W0, img=IMG, device=DEV)
    mi, mf = K.mix_table(np.array([[1, 1, 0, 0, 0, 0]] * B), np.array([[0.5, 0.5]] * B), B=B, img=IMG, device=DEV)
    out = torch.full((B * TUBES * PPF + 2, KC + 8), NAN_BITS, dtype=torch.int16, device=DEV).view(BF16)
    m3, s3 = (ctypes.c_float * 3)(*A.MEAN), (ctypes.c_float * 3)(*A.STD)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(frames=_ptr(fr), Bs=BS, H0=H0, W0=W0, keep=_ptr(keep), aug_i=_ptr(aug), mix_i=None, mix_f=None, B=B, tubes=TUBES,
                tubelet=TB, n=PPF, img=IMG, patch=PATCH, mean3=m3, std3=s3, out=_ptr(out), ldo=KC + 8)
    bad = [("frames", None), ("keep", None), ("aug_i", None), ("out", None), ("mean3", None), ("std3", None), ("mix_i", _ptr(mi)),
           ("mix_f", _ptr(mf)), ("Bs", 0), ("Bs", -1), ("H0", 0), ("W0", 0), ("B", 0), ("tubes", 0), ("tubelet", -1), ("n", 0), ("patch", 0),
           ("img", 0), ("img", IMG + 4), ("patch", 4), ("ldo", KC + 4), ("ldo", KC - 8), ("out", _ptr(out, 8))]
    for key, val in bad:
        args = dict(base)
        args[key] = val
        assert lib.tvts_patch_gather_tube_u8_aug(*args.values(), st) == EINVAL, (key, val)
    torch.cuda.synchronize()
    assert (out.view(torch.int16) == NAN_BITS).all()
    for extra in (dict(), dict(mix_i=_ptr(mi), mix_f=_ptr(mf))):   # the unchanged arguments are accepted, with and without a mix
        assert lib.tvts_patch_gather_tube_u8_aug(*dict(base, **extra).values(), st) == 0
    torch.cuda.synchronize()
    g = out.view(torch.int16)
    assert not (g[:B * TUBES * PPF, :KC] == NAN_BITS).any() and (g[:, KC:] == NAN_BITS).all() and (g[B * TUBES * PPF:] == NAN_BITS).all()


def test_aug_table_refuses_every_out_of_range_column(K):
    good = np.array(ERASED, dtype=np.int64)
    K.aug_table(good, Bs=BS, H0=H0, W0=W0, img=IMG, device=DEV)
    for col, value in [(0, BS), (0, -1), (1, -1), (1, H0), (2, -1), (2, W0), (3, 0), (3, H0 + 1), (4, 0), (4, W0 + 1), (5, 2), (5, -1), (6, 4),
                       (6, -1), (7, -1), (7, IMG), (8, -1), (8, IMG), (9, -1), (9, IMG + 1), (10, -1), (10, IMG + 1), (12, 1 << 32), (13, 1),
                       (14, -1), (15, 5)]:
        bad = good.copy()
        bad[1, col] = value
        with pytest.raises(ValueError):
            K.aug_table(bad, Bs=BS, H0=H0, W0=W0, img=IMG, device=DEV)


# ================================================================================================ 7. the step, end to end
def drawn_plans(img, classes):
    """a seeded Augment draw for BS clips x NS views that erases at least one sample and flips at least one, and a seeded Mixup
    draw in elem mode that holds a mixup and a cutmix sample"""
    import random
    import v1_mixup_ref as M
    from tvts_amd.downstream.finetune_v1 import Augment, Mixup
    py_state, np_state = random.getstate(), np.random.get_state()
    try:
        for seed in range(200):
            random.seed(seed)
            np.random.seed(seed)
            plan = Augment(img, hflip=0.5, reprob=0.5, remode="pixel", num_sample=NS, noise_seed=seed).draw(BS, 70, 90)
            mix = Mixup(num_classes=classes, mode="elem", label_smoothing=0.1, **M.DEFAULT).draw(len(plan), img)
            if (plan.aug_i[:, 6] > 0).any() and (plan.aug_i[:, 5] == 1).any() and M.holds("both", mix.mix_i):
                return plan, mix
    finally:
        random.setstate(py_state)
        np.random.set_state(np_state)
    raise AssertionError("no seed below 200 draws an erased, a flipped, a mixup and a cutmix sample")


def run_step(m, samples, targets, **kw):
    """one step with update_freq 2 (the first call accumulates: the gradient stays in the store) -> loss, logits, flat gradient"""
    from test_v1_finetune_gpu import stepper
    from tvts_amd import hip
    hip.zero_(m.store.grad)
    step, _ = stepper(m, clip_grad=0.05, update_freq=2, smoothing=0.1)
    out = step.step(samples, targets, **kw)
    torch.cuda.synchronize()
    return dict(loss=out["loss"].reshape(1).clone(), logits=out["logits"].clone(), gradient=m.store.grad.clone())


def same_bits(a, b, what):
    for nm in a:
        x, y = a[nm].view(torch.int32).cpu(), b[nm].view(torch.int32).cpu()
        assert torch.equal(x, y), f"{what}: {nm}: {int((x != y).sum())} of {x.numel()} elements differ"


def test_step_with_a_plan_is_the_step_on_the_gathered_clip(K):
    """the new gather with all patches kept, its bf16 rows folded back into an fp32 clip, fed to a twin model's step(clip, targets):
    step(frames_u8, targets, aug=plan) gives the twin's loss, logits and whole flat gradient bit for bit; the same with a MixPlan
    (the twin gets the already mixed clip and the soft targets of K.mix_targets); aug=None before and after gives identical bits"""
    from test_v1_finetune_gpu import F, build
    kw, C = S.TINY, F["classes"]
    img, patch, tb, frames_n = kw["img_size"], kw["patch_size"], kw["tubelet_size"], 8
    fr = A.case_frames(31, BS, 70, 90, frames=frames_n)
    plan, mix = drawn_plans(img, C)
    labels = torch.randint(0, C, (BS,), generator=torch.Generator().manual_seed(64)).repeat_interleave(NS)
    m, twin = build(rate=0.0), build(rate=0.0)
    keep = full_keep(B, frames_n // tb, (img // patch) ** 2)
    fr_t = torch.from_numpy(fr)
    centre = torch.from_numpy(A.case_frames(32, B, 70, 90, frames=frames_n))
    before = run_step(m, centre, labels)
    for what, mplan in (("aug", None), ("aug + mix", mix)):
        rows, _ = launch(K, fr, plan.aug_i, mix=None if mplan is None else (mplan.mix_i, mplan.mix_f), img=img, patch=patch, tb=tb)
        clip = torch.from_numpy(fold(rows, keep, img, patch, tb)).to(F32)
        assert not torch.isnan(clip).any()
        targets = labels
        if mplan is not None:
            soft = torch.empty(B, C, dtype=F32, device=DEV)
            K.mix_targets(labels.to(torch.int32).to(DEV), K.mix_table(mplan.mix_i, mplan.mix_f, B=B, img=img, device=DEV), soft,
                          smoothing=mplan.smoothing)
            targets = soft.cpu()
        got = run_step(m, fr_t, labels, aug=plan, mix=mplan)
        want = run_step(twin, clip, targets)
        same_bits(got, want, what)
        assert not torch.equal(got["logits"], before["logits"])
    same_bits(run_step(m, centre, labels), before, "aug=None after the aug calls")


def test_step_refuses_fp32_samples_with_a_plan(K):
    from test_v1_finetune_gpu import build, stepper
    from tvts_amd.downstream.finetune_v1 import Augment
    m = build(rate=0.0)
    step, _ = stepper(m)
    plan = Augment(S.TINY["img_size"], reprob=0.0).draw(2, 70, 90)
    with pytest.raises(ValueError):
        step.step(S.synth_clip(S.TINY, 2, 8, 1), torch.tensor([0, 1]), aug=plan)
    with pytest.raises(ValueError):
        m.engine.finetune_forward(S.synth_clip(S.TINY, 2, 8, 1).to(DEV), 2, 4, aug=K.aug_table(plan.aug_i, Bs=2, H0=70, W0=90, img=64, device=DEV))
