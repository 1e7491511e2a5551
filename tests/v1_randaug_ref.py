"""numpy restatement of the fifteen RandAugment operations of v1/downstream/rand_augment.py as PIL computes them on uint8 RGB
frames -- the arithmetic tvts_amd/csrc/randaug.hip is held to, bit for bit.  tests/test_v1_randaug_cpu.py pins it to the reference's
own run under PIL (tests/golden/v1_randaug.npz) and, where PIL imports, to PIL directly on fresh frames.

Every function takes and returns one frame uint8 [H, W, 3].  ``apply_row`` runs one row of a RandAugment plan (the table of
tvts_amd.downstream.finetune_v1.ra_row: op code, resample, integer argument; affine a..f, blend factor); ``apply_named`` runs
an operation by the name of the reference function with the argument the reference passed it.

PIL's types are kept: double for coordinates and interpolation, float (numpy float32, every operation rounded, no FMA) for the
blends and the SMOOTH filter, integers for the tables."""
import numpy as np

from tvts_amd.downstream import finetune_v1 as F

FILL = 128


def to_l(fr):
    """Image.convert("L") of an RGB frame -> uint8 [H, W]"""
    f = fr.astype(np.int64)
    return ((19595 * f[..., 0] + 38470 * f[..., 1] + 7471 * f[..., 2] + 0x8000) >> 16).astype(np.uint8)


def hist4(fr):
    """-> int64 [4, 256]: the histograms of R, G, B and L"""
    h = [np.bincount(fr[..., c].ravel(), minlength=256) for c in range(3)]
    h.append(np.bincount(to_l(fr).ravel(), minlength=256))
    return np.stack(h).astype(np.int64)


def point(fr, lut):
    """lut integer [3, 256] (or [256] for all channels)"""
    lut = np.broadcast_to(np.asarray(lut), (3, 256))
    return np.stack([lut[c][fr[..., c]] for c in range(3)], axis=-1).astype(np.uint8)


def lut_invert():
    return 255 - np.arange(256)


def lut_solarize(thresh):
    i = np.arange(256)
    return np.where(i < thresh, i, 255 - i)


def lut_solarize_add(add):
    i = np.arange(256)
    return np.where(i < 128, np.minimum(255, i + add), i)


def lut_posterize(bits):
    return np.arange(256) & ~(2 ** (8 - bits) - 1)


def lut_autocontrast(h):
    """h: one channel's histogram [256]"""
    nz = np.nonzero(h)[0]
    if len(nz) == 0:
        return np.arange(256)
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    return np.array([min(255, max(0, int(i * scale + off))) for i in range(256)])


def lut_equalize(h):
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return np.arange(256)
    step = (sum(nz) - nz[-1]) // 255
    if step == 0:
        return np.arange(256)
    n, lut = step // 2, []
    for i in range(256):
        lut.append(min(n // step, 255))
        n += int(h[i])
    return np.array(lut)


def blend(deg, fr, factor):
    """Image.blend(degenerate, image, factor) in float"""
    f = np.float32(factor)
    d, i = deg.astype(np.float32), fr.astype(np.float32)
    t = d + f * (i - d)
    if not (np.float32(0) <= f <= np.float32(1)):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)  # truncation


def smooth(fr):
    """ImageFilter.SMOOTH: 3 x 3 (1 1 1 / 1 5 1 / 1 1 1) / 13 in float, rows from the bottom one up, the one-pixel border copied"""
    H, W, _ = fr.shape
    out = fr.copy()
    if H < 3 or W < 3:
        return out
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float64) / 13).astype(np.float32)
    f = fr.astype(np.float32)
    ss = np.full((H - 2, W - 2, 3), np.float32(0.5), dtype=np.float32)
    for r, dy in ((0, 2), (1, 1), (2, 0)):  # the kernel's first row goes with the row below
        rows = f[dy:dy + H - 2]
        ss = ss + ((rows[:, 0:W - 2] * k[3 * r] + rows[:, 1:W - 1] * k[3 * r + 1]) + rows[:, 2:W] * k[3 * r + 2])
    out[1:-1, 1:-1] = np.clip(ss, np.float32(0), np.float32(255)).astype(np.int32).astype(np.uint8)
    return out


def affine(fr, coef, resample):
    """Image.transform(size, AFFINE, coef, resample, fillcolor=(128, 128, 128)); resample 2 bilinear, 3 bicubic"""
    H, W, _ = fr.shape
    a, b, c, d, e, f = (float(v) for v in coef)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64) + 0.5)
    xin = a * xs + b * ys + c
    yin = d * xs + e * ys + f
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x0, y0 = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    src = fr.astype(np.float64)

    def tap(yy, xx):
        return src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    if resample == 2:
        v1 = tap(y0, x0) + (tap(y0, x0 + 1) - tap(y0, x0)) * dx
        v2 = tap(y0 + 1, x0) + (tap(y0 + 1, x0 + 1) - tap(y0 + 1, x0)) * dx
        v = v1 + (v2 - v1) * dy
        out = v.astype(np.int64)
    elif resample == 3:
        def cubic(v1, v2, v3, v4, t):
            p1 = v2
            p2 = -v1 + v3
            p3 = 2 * (v1 - v2) + v3 - v4
            p4 = -v1 + v2 - v3 + v4
            return p1 + t * (p2 + t * (p3 + t * p4))
        rows = [cubic(*(tap(y0 - 1 + r, x0 - 1 + k) for k in range(4)), dx) for r in range(4)]
        v = cubic(*rows, dy)
        out = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v.astype(np.int64)))
    else:
        raise ValueError("resample: 2 (bilinear) or 3 (bicubic)")
    return np.where(inside[..., None], out, FILL).astype(np.uint8)


def apply_row(fr, ri, rd):
    """one plan row on one frame: ri = (op, resample, iarg, 0), rd = (a, b, c, d, e, f, factor, 0)"""
    op, resample, iarg = int(ri[0]), int(ri[1]), int(ri[2])
    if op == F.RA_NONE:
        return fr.copy()
    if op == F.RA_AUTOCONTRAST:
        h = hist4(fr)
        return point(fr, [lut_autocontrast(h[c]) for c in range(3)])
    if op == F.RA_EQUALIZE:
        h = hist4(fr)
        return point(fr, [lut_equalize(h[c]) for c in range(3)])
    if op == F.RA_INVERT:
        return point(fr, lut_invert())
    if op == F.RA_SOLARIZE:
        return point(fr, lut_solarize(iarg))
    if op == F.RA_SOLARIZE_ADD:
        return point(fr, lut_solarize_add(iarg))
    if op == F.RA_POSTERIZE:
        return point(fr, lut_posterize(iarg))
    if op == F.RA_COLOR:
        return blend(np.repeat(to_l(fr)[..., None], 3, axis=-1), fr, rd[6])
    if op == F.RA_CONTRAST:
        h = hist4(fr)[3]
        mean = int(float(int((h * np.arange(256)).sum())) / float(fr.shape[0] * fr.shape[1]) + 0.5)
        return blend(np.full_like(fr, mean), fr, rd[6])
    if op == F.RA_BRIGHTNESS:
        return blend(np.zeros_like(fr), fr, rd[6])
    if op == F.RA_SHARPNESS:
        return blend(smooth(fr), fr, rd[6])
    if op == F.RA_AFFINE:
        return affine(fr, rd[:6], resample)
    raise ValueError(f"op code {op}")


def apply_named(fr, fn, arg, resample):
    """the reference function `fn` (its __name__) with the level argument the reference passed (None for the three without)"""
    ri, rd = F.ra_row(fn, arg, resample, fr.shape[0], fr.shape[1])
    return apply_row(fr, ri, rd)


def apply_plan(frames, ra_i, ra_d, num_sample):
    """frames uint8 [Bs, T, H, W, 3], a plan [B, L, 4] / [B, L, 8] -> the augmented views uint8 [B, T, H, W, 3]"""
    out = []
    for b in range(ra_i.shape[0]):
        clip = frames[b // num_sample]
        for j in range(ra_i.shape[1]):
            if int(ra_i[b, j, 0]) != F.RA_NONE:
                clip = np.stack([apply_row(f, ra_i[b, j], ra_d[b, j]) for f in clip])
        out.append(np.array(clip))
    return np.stack(out)


def case_frames(seed, n, H, W):
    """seeded uint8 frames [n, H, W, 3]: smooth blobs plus noise, so that histograms have empty ends and equalize has work to do"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((n, H, W, 3), dtype=np.uint8)
    for i in range(n):
        for c in range(3):
            base = 110 + 70 * np.sin(x / rng.uniform(3, 9) + rng.uniform(0, 6)) * np.cos(y / rng.uniform(3, 9) + rng.uniform(0, 6))
            out[i, ..., c] = np.clip(base + rng.randint(-7, 8, size=(H, W)) + rng.randint(-20, 30), 3 + 4 * c, 250 - 9 * c)
    return out
