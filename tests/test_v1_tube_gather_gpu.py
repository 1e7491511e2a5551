"""The seven v1 tubelet gathers are one kernel frame over four source policies (tvts_amd/csrc/embed.hip: tube_gather_kernel), so
the tests that compare one entry point with another compare the frame with itself.  Here every entry point is pinned to the HOST
im2col of the host-normalised clip, bit for bit, at the edges of the frame's column loop (run with -m gpu)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
from test_v1_mixup_gpu import GEOMS  # noqa: E402  K = 384, 3072, 6144: under one 2048-column pass of the block, one and a half, three
from v1_gather_ref import im2col_ref, normalise_u8  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16
B = 2


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_every_entry_point_against_the_host_im2col(K, geom):
    """neutral tables (mode-0 mix rows whose partner, box and lam would show; aug rows with h == w == img, no flip, no erase; view
    rows with t0 = 0, tstep = 1) on one seeded input: source frames larger than img behind a non-zero crop per sample, keep a
    shuffled strict subset, ldo = K + 8 with the guard columns and rows checked"""
    img, p, tb, T = geom
    tubes, ppf, H0, W0 = T // tb, (img // p) ** 2, img + 5, img + 7
    n, Kc = ppf - 1, 3 * tb * p * p
    g = torch.Generator().manual_seed(1700 + Kc)
    frames = torch.randint(0, 256, (B, T, H0, W0, 3), generator=g, dtype=torch.uint8)
    keep = torch.stack([torch.stack([torch.randperm(ppf, generator=g)[:n] for _ in range(tubes)]) for _ in range(B)])
    assert n < ppf and any(not torch.equal(k, k.sort().values) for k in keep.reshape(-1, n))
    crop = [[1, 6], [4, 2]]
    cut = torch.stack([frames[b, :, y:y + img, x:x + img] for b, (y, x) in enumerate(crop)])
    video = normalise_u8(cut).permute(0, 1, 4, 2, 3).contiguous()            # [B, T, 3, img, img]
    want = im2col_ref(video, keep, tb, p).bfloat16()
    # the table forms name their source clip: sample b reads clip 1 - b there
    video_x = video.flip(0)
    want_x = im2col_ref(video_x, keep, tb, p).bfloat16()
    src_rows = [[1 - b, *crop[1 - b]] for b in range(B)]

    fr_d, keep_d = frames.to(DEV), keep.to(torch.int32).to(DEV)
    video_d, cm_d = video.to(DEV), video.permute(0, 2, 1, 3, 4).contiguous().to(DEV)
    crop_d = torch.tensor(crop, dtype=torch.int32, device=DEV)
    mix = K.mix_table(np.array([[1, 0, 2, img - 3, 1, img - 2], [0, 0, 0, img, 0, img]]), np.array([[0.25, 0.75], [0.0, 1.0]]),
                      B=B, img=img, device=DEV)
    aug = K.aug_table(np.array([[s, y, x, img, img, 0, 0, 0, 0, 0, 0, 77 + s, 5, 0, 0, 0] for s, y, x in src_rows]), Bs=B, H0=H0, W0=W0,
                      img=img, device=DEV)
    view = K.view_table(np.array([[s, 0, 1, y, x, 0, 0, 0] for s, y, x in src_rows]), Bs=B, Tsrc=T, H0=H0, W0=W0, T=T, img=img,
                        device=DEV)
    kw = dict(B=B, tubes=tubes, tubelet=tb, n=n, img=img, patch=p)
    forms = [
        ("tube", want, lambda o: K.patch_gather_tube(video_d, keep_d, o, **kw)),
        ("tube_cm", want, lambda o: K.patch_gather_tube(cm_d, keep_d, o, channel_major=True, **kw)),
        ("tube_cm_mix", want, lambda o: K.patch_gather_tube_mix(cm_d, keep_d, o, mix, **kw)),
        ("tube_u8", want, lambda o: K.patch_gather_tube_u8(fr_d, keep_d, o, crop=crop_d, **kw)),
        ("tube_u8_mix", want, lambda o: K.patch_gather_tube_u8_mix(fr_d, keep_d, o, mix, crop=crop_d, **kw)),
        ("tube_u8_aug", want_x, lambda o: K.patch_gather_tube_u8_aug(fr_d, keep_d, o, aug, **kw)),
        ("tube_u8_aug + mix", want_x, lambda o: K.patch_gather_tube_u8_aug(fr_d, keep_d, o, aug, mix, **kw)),
        ("tube_u8_view", want_x, lambda o: K.patch_gather_tube_u8_view(fr_d, keep_d, o, view, **kw)),
    ]
    M = B * tubes * n
    for name, ref, run in forms:
        buf, out = KB.guarded(M, Kc, BF16, DEV)
        assert out.stride(0) == Kc + 8
        run(out)
        torch.cuda.synchronize()
        what = f"tvts_patch_gather_{name} at {geom}"
        KB.check_guards(buf, M, Kc, what)
        KB.assert_equal_bits(out.cpu(), ref, what + " against the host im2col")
