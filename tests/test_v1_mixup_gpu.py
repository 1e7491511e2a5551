"""Mixup / CutMix fused into the v1 fine-tuning step (run with -m gpu).  Every comparison is of bytes.

The expected mixed clip and soft targets come from tests/v1_mixup_ref.py, a torch-CPU restatement of the mix table's semantics; for
every case of tests/golden/v1_mixup.npz the tests first check that the restatement's sha256 is the one recorded from the reference
class's own run, and then use it as the expected value.  The fp32 mix kernel is compared with the EXISTING channel-major gather
run on the restatement's mixed clip, the uint8 mix kernel with the fp32 mix kernel on host-cropped, host-normalised frames, the
soft targets with the reference's, and FinetuneStep.step(clip, labels, mix=plan) with the same step on the host-mixed clip and
host-built soft targets: loss, logits, grad norm and the parameter store after one update."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import v1_downstream_synth as S  # noqa: E402
import v1_mixup_ref as M  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
EINVAL = -22
NAMES = list(M.CASES)
# (img, patch, tubelet, frames): K = 3 * tubelet * patch^2 = 384 (less than one 2048-column pass of the block), 3072 (two), 6144 (three)
GEOMS = [(32, 8, 2, 4), (64, 16, 4, 4), (64, 32, 2, 4)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


@pytest.fixture(scope="module")
def fx(golden):
    return golden("v1_mixup")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(rows, cols, dtype, pad=8, extra=2):
    """-> (view [rows, cols] with leading dimension cols + pad inside a NaN-filled buffer of rows + extra rows, the buffer)"""
    buf = torch.full((rows + extra, cols + pad), NAN, dtype=dtype, device=DEV)
    return buf[:rows, :cols], buf


def guards_intact(view, buf):
    rows, cols = view.shape
    assert torch.isnan(buf[:rows, cols:]).all() and torch.isnan(buf[rows:]).all(), "the kernel wrote outside its output"


def same_bytes(a, b, what):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ai, bi = a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32)
    bad = int((ai != bi).sum())
    assert bad == 0, f"{what}: {bad} of {ai.numel()} elements differ"


def keep_of(B, tubes, img, patch):
    """every patch of every tube, in DEScending order (so that a row's patch is not its index)"""
    ppf = (img // patch) ** 2
    return torch.arange(ppf - 1, -1, -1, dtype=torch.int32).repeat(B, tubes, 1).contiguous().to(DEV)


def geom_kw(B, geom):
    img, patch, tb, frames = geom
    return dict(B=B, tubes=frames // tb, tubelet=tb, n=(img // patch) ** 2, img=img, patch=patch)


def gather_plain(K, clip, geom):
    """the existing channel-major gather on an fp32 clip [B, 3, T, img, img] -> bf16 rows on the device"""
    kw = geom_kw(clip.shape[0], geom)
    out, buf = guarded(kw["B"] * kw["tubes"] * kw["n"], 3 * kw["tubelet"] * kw["patch"] ** 2, BF16)
    K.patch_gather_tube(clip.to(DEV).contiguous(), keep_of(kw["B"], kw["tubes"], kw["img"], kw["patch"]), out, channel_major=True, **kw)
    guards_intact(out, buf)
    return out


def gather_mix(K, clip, mi, mf, geom):
    kw = geom_kw(clip.shape[0], geom)
    out, buf = guarded(kw["B"] * kw["tubes"] * kw["n"], 3 * kw["tubelet"] * kw["patch"] ** 2, BF16)
    table = K.mix_table(mi, mf, B=kw["B"], img=kw["img"], device=DEV)
    K.patch_gather_tube_mix(clip.to(DEV).contiguous(), keep_of(kw["B"], kw["tubes"], kw["img"], kw["patch"]), out, table, **kw)
    guards_intact(out, buf)
    return out


def check_fp32(K, clip, mi, mf, geom, what):
    mi, mf = np.asarray(mi, dtype=np.int32), np.asarray(mf, dtype=np.float32)
    want = gather_plain(K, M.mix_clip(clip, mi, mf), geom)
    same_bytes(gather_mix(K, clip, mi, mf, geom), want, what)
    return want


# ================================================================================================ 1. the fp32 mix kernel
@pytest.mark.parametrize("name", NAMES)
def test_fp32_mix_every_fixture_case(K, fx, name):
    mi, mf = fx[name + ".mix_i"], fx[name + ".mix_f"]
    for geom in GEOMS:
        clip, _ = M.case_inputs(fx, name, img=geom[0], frames=geom[3])
        if geom[0] == M.IMG:  # the fixture's own size: the restatement is pinned to the reference's run first
            assert M.sha256(M.mix_clip(clip, mi, mf)) == str(fx[name + ".sha256"])
        check_fp32(K, clip, mi, mf, geom, f"{name} at {geom}")


def hand_plans(img, patch, frames):
    """eight samples, one hand-made row each -> (mix_i, mix_f)"""
    p = patch
    rows = [
        (3, 2, 5, 5, 0, img),              # an empty box (yl == yh)
        (4, 2, 0, img, 0, img),            # the whole image
        (7, 2, 3, img - 3, 11, 12),        # one pixel wide, inside one 8-pixel group
        (0, 2, p, 2 * p, p, 2 * p),        # edges on patch boundaries
        (4, 1, 0, 0, 0, 0),                # partner == self, mixup
        (5, 2, 1, img - 1, 9, img - 7),    # partner == self, cutmix; cut inside the first and the last 8-pixel group
        (1, 3, 1, frames - 1, 5, img - 12),  # pair-mode cutmix: the frames [1, frames - 1), the rows [5, img - 12)
        (2, 0, 0, img, 0, img),            # unmixed (the box is not read)
    ]
    lam = np.array([[0.3, 0.7], [0.0, 1.0], [0.9, 0.1], [0.5, 0.5], [0.37, 0.63], [0.2, 0.8], [0.6, 0.4], [0.123, 0.877]], dtype=np.float32)
    return np.array(rows, dtype=np.int32), lam


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_fp32_mix_hand_made_plans(K, geom):
    img, patch, tb, frames = geom
    clip = S.synth_clip(dict(img_size=img), 8, frames, 31 + img + patch)
    clip[7, :, :, 2, :9] = -0.0   # the unmixed sample holds -0.0: the sign survives
    clip[7, 1, 1, 3, 4] = NAN
    mi, mf = hand_plans(img, patch, frames)
    want = check_fp32(K, clip, mi, mf, geom, f"hand-made plans at {geom}")
    kw = geom_kw(8, geom)
    rows7 = want[7 * kw["tubes"] * kw["n"]:].view(torch.int16)
    assert int((rows7 == -32768).sum()) == 3 * frames * 9  # bf16 -0.0 = 0x8000, every one of them
    # B = 2: a mixup sample and a cutmix sample, each other's partners
    mi2 = np.array([[1, 1, 0, 0, 0, 0], [0, 2, 7, 19, 13, 30]], dtype=np.int32)
    check_fp32(K, clip[:2], mi2, mf[:2], geom, f"B = 2 at {geom}")


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_all_mode_zero_is_the_unmixed_kernel(K, geom):
    """a table of mode-0 rows (partner, box and lam hold values that would show): the bytes of tvts_patch_gather_tube_cm on the
    clip itself, -0.0 and NaN included"""
    img, patch, tb, frames = geom
    clip = S.synth_clip(dict(img_size=img), 4, frames, 77 + patch)
    clip[0, 0, 0, 0, :8] = -0.0
    clip[3, 2, frames - 1, img - 1, img - 3:] = torch.tensor([NAN, float("inf"), -0.0])
    mi = np.array([[1, 0, 2, 9, 3, 11], [0, 0, 0, img, 0, img], [3, 0, 0, 0, 0, 0], [2, 0, 5, 6, 7, 8]], dtype=np.int32)
    mf = np.array([[0.5, 0.5], [0.0, 1.0], [1.0, 0.0], [0.25, 0.75]], dtype=np.float32)
    same_bytes(gather_mix(K, clip, mi, mf, geom), gather_plain(K, clip, geom), f"mode 0 at {geom}")


# ================================================================================================ 2. the uint8 mix kernel
def u8_case(B, img, frames, seed):
    """frames uint8 [B, T, img + 5, img + 5, 3], a different crop per sample, and the host-cropped, host-normalised clip"""
    H0 = W0 = img + 5
    fr = torch.randint(0, 256, (B, frames, H0, W0, 3), generator=gen(seed), dtype=torch.uint8)
    crop = torch.tensor([[(2 * b + 1) % 6, (5 - b) % 6] for b in range(B)], dtype=torch.int32)
    mean, std = torch.tensor(MEAN).view(1, 1, 1, 3), torch.tensor(STD).view(1, 1, 1, 3)
    clip = torch.stack([((fr[b, :, int(y0):int(y0) + img, int(x0):int(x0) + img].float() / 255 - mean) / std).permute(3, 0, 1, 2)
                        for b, (y0, x0) in enumerate(crop)]).contiguous()
    return fr, crop, clip


@pytest.mark.parametrize("plan", ["batch_mixup", "batch_cutmix", "pair", "elem_prob"])
@pytest.mark.parametrize("geom", GEOMS[:2], ids=str)
def test_u8_mix_is_the_fp32_mix_on_host_normalised_frames(K, fx, geom, plan):
    img, patch, tb, frames = geom
    mi, mf = fx[plan + ".mix_i"], fx[plan + ".mix_f"]
    fr, crop, clip = u8_case(M.B, img, frames, 5 + img)
    assert len({tuple(c.tolist()) for c in crop}) == M.B
    kw = geom_kw(M.B, geom)
    out, buf = guarded(kw["B"] * kw["tubes"] * kw["n"], 3 * tb * patch * patch, BF16)
    table = K.mix_table(mi, mf, B=M.B, img=img, device=DEV)
    K.patch_gather_tube_u8_mix(fr.to(DEV), keep_of(M.B, kw["tubes"], img, patch), out, table, crop=crop.to(DEV), **kw)
    guards_intact(out, buf)
    same_bytes(out, gather_mix(K, clip, mi, mf, geom), f"uint8 {plan} at {geom}")
    same_bytes(out, gather_plain(K, M.mix_clip(clip, mi, mf), geom), f"uint8 {plan} at {geom} against the host mix")


def test_u8_mix_centre_crop_and_mode_zero(K):
    """crop = NULL: both samples take the centre crop; an all-mode-0 table gives the unmixed uint8 kernel's bytes"""
    geom = GEOMS[0]
    img, patch, tb, frames = geom
    fr, _, _ = u8_case(2, img, frames, 17)
    kw = geom_kw(2, geom)
    keep = keep_of(2, kw["tubes"], img, patch)
    mean, std = torch.tensor(MEAN).view(1, 1, 1, 1, 3), torch.tensor(STD).view(1, 1, 1, 1, 3)
    clip = ((fr[:, :, 2:2 + img, 2:2 + img].float() / 255 - mean) / std).permute(0, 4, 1, 2, 3).contiguous()  # (5 - 0) / 2 -> 2
    outs = []
    for mi in ([[1, 1, 0, 0, 0, 0], [0, 2, 3, 30, 5, 18]], [[1, 0, 0, 9, 0, 9], [0, 0, 0, 0, 0, 0]]):
        mi, mf = np.array(mi, dtype=np.int32), np.array([[0.25, 0.75], [0.5, 0.5]], dtype=np.float32)
        out, buf = guarded(2 * kw["tubes"] * kw["n"], 3 * tb * patch * patch, BF16)
        K.patch_gather_tube_u8_mix(fr.to(DEV), keep, out, K.mix_table(mi, mf, B=2, img=img, device=DEV), **kw)
        guards_intact(out, buf)
        same_bytes(out, gather_plain(K, M.mix_clip(clip, mi, mf), geom), "uint8 mix, centre crop")
        outs.append(out)
    plain, buf = guarded(2 * kw["tubes"] * kw["n"], 3 * tb * patch * patch, BF16)
    K.patch_gather_tube_u8(fr.to(DEV), keep, plain, **kw)
    same_bytes(outs[1], plain, "uint8 mix, all mode 0, against tvts_patch_gather_tube_u8")


# ================================================================================================ 3. soft targets
@pytest.mark.parametrize("name", NAMES)
def test_mix_targets_every_fixture_case(K, fx, name):
    C, eps = int(fx[name + ".classes"]), float(fx[name + ".smoothing"])
    _, labels = M.case_inputs(fx, name)
    out, buf = guarded(M.B, C, F32, pad=3)
    table = K.mix_table(fx[name + ".mix_i"], fx[name + ".mix_f"], B=M.B, img=M.IMG, device=DEV)
    K.mix_targets(labels.to(torch.int32).to(DEV), table, out, smoothing=eps)
    guards_intact(out, buf)
    same_bytes(out, torch.from_numpy(fx[name + ".targets"]), f"{name}: soft targets against the reference's")


@pytest.mark.parametrize("C", [5, 174, 1000])
def test_mix_targets_same_label_and_unmixed_rows(K, C):
    """partners with the same label, a partner that is the sample itself, an unmixed row whose lam cells hold values that would
    show; against the restatement"""
    labels = torch.tensor([2, C - 1, 2, 0, C - 1, 3])
    mi = np.array([[2, 1, 0, 0, 0, 0], [4, 2, 0, 8, 0, 8], [0, 3, 0, 2, 0, 8], [3, 1, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0], [1, 2, 0, 0, 0, 0]],
                  dtype=np.int32)
    mf = np.array([[0.3, 0.7], [0.9375, 0.0625], [0.1, 0.9], [0.6, 0.4], [0.5, 0.5], [1.0, 0.0]], dtype=np.float32)
    for eps in (0.0, 0.1):
        out, buf = guarded(6, C, F32, pad=5)
        K.mix_targets(labels.to(torch.int32).to(DEV), K.mix_table(mi, mf, B=6, img=8, device=DEV), out, smoothing=eps)
        guards_intact(out, buf)
        same_bytes(out, M.mix_targets(labels, mi, mf, C, eps), f"soft targets C={C} smoothing={eps}")


# ================================================================================================ 4. refusals
def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def test_einval_for_each_refused_argument(K):
    """null pointers, non-positive sizes, the alignment / ldo conditions: TVTS_EINVAL and nothing launched (the outputs keep
    their NaN fill)"""
    lib = K._lib.load()
    img, patch, tb, frames = GEOMS[0]
    B, tubes, n, Kc = 2, frames // tb, (img // patch) ** 2, 3 * tb * patch * patch
    clip = S.synth_clip(dict(img_size=img), B, frames, 3).to(DEV)
    fr = torch.zeros(B, frames, img + 5, img + 5, 3, dtype=torch.uint8, device=DEV)
    keep = keep_of(B, tubes, img, patch)
    mi, mf = K.mix_table(np.array([[1, 1, 0, 0, 0, 0], [0, 2, 0, 8, 0, 8]]), np.array([[0.5, 0.5], [0.5, 0.5]]), B=B, img=img, device=DEV)
    out = torch.full((B * tubes * n + 2, Kc + 8), NAN, dtype=BF16, device=DEV)
    m3, s3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    cm = dict(video=_ptr(clip), keep=_ptr(keep), mix_i=_ptr(mi), mix_f=_ptr(mf), B=B, tubes=tubes, tubelet=tb, n=n, img=img,
              patch=patch, out=_ptr(out), ldo=Kc + 8)
    u8 = dict(frames=_ptr(fr), H0=img + 5, W0=img + 5, crop=None, keep=_ptr(keep), mix_i=_ptr(mi), mix_f=_ptr(mf), B=B, tubes=tubes,
              tubelet=tb, n=n, img=img, patch=patch, mean3=m3, std3=s3, out=_ptr(out), ldo=Kc + 8)
    bad_common = [("keep", None), ("mix_i", None), ("mix_f", None), ("out", None), ("B", 0), ("tubes", 0), ("tubelet", -1), ("n", 0),
                  ("patch", 0), ("img", 0), ("img", img + 4), ("patch", 4), ("ldo", Kc + 4), ("ldo", Kc - 8), ("out", _ptr(out, 8))]
    for fn, base, extra in ((lib.tvts_patch_gather_tube_cm_mix, cm, [("video", None), ("video", _ptr(clip, 4))]),
                            (lib.tvts_patch_gather_tube_u8_mix, u8, [("frames", None), ("mean3", None), ("std3", None),
                                                                    ("H0", img - 1), ("W0", img - 1)])):
        for key, val in bad_common + extra:
            args = dict(base)
            args[key] = val
            assert fn(*args.values(), st) == EINVAL, (fn.__name__, key, val)
    # the unmixed forms of the same frame: the alignment conditions, and the NULL pointers of tvts_patch_gather_tube (nothing is
    # read before the refusal, so the channel-major clip stands in for a frame-major one)
    plain, plain_u8 = ({k: v for k, v in d.items() if k not in ("mix_i", "mix_f")} for d in (cm, u8))
    for fn, base, bad in ((lib.tvts_patch_gather_tube, plain, [("video", None), ("keep", None), ("out", None), ("video", _ptr(clip, 4)),
                                                               ("out", _ptr(out, 8))]),
                          (lib.tvts_patch_gather_tube_cm, plain, [("video", _ptr(clip, 4)), ("out", _ptr(out, 8))]),
                          (lib.tvts_patch_gather_tube_u8, plain_u8, [("out", _ptr(out, 8))])):
        for key, val in bad:
            args = dict(base)
            args[key] = val
            assert fn(*args.values(), st) == EINVAL, (fn.__name__, key, val)
    lab = torch.zeros(B, dtype=torch.int32, device=DEV)
    tout = torch.full((B + 1, 16), NAN, dtype=F32, device=DEV)
    mt = dict(labels=_ptr(lab), mix_i=_ptr(mi), mix_f=_ptr(mf), B=B, C=5, smoothing=0.1, out=_ptr(tout), ldo=16)
    for key, val in [("labels", None), ("mix_i", None), ("mix_f", None), ("out", None), ("B", 0), ("C", 0), ("ldo", 4), ("smoothing", -0.1),
                     ("smoothing", 1.0), ("smoothing", NAN)]:
        args = dict(mt)
        args[key] = val
        assert lib.tvts_mix_targets(*args.values(), st) == EINVAL, ("tvts_mix_targets", key, val)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(tout).all()
    # the unchanged arguments are accepted
    assert lib.tvts_patch_gather_tube_cm_mix(*cm.values(), st) == 0 and lib.tvts_patch_gather_tube_u8_mix(*u8.values(), st) == 0
    assert lib.tvts_mix_targets(*mt.values(), st) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out[:B * tubes * n, :Kc]).any() and torch.isnan(out[:, Kc:]).all() and not torch.isnan(tout[:B, :5]).any()


def test_wrappers_refuse_a_bad_plan_before_the_upload(K):
    for mi in ([[2, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], [[1, 4, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], [[1, 2, 9, 8, 0, 0], [0, 0, 0, 0, 0, 0]],
               [[1, 2, 0, 0, 0, 33], [0, 0, 0, 0, 0, 0]]):
        with pytest.raises(ValueError):
            K.mix_table(np.array(mi), np.array([[0.5, 0.5], [1.0, 0.0]]), B=2, img=32, device=DEV)


# ================================================================================================ 5. the step, end to end
def drawn_plan(mode, want, B, img, classes):
    """the first seeded draw of the default recipe in `mode` that holds `want` -> MixPlan"""
    from tvts_amd.downstream.finetune_v1 import Mixup
    fn = Mixup(num_classes=classes, mode=mode, label_smoothing=0.1, **M.DEFAULT)
    state = np.random.get_state()
    try:
        for seed in range(200):
            np.random.seed(seed)
            plan = fn.draw(B, img)
            if M.holds(want, plan.mix_i):
                return plan
    finally:
        np.random.set_state(state)
    raise AssertionError(f"no seed below 200 draws '{want}' in {mode} mode")


def run_step(samples, targets, mix):
    from test_v1_finetune_gpu import F, build, stepper
    m = build(rate=0.0)
    step, _ = stepper(m, clip_grad=0.05, smoothing=0.3)  # (with a plan, the plan's smoothing is used, not this one)
    out = step.step(samples, targets, mix=mix)
    torch.cuda.synchronize()
    return dict(loss=out["loss"].reshape(1), logits=out["logits"], grad_norm=out["grad_norm"].reshape(1),
                class_acc=out["class_acc"].reshape(1), parameters=m.store.flat.clone(), exp_avg=m.store.m.clone())


@pytest.mark.parametrize("mode,want", [("batch", "all1"), ("elem", "both")])
def test_step_with_a_plan_is_the_step_on_the_host_mixed_clip(K, mode, want):
    from test_v1_finetune_gpu import F
    kw, C, B, T = S.TINY, F["classes"], 4, 8
    clip = S.synth_clip(kw, B, T, 61)
    labels = torch.randint(0, C, (B,), generator=gen(62))
    plan = drawn_plan(mode, want, B, kw["img_size"], C)
    got = run_step(clip, labels, plan)
    host = run_step(M.mix_clip(clip, plan.mix_i, plan.mix_f), M.mix_targets(labels, plan.mix_i, plan.mix_f, C, plan.smoothing), None)
    for nm in got:
        same_bytes(got[nm], host[nm], f"{mode}-mode plan, device mix vs host mix: {nm}")
    plain = run_step(clip, labels, None)
    assert not torch.equal(plain["logits"], got["logits"])  # (the plan did something)


def test_step_with_a_plan_on_uint8_frames(K):
    """uint8 frames (centre crop, normalisation and the mix on the device) against the fp32 form of the same step"""
    from test_v1_finetune_gpu import F
    kw, C, B, T = S.TINY, F["classes"], 4, 8
    img = kw["img_size"]
    fr = torch.randint(0, 256, (B, T, img + 3, img + 6, 3), generator=gen(63), dtype=torch.uint8)  # centre crop offsets 2 and 3
    mean, std = torch.tensor(MEAN).view(1, 1, 1, 1, 3), torch.tensor(STD).view(1, 1, 1, 1, 3)
    clip = ((fr[:, :, 2:2 + img, 3:3 + img].float() / 255 - mean) / std).permute(0, 4, 1, 2, 3).contiguous()
    labels = torch.randint(0, C, (B,), generator=gen(64))
    plan = drawn_plan("elem", "both", B, img, C)
    a, b = run_step(fr, labels, plan), run_step(clip, labels, plan)
    for nm in a:
        same_bytes(a[nm], b[nm], f"uint8 frames vs fp32 clip under a plan: {nm}")
