"""RandAugment of the v1 fine-tuning recipe, host side: the draw (tvts_amd.downstream.finetune_v1.RandAugment), the plan tables and
the numpy restatement of the operations (tests/v1_randaug_ref.py) against the reference's own run under PIL
(tests/golden/v1_randaug.npz, written by tests/golden/make_golden_v1_randaug.py).  Everything is compared bit for bit."""
import json
import os
import random

import numpy as np
import pytest

import v1_randaug_ref as R
from tvts_amd import hip
from tvts_amd.downstream import finetune_v1 as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "v1_randaug.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def op_cases(gold):
    for k, (fn, arg, rs) in enumerate(zip(gold["op.fn"], gold["op.arg"], gold["op.resample"])):
        yield k, str(fn), None if np.isnan(arg) else float(arg), int(rs)


def chain(gold, k):
    Bs, ns, T, H, W = (int(v) for v in gold["chain.shape"])
    return dict(cfg=str(gold[f"chain.{k}.cfg"]), interp=str(gold[f"chain.{k}.interp"]), seed=int(gold[f"chain.{k}.seed"]),
                frames=gold[f"chain.{k}.frames"], views=gold[f"chain.{k}.views"], rec=json.loads(str(gold[f"chain.{k}.rec"])),
                next_random=float(gold[f"chain.{k}.next_random"]), next_uniform=float(gold[f"chain.{k}.next_uniform"]),
                Bs=Bs, ns=ns, T=T, H=H, W=W)


def test_fixture_holds_what_the_tests_rely_on(gold):
    fns = {fn for _, fn, _, _ in op_cases(gold)}
    assert len(fns) == 15
    cases = {(fn, arg) for _, fn, arg, _ in op_cases(gold)}
    assert {("posterize", 0.0), ("posterize", 8.0), ("solarize", 0.0), ("solarize", 256.0)} <= cases
    for fn in ("rotate", "shear_x", "shear_y", "translate_x_rel", "translate_y_rel"):
        got = {(arg > 0, rs) for _, f, arg, rs in op_cases(gold) if f == fn}
        assert {s for s, _ in got} == {True, False} and {r for _, r in got} == {2, 3}, fn
    assert gold["op.frame_a"].shape == (19, 27, 3) and gold["op.frame_b"].shape == (40, 70, 3)
    recs = [v for k in range(int(gold["chain.n"])) for v in chain(gold, k)["rec"]]
    assert {n for v in recs for n, _, _ in v} == fns
    assert {0, 4} <= {len(v) for v in recs}
    assert any(len({n for n, _, _ in v}) < len(v) for v in recs)


def test_restatement_reproduces_every_op_frame(gold):
    for k, fn, arg, rs in op_cases(gold):
        for fr, want in ((gold["op.frame_a"], gold["op.out_a"][k]), (gold["op.frame_b"], gold["op.out_b"][k])):
            got = R.apply_named(fr, fn, arg, rs)
            assert np.array_equal(got, want), (fn, arg, rs, fr.shape, int((got != want).sum()))


def test_posterize_to_8_bits_is_no_op_row():
    ri, _ = F.ra_row("posterize", 8, 0, 19, 27)
    assert ri[0] == F.RA_NONE


@pytest.mark.parametrize("k", [0, 1, 2])
def test_draw_and_restatement_reproduce_the_chain(gold, k):
    """under the fixture's seed the draw names the reference's op functions, arguments and resample per view, leaves `random` and
    `np.random` where the reference left them, and the restatement run over the plan gives the reference's frames"""
    c = chain(gold, k)
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    plan = F.RandAugment(c["cfg"], interpolation=c["interp"]).draw(c["Bs"] * c["ns"], c["H"], c["W"], num_sample=c["ns"])
    assert random.random() == c["next_random"] and float(np.random.uniform()) == c["next_uniform"]
    geo = ("rotate", "shear_x", "shear_y", "translate_x_rel", "translate_y_rel")
    got = [[[n, None if a is None else float(a), r if n in geo else 0] for n, a, r in view] for view in plan.ops]
    assert got == c["rec"]
    ri, rd = hip.check_randaug_plan(plan.ra_i, plan.ra_d, B=c["Bs"] * c["ns"])
    assert [int((row[:, 0] != 0).sum()) for row in ri] == [len(v) for v in c["rec"]]
    views = R.apply_plan(c["frames"], ri, rd, c["ns"])
    assert np.array_equal(views, c["views"]), int((views != c["views"]).sum())


def test_config_parity_points():
    inc0, inc1, plain = F.RandAugment("rand-m10-n3-inc0"), F.RandAugment("rand-m7-n4-mstd0.5-inc1"), F.RandAugment("rand-m9-n2-w0")
    assert inc0.increasing and inc1.increasing and not plain.increasing  # bool("0") is true
    assert (inc1.magnitude, inc1.num_layers, inc1.magnitude_std, inc1.weights) == (7, 4, 0.5, None)
    w = dict(zip([o[0] for o in F._RA_OPS], plain.weights))
    assert abs(sum(plain.weights) - 1) < 1e-12 and w["posterize"] == 0 and w["invert"] == 0 and w["rotate"] == 0.3 / sum(F._RA_WEIGHTS_0)
    d = F.RandAugment("rand")
    assert (d.magnitude, d.num_layers, d.magnitude_std) == (10.0, 2, 0)
    # translate: pct * W0 in x, pct * H0 in y; rotate: PIL's matrix about (W0 / 2, H0 / 2)
    assert F.ra_row("translate_x_rel", 0.25, 2, 20, 40)[1][:6] == (1.0, 0.0, 10.0, 0.0, 1.0, 0.0)
    assert F.ra_row("translate_y_rel", 0.25, 3, 20, 40)[1][:6] == (1.0, 0.0, 0.0, 0.0, 1.0, 5.0)
    a, b, c_, d_, e, f = F.ra_row("rotate", 90.0, 3, 20, 40)[1][:6]
    assert (a, b, d_, e) == (0.0, -1.0, 1.0, 0.0) and (c_, f) == (0.0 * -20 + -1.0 * -10 + 0.0 + 20, 1.0 * -20 + 0.0 * -10 + 0.0 + 10)


def test_augment_interleaves_randaug_with_crop_and_erase():
    """per view: the RandAugment draws, then crop, flip and erase -- the order ssv2.py:174-227 draws in"""
    kw = dict(hflip=0.5, reprob=0.5, remode="pixel", noise_seed=5)
    H0, W0, Bs, ns = 37, 53, 3, 2
    random.seed(11)
    np.random.seed(11)
    plan = F.Augment(32, num_sample=ns, randaug=F.RandAugment("rand-m7-n4-mstd0.5-inc1"), **kw).draw(Bs, H0, W0)
    after = (random.random(), np.random.uniform())
    random.seed(11)
    np.random.seed(11)
    ra, one = F.RandAugment("rand-m7-n4-mstd0.5-inc1"), F.Augment(32, num_sample=1, **kw)
    views, rows = [], []
    for b in range(Bs * ns):
        views.append(ra.draw_view(H0, W0))
        rows.append(one.draw(1, H0, W0).aug_i[0])
    assert (random.random(), np.random.uniform()) == after
    want = F.ra_plan(views, 4, ns)
    assert np.array_equal(plan.ra.ra_i, want.ra_i) and np.array_equal(plan.ra.ra_d, want.ra_d) and plan.ra.num_sample == ns
    assert np.array_equal(plan.aug_i[:, 1:], np.stack(rows)[:, 1:]) and list(plan.aug_i[:, 0]) == [0, 0, 1, 1, 2, 2]
    assert plan.ra.ra_i.shape == (6, 4, 4) and plan.ra.ra_d.shape == (6, 4, 8) and plan.ra.ra_d.dtype == np.float64
    assert any(len(v) for v in plan.ra.ops)


def test_plans_without_randaug_are_unchanged():
    random.seed(3)
    np.random.seed(3)
    p = F.Augment(32, num_sample=2).draw(2, 37, 53)
    assert p.ra is None and F.AugPlan(p.aug_i).ra is None and len(F.AugPlan(p.aug_i)) == 4


def test_refusals():
    with pytest.raises(ValueError):
        F.RandAugment("rand-m7-n4", interpolation="random")
    for interp in ("lanczos", "nearest", "hamming"):
        with pytest.raises(ValueError):
            F.RandAugment("rand-m7-n4", interpolation=interp)
    with pytest.raises(ValueError):
        F.RandAugment("rand-m7-n9")
    for cfg in ("augmix-m5", "original", ""):
        with pytest.raises(ValueError):
            F.RandAugment(cfg)
    ra = F.RandAugment("rand-m7-n8")
    for hw in ((2, 30), (30, 2)):
        with pytest.raises(ValueError):
            ra.draw(1, *hw)
        with pytest.raises(ValueError):
            F.Augment(32, randaug=ra).draw(1, *hw)
    assert F.RandAugment("rand-m7-n8").draw(1, 3, 3).ra_i.shape == (1, 8, 4)


def test_check_randaug_plan_refuses_every_bad_column():
    random.seed(1)
    np.random.seed(1)
    good = F.RandAugment("rand-m7-n4-mstd0.5-inc1").draw(4, 19, 27, num_sample=2)
    ri, rd = hip.check_randaug_plan(good.ra_i, good.ra_d, B=4)
    assert ri.dtype == np.int32 and rd.dtype == np.float64 and ri.flags.c_contiguous and rd.flags.c_contiguous

    def bad(i=None, d=None, **kw):
        bi, bd = good.ra_i.copy(), good.ra_d.copy()
        if i:
            bi[i[0]] = i[1]
        if d:
            bd[d[0]] = d[1]
        with pytest.raises(ValueError):
            hip.check_randaug_plan(kw.get("ri", bi), kw.get("rd", bd), B=kw.get("B", 4))
    row = lambda *v: np.array(v)  # noqa: E731
    bad(i=((0, 0), row(12, 0, 0, 0)))
    bad(i=((0, 0), row(-1, 0, 0, 0)))
    bad(i=((0, 0), row(11, 1, 0, 0)))
    bad(i=((0, 0), row(3, 2, 0, 0)))
    bad(i=((0, 0), row(4, 0, 257, 0)))
    bad(i=((0, 0), row(6, 0, 8, 0)))
    bad(i=((0, 0), row(5, 0, -1, 0)))
    bad(i=((0, 0), row(7, 0, 3, 0)))
    bad(i=((0, 0), row(3, 0, 0, 1)))
    bad(i=((0, slice(0, 2)), np.array([[0, 0, 0, 0], [3, 0, 0, 0]])))  # an op behind an empty slot
    bad(d=((0, 0, 6), np.nan))
    bad(d=((1, 1, 2), np.inf))
    bad(d=((0, 0, 7), 1.0))
    bad(B=5)
    bad(ri=good.ra_i.astype(np.float32))
    bad(rd=good.ra_d[:, :3])
    bad(ri=np.zeros((4, 9, 4), dtype=np.int32), rd=np.zeros((4, 9, 8)))
    with pytest.raises(ValueError):  # raised before anything touches a device
        hip.RandaugTable(good.ra_i[:3], good.ra_d[:3], Bs=2, num_sample=2, device="cuda")


def test_final_rows_of_a_plan():
    ri = np.zeros((4, 3, 4), dtype=np.int32)
    ri[1, :1, 0] = ri[2, :2, 0] = ri[3, :3, 0] = 3
    assert list(hip.randaug_rows(ri, Bs=2, num_sample=2)) == [0, 2 + 1, 2 + 4 + 2, 2 + 3]


def test_restatement_against_pil_on_fresh_frames():
    """a property test where PIL imports: every op at drawn arguments on frames of drawn sizes, the restatement against PIL itself"""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageOps
    rng = np.random.RandomState(77)
    fill = dict(fillcolor=(128, 128, 128))

    def pil(fn, im, arg, rs):
        if fn == "auto_contrast":
            return ImageOps.autocontrast(im)
        if fn == "equalize":
            return ImageOps.equalize(im)
        if fn == "invert":
            return ImageOps.invert(im)
        if fn == "solarize":
            return ImageOps.solarize(im, arg)
        if fn == "solarize_add":
            return im.point([min(255, i + arg) if i < 128 else i for i in range(256)] * 3)
        if fn == "posterize":
            return im if arg >= 8 else ImageOps.posterize(im, arg)
        if fn in ("color", "contrast", "brightness", "sharpness"):
            return getattr(ImageEnhance, fn.capitalize())(im).enhance(arg)
        if fn == "rotate":
            return im.rotate(arg, resample=rs, **fill)
        w, h = im.size
        data = {"shear_x": (1, arg, 0, 0, 1, 0), "shear_y": (1, 0, 0, arg, 1, 0), "translate_x_rel": (1, 0, arg * w, 0, 1, 0),
                "translate_y_rel": (1, 0, 0, 0, 1, arg * h)}[fn]
        return im.transform(im.size, Image.AFFINE, data, resample=rs, **fill)
    for trial in range(40):
        H, W = int(rng.randint(3, 34)), int(rng.randint(3, 50))
        fr = R.case_frames(500 + trial, 1, H, W)[0] if trial % 2 else rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        if trial % 7 == 0:
            fr[:] = fr[0, 0]  # a constant frame
        for fn, rule, _ in F._RA_OPS:
            rs = int(rng.choice([2, 3]))
            arg = {None: None, "rotate": rng.uniform(-30, 30), "enhance": rng.uniform(0.1, 1.9), "shear": rng.uniform(-0.3, 0.3),
                   "translate_rel": rng.uniform(-0.45, 0.45), "posterize": int(rng.randint(0, 9)), "solarize": int(rng.randint(0, 257)),
                   "solarize_add": int(rng.randint(0, 111))}[rule]
            want = np.asarray(pil(fn, Image.fromarray(fr), arg, rs))
            got = R.apply_named(fr, fn, arg, rs)
            assert np.array_equal(got, want), (fn, arg, rs, H, W, int((got != want).sum()))
