"""The forward-only encoders (TVTSv2Base.encode_video / encode_text, zero_shot.class_embeddings): against the reference's own
outputs, against the training-path forward on the same weights at the downstream geometry, their memory per clip, and their
isolation from the training step."""
import importlib
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tvts_oracle as O  # noqa: E402  (checker only)

DEV = "cuda:0"


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def cos_rows(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return torch.nn.functional.cosine_similarity(a, b, dim=1)


def _downstream(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    mod = importlib.import_module(f"tvts_amd.downstream.model_TVTSv2_ViT_{name}")
    m = getattr(mod, f"TVTSv2_{name}")(load_checkpoint=None, pretrained=False)
    m.load_state_dict(O.synth_params(dict(O.ARCHS[name], mask_ratio=0.0, sort_head=False), seed=0), strict=True)
    return m


@pytest.fixture(scope="module")
def b16():
    return _downstream("B_16")


@pytest.fixture(scope="module")
def h14():
    m = _downstream("H_14")
    yield m
    del m
    torch.cuda.empty_cache()


def test_encode_text_is_compute_text(b16, golden):
    from tvts_amd.downstream import zero_shot as Z
    f = golden("downstream_b16")
    b = O.synth_batch(O.ARCHS["B_16"], B=2, T=4, seed=int(f["batch_seed"]), n_trans=1)
    for text in (b["text"], torch.tensor(f["prompts"])):
        want, _ = b16.compute_text(text)
        got = b16.encode_text(text)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # class embeddings of prompts of different lengths, text only, against the per-class pass beside dummy frames
    g = torch.Generator().manual_seed(4)
    a = O.ARCHS["B_16"]
    classes = []
    for c, (P, cl) in enumerate(((3, 9), (2, 9), (4, 14), (1, 6))):
        ids = torch.zeros(P, a["context"], dtype=torch.int64)
        ids[:, 0] = a["vocab"] - 2
        ids[:, 1:cl - 1] = torch.randint(1, 1000, (P, cl - 2), generator=g)
        ids[:, cl - 1] = a["vocab"] - 1
        classes.append(ids)
    got = Z.class_embeddings(b16, classes)
    for c, ids in enumerate(classes):
        want = Z.class_embedding(b16, ids, 196)
        assert rel(got[c], want.cpu()) < 1e-6, (c, rel(got[c], want.cpu()))


@pytest.mark.parametrize("name,B,T,n", [("B_16", 2, 4, 196), ("B_32", 2, 5, 49), ("H_14", 1, 2, 256)])
def test_encode_video_against_reference_golden(name, B, T, n, golden, request):
    m = request.getfixturevalue(name.lower().replace("_", "")) if name != "B_32" else _downstream(name)
    f = golden("downstream_" + name.lower().replace("_", ""))
    b = O.synth_batch(O.ARCHS[name], B=B, T=T, seed=int(f["batch_seed"]), n_trans=1)
    keep = torch.arange(n).unsqueeze(0).expand(B, -1)
    ve = m.encode_video(b["video"], keep)
    _, ve_train = m({"text": b["text"], "video": b["video"], "keep_ind": keep})
    e, e_train = rel(ve, f["ve"]), rel(ve_train, f["ve"])
    assert e < 0.02 and float(cos_rows(ve, f["ve"]).min()) > 0.9995, (e, cos_rows(ve, f["ve"]))
    assert e <= 1.25 * e_train + 1e-4, (e, e_train)
    if name == "B_32":
        del m
        torch.cuda.empty_cache()


def _clips(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, 3, 224, 224, generator=g)


@pytest.mark.parametrize("name,B,n", [("B_16", 4, 196), ("H_14", 2, 256)])
def test_encode_video_against_the_training_forward_at_full_frames(name, B, n, request):
    m = request.getfixturevalue(name.lower().replace("_", ""))
    v = _clips(B, 12, seed=21)
    keep = torch.arange(n).unsqueeze(0)
    got = m.encode_video(v, keep)
    with torch.no_grad():
        _, want = m.compute_video(v, keep.expand(B, -1))
    c = cos_rows(got, want.cpu())
    print(f"\n   [{name} T=12 n={n}] worst per-clip cosine encode_video vs training forward: {float(c.min()):.7f}")
    assert float(c.min()) >= 0.9999, c


def _peak(fn, B, v):
    fn(v[:B])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn(v[:B])
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


@pytest.mark.parametrize("name,n,limit_mb", [("B_16", 196, 120), ("H_14", 256, 250)])
def test_encode_video_memory_per_clip(name, n, limit_mb, request):
    m = request.getfixturevalue(name.lower().replace("_", ""))
    v = _clips(6, 12, seed=22).to(DEV)
    keep = torch.arange(n).unsqueeze(0)
    eng = m.engine
    # workspaces only grow: start both measurements from none, B = 2 first (B = 6 then replaces every buffer it grows)
    eng._inf.clear()
    torch.cuda.empty_cache()
    p2 = _peak(lambda x: m.encode_video(x, keep), 2, v)
    enc = (_peak(lambda x: m.encode_video(x, keep), 6, v) - p2) / 4 / 1e6
    msg = f"\n   [{name} T=12 n={n}] encode_video peak growth {enc:.1f} MB per clip"
    assert enc <= limit_mb, enc
    if name == "B_16":
        def train(x):
            with torch.no_grad():
                m.compute_video(x, keep.expand(x.shape[0], -1))
        eng.buf.clear(); eng._back.clear(); eng._seen.clear()
        torch.cuda.empty_cache()
        q2 = _peak(train, 2, v)
        tr = (_peak(train, 6, v) - q2) / 4 / 1e6
        msg += f", training-path forward {tr:.1f} MB per clip"
        assert enc <= tr / 8, (enc, tr)
    print(msg)


def test_encoders_leave_the_training_step_alone():
    from tvts_amd import arch as A
    from tvts_amd.engine import LossHead
    from tvts_amd.model._common import TVTSv2Base
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    P = O.synth_params(oarch, seed=3)
    batch = O.synth_batch(oarch, B=4, T=3, seed=5, caption_len=11)
    args = types.SimpleNamespace(local_rank=0, rank=0, world_size=1)

    def step(m):
        m._fresh_shadows(); m._sync_requires_grad()
        eng = m.engine
        pb = eng.prepare_batch(batch)
        m.store.grad.zero_()
        te, ve, pred = eng.forward(pb)
        head = LossHead(m.store.device)
        l1, dv, dt = head.contrastive(ve, te)
        l2, dp = head.sorting(pred, batch["label"].reshape(-1).to(torch.int32).to(DEV))
        eng.backward(dt, dv, dp)
        torch.cuda.synchronize()
        return l1.clone(), l2.clone(), m.store.grad.clone()

    used = TVTSv2Base(args, arch=dict(a))
    used.load_state_dict(P, strict=True)
    e1 = used.encode_video(batch["video"])
    used.encode_text(batch["text"])
    used.encode_video(batch["video"][:2, :2], batch["keep_ind"][:2])
    assert torch.isfinite(e1).all() and e1.shape == (4, a["embed"])
    got = step(used)
    fresh = TVTSv2Base(args, arch=dict(a))
    fresh.load_state_dict(P, strict=True)
    want = step(fresh)
    for g, w, what in zip(got, want, ("loss1", "loss2", "gradients")):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), what
