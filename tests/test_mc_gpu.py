"""SSv2 multiple choice on the HIP engine: tvts_mc_logits against float64 torch, the _mc model classes against the reference's own
outputs (tests/golden/mc_b16.npz) and against the encoders called directly, and their isolation from the training step."""
import importlib
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tvts_oracle as O  # noqa: E402  (checker only)

DEV = "cuda:0"


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def cos_rows(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return torch.nn.functional.cosine_similarity(a, b, dim=-1)


def _mc_model(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    mod = importlib.import_module(f"tvts_amd.downstream.model_TVTSv2_ViT_{name}_mc")
    m = getattr(mod, f"TVTSv2_{name}")(load_checkpoint=None, pretrained=False)
    arch = dict(O.ARCHS[name], mask_ratio=0.0, sort_head=False)
    P = O.synth_params(arch, seed=0)
    assert list(m.state_dict().keys()) == list(P.keys())  # the downstream state dict: no pred_model.* keys, reference order
    m.load_state_dict(P, strict=True)
    return m


@pytest.mark.parametrize("C,B,E", [(174, 1, 512), (174, 16, 512), (8, 3, 512), (174, 16, 1024), (5, 2, 96)])
def test_mc_logits_against_float64(C, B, E):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd.downstream import zero_shot as Z
    g = torch.Generator(device=DEV).manual_seed(C + B + E)
    t = torch.randn(C, B, E, generator=g, device=DEV) * 3.0
    v = torch.randn(B, E, generator=g, device=DEV) * 0.2
    got = Z.mc_logits(t, v)
    assert got.shape == (B, C) and got.dtype == torch.float32
    td, vd = t.double(), v.double()
    want = 100.0 * torch.einsum("be,cbe->bc", vd / vd.norm(dim=-1, keepdim=True), td / td.norm(dim=-1, keepdim=True))
    assert rel(got, want) < 1e-5, rel(got, want)
    assert torch.equal(Z.mc_logits(t, v).view(torch.int32), got.view(torch.int32))
    with pytest.raises(ValueError):
        Z.mc_logits(t, v[:, :-1])


def test_mc_b16_against_reference_golden(golden):
    from tvts_amd.downstream import zero_shot as Z
    f = golden("mc_b16")
    B, T, C = int(f["B"]), int(f["T"]), int(f["C"])
    m = _mc_model("B_16")
    video = O.synth_batch(O.ARCHS["B_16"], B=B, T=T, seed=int(f["batch_seed"]), n_trans=1)["video"]
    data = {"text": torch.tensor(f["text"]), "video": video, "keep_ind": torch.arange(196).unsqueeze(0).expand(B, -1)}
    te, ve = m(data, return_embeds=True)
    assert te.shape == (C, B, 512) and ve.shape == (B, 512)
    et, ev = rel(te, f["te"]), rel(ve, f["ve"])
    ct, cv = float(cos_rows(te, f["te"]).min()), float(cos_rows(ve, f["ve"]).min())
    logits = Z.mc_logits(te, ve)
    dl = float((logits.cpu() - torch.tensor(f["logits"])).abs().max())
    print(f"mc B_16: te rel {et:.3e} cos {ct:.6f} | ve rel {ev:.3e} cos {cv:.6f} | max |logits - golden| {dl:.4f}")
    assert et < 0.02 and ev < 0.02 and ct > 0.9995 and cv > 0.9995, (et, ev, ct, cv)
    assert dl < 0.5, dl
    label = torch.tensor(f["label"]).to(DEV)
    assert Z.accuracy(logits, label, (1, 5)) == [float(f["acc1"]), float(f["acc5"])]
    with pytest.raises(ValueError):
        m(data, return_embeds=False)
    with pytest.raises(ValueError):
        m(dict(data, text=data["text"][:-1]), return_embeds=True)
    assert all(not p.requires_grad for p in m.parameters())


@pytest.mark.parametrize("name,n", [("B_32", 49), ("H_14", 256)])
def test_mc_other_archs(name, n):
    m = _mc_model(name)
    a = O.ARCHS[name]
    B, T, C = 2, 2, 5
    video = O.synth_batch(a, B=B, T=T, seed=8, n_trans=1)["video"]
    g = torch.Generator().manual_seed(9)
    text = torch.zeros(C * B, a["context"], dtype=torch.int32)
    for r, ln in enumerate((4, 40, 17, 9, 33, 77, 16, 2, 25, 12)):
        text[r, 0] = a["vocab"] - 2
        text[r, 1:ln - 1] = torch.randint(1, 1000, (max(ln - 2, 0),), generator=g, dtype=torch.int32)
        text[r, ln - 1] = a["vocab"] - 1
    keep = torch.arange(n).unsqueeze(0).expand(B, -1)
    te, ve = m({"text": text, "video": video, "keep_ind": keep})
    assert te.shape == (C, B, a["embed"]) and ve.shape == (B, a["embed"])
    assert bool(torch.isfinite(te).all()) and bool(torch.isfinite(ve).all())
    want_t = m.encode_text(text, packed=True).view(C, B, -1)
    want_v = m.encode_video(video, keep)
    assert torch.equal(te.view(torch.int32), want_t.view(torch.int32)) and torch.equal(ve.view(torch.int32), want_v.view(torch.int32))
    del m
    torch.cuda.empty_cache()


def test_mc_forward_leaves_the_training_step_alone():
    """test_infer_gpu.py::test_encoders_leave_the_training_step_alone for the packed encoder: a training step before and after a
    multiple-choice forward (its two encoder calls) on the same model gives the same bits."""
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

    m = TVTSv2Base(args, arch=dict(a))
    m.load_state_dict(P, strict=True)
    before = step(m)
    ragged = batch["text"].clone()  # 16 captions of 11 tokens: cut some of them shorter
    for r, n in enumerate((3, 11, 7, 2, 9, 11, 5, 8)):
        ragged[r, n - 1] = a["vocab"] - 1
        ragged[r, n:] = 0
    ve = m.encode_video(batch["video"])
    te = m.encode_text(ragged, packed=True)
    assert te.shape == (16, a["embed"]) and bool(torch.isfinite(te).all()) and bool(torch.isfinite(ve).all())
    with torch.no_grad():
        want = O.text_tower({k: v for k, v in P.items() if k.startswith("text_")}, ragged, oarch)
    assert rel(te, want) < 0.02, rel(te, want)
    after = step(m)
    for g, w, what in zip(after, before, ("loss1", "loss2", "gradients")):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), what
