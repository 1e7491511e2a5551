"""SSv2 multiple choice, CPU side: the reference's own outputs (tests/golden/mc_b16.npz, written by tests/golden/make_golden_mc.py
from v2/downstream/model_TVTSv2_ViT_B_16_mc.py) against the oracle, the premise of the packed text encoder on the reference's side
(a caption alone, cut behind its own EOT token, gives what it gives inside a batch), and the new surface of the package."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle import tvts_oracle as O
from tvts_amd import _lib

RTOL = 1e-5  # test_oracle_golden.py: fp32 restatement against the reference
NEW_ENTRY_POINTS = ("tvts_text_embed_packed", "tvts_attn_fwd_packed", "tvts_attn_fwd_packed_last", "tvts_mc_logits")


def relerr(a, b):
    a = torch.as_tensor(np.asarray(a), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64) if not isinstance(b, torch.Tensor) else b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def fixture_and_params(golden):
    f = golden("mc_b16")
    arch = dict(O.ARCHS["B_16"], mask_ratio=0.0, sort_head=False)
    return f, arch, O.synth_params(arch, seed=int(f["seed"]))


def test_fixture_covers_the_tile_boundaries(golden):
    f = golden("mc_b16")
    B, C = int(f["B"]), int(f["C"])
    text = torch.tensor(f["text"])
    assert text.shape == (C * B, 77) and text.dtype == torch.int32 and f["label"].shape == (B,)
    lens = set((text.argmax(-1) + 1).tolist())
    assert {15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 76, 77} <= lens and min(lens) == 2
    for r in range(C * B):  # SOT first, EOT last, zeros behind
        n = int(text[r].argmax()) + 1
        assert int(text[r, 0]) == 49406 and int(text[r, n - 1]) == 49407 and not text[r, n:].any()
    # every decision of the accuracy count clears twice the GPU test's gate on the logits
    logits, label = torch.tensor(f["logits"]), torch.tensor(f["label"])
    d = (logits - logits.gather(1, label.view(-1, 1))).abs()
    d.scatter_(1, label.view(-1, 1), float("inf"))
    assert float(d.min()) > 1.0


def test_oracle_reproduces_the_reference_mc_model(fixture_and_params):
    f, arch, P = fixture_and_params
    B, T, C = int(f["B"]), int(f["T"]), int(f["C"])
    video = O.synth_batch(O.ARCHS["B_16"], B=B, T=T, seed=int(f["batch_seed"]), n_trans=1)["video"]
    with torch.no_grad():
        te = O.text_tower(P, torch.tensor(f["text"]), arch).view(C, B, -1)
        ve, _ = O.video_tower(P, video, torch.arange(196).unsqueeze(0).expand(B, -1), arch)
    assert te.shape == f["te"].shape and ve.shape == f["ve"].shape
    assert relerr(f["te"], te) < RTOL and relerr(f["ve"], ve) < RTOL, (relerr(f["te"], te), relerr(f["ve"], ve))
    # the script's arithmetic (zero_ssv2_mc_TVTSv2_ViT_B_16.py:80-88) on the stored embeddings
    t, v = torch.tensor(f["te"]), torch.tensor(f["ve"])
    t, v = t / t.norm(dim=-1, keepdim=True), v / v.norm(dim=-1, keepdim=True)
    logits = 100.0 * torch.einsum("be,cbe->bc", v, t)
    assert relerr(f["logits"], logits) < RTOL
    from tvts_amd.downstream import zero_shot as Z
    assert Z.accuracy(logits, torch.tensor(f["label"]), (1, 5)) == [float(f["acc1"]), float(f["acc5"])]


def test_a_caption_alone_is_the_caption_in_its_batch(fixture_and_params):
    """the premise of packing: rows behind a caption's EOT token do not reach its EOT row (causal mask), so the caption cut at
    its own length evaluates the same sums; what differs is the blocking of the fp32 matrix products"""
    f, arch, P = fixture_and_params
    text = torch.tensor(f["text"])
    with torch.no_grad():
        batched = O.text_tower(P, text, arch)
        for r in range(text.shape[0]):
            alone = O.text_tower(P, text[r:r + 1], arch)
            assert alone.shape == (1, arch["embed"])
            assert relerr(batched[r:r + 1], alone) < RTOL, (r, relerr(batched[r:r + 1], alone))


def test_new_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert name in protos, name
        assert hasattr(lib, name), name
    # the descriptor comes right behind the token / qkv pointers and the stream is last, like everywhere in the header
    for name in NEW_ENTRY_POINTS[:3]:
        assert "seq_start" in protos[name][2] and protos[name][2][-1] == "stream"


@pytest.mark.parametrize("name", ["B_16", "B_32", "H_14"])
def test_mc_modules_import(name):
    mod = importlib.import_module(f"tvts_amd.downstream.model_TVTSv2_ViT_{name}_mc")
    from tvts_amd.downstream._common import MCBase
    cls = getattr(mod, f"TVTSv2_{name}")
    assert issubclass(cls, MCBase) and cls.ARCH_NAME == name and callable(mod.sim_matrix)


def test_pack_captions_layout():
    from tvts_amd.model._common import pack_captions
    ids = torch.zeros(4, 10, dtype=torch.int64)
    for r, n in enumerate((5, 2, 7, 2)):
        ids[r, :n] = torch.arange(1, n + 1) + 10 * r
        ids[r, n - 1] = 99
    packed, seq_start, order, max_len = pack_captions(ids, ids.argmax(-1))
    assert order.tolist() == [1, 3, 0, 2] and seq_start.tolist() == [0, 2, 4, 9, 16] and max_len == 7
    assert packed.dtype == torch.int32 and seq_start.dtype == torch.int32
    assert packed.tolist() == [11, 99, 31, 99, 1, 2, 3, 4, 99, 21, 22, 23, 24, 25, 26, 99]
