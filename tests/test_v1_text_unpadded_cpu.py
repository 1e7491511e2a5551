"""arch["text_unpadded"] (the v1 text tower over packed captions), host side (no GPU): hip.pack_captions(lens=...) against a plain
numpy restatement, its default (the CLIP rule) unchanged on the inputs of tests/test_text_packed_cpu.py, and the refusals."""
import types

import numpy as np
import pytest
import torch

from test_text_packed_cpu import CASES, _ids, _loop
from tvts_amd import arch as A
from tvts_amd import hip as K

LENS = {
    "ragged": [13, 2, 16, 17, 1, 33, 50, 49, 80, 3],
    "all_equal": [24] * 6,
    "one": [7],
}


def _tokenizer(lens, width=None, seed=0, pad=0):
    """right-padded [N, width] ids the way a BERT tokenizer pads them ([CLS] 101 first, [SEP] 102 last, pad id behind it: the row's
    largest id says nothing about its length) and the lengths"""
    width = max(lens) if width is None else width
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lens), width), pad, dtype=torch.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = torch.randint(1000, 30000, (n,), generator=g)
        ids[r, 0] = 101
        if n > 1:
            ids[r, n - 1] = 102
    return ids, torch.tensor(lens, dtype=torch.int64)


def _restated(ids, lens, context):
    """the descriptors from plain numpy / Python loops"""
    a, lens = ids.numpy(), [int(n) for n in lens]
    flat = [int(a[r, j]) for r, n in enumerate(lens) for j in range(n)]
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos = [j for n in lens for j in range(n)]
    pos_order = sorted(range(len(pos)), key=lambda r: (pos[r], r))
    pos_seg = [sum(1 for q in pos if q < l) for l in range(context + 1)]
    return flat, starts.tolist(), pos_order, pos_seg


@pytest.mark.parametrize("width", [None, 96])
@pytest.mark.parametrize("name", list(LENS))
def test_pack_captions_by_lengths(name, width):
    lens = LENS[name]
    ids, ln = _tokenizer(lens, width, seed=len(lens))
    context = 128
    pk = K.pack_captions(ids, context, lens=ln)
    flat, starts, pos_order, pos_seg = _restated(ids, lens, context)
    M = sum(lens)
    assert pk["ids"].dtype == torch.int32 and pk["ids"].tolist() == flat
    assert pk["seq_start"].dtype == torch.int32 and pk["seq_start"].tolist() == starts
    assert pk["cls_rows"].dtype == torch.int32 and pk["cls_rows"].tolist() == starts[:-1]
    assert pk["eot_rows"].tolist() == [s - 1 for s in starts[1:]]
    assert pk["max_len"] == max(lens) and isinstance(pk["max_len"], int)
    assert pk["pos_order"].dtype == torch.int32 and pk["pos_order"].tolist() == pos_order
    assert pk["pos_seg"].dtype == torch.int32 and pk["pos_seg"].tolist() == pos_seg and pos_seg[-1] == M
    order, seg = K.token_sort(pk["ids"])
    assert torch.equal(pk["tok_order"], order) and torch.equal(pk["tok_seg"], seg)
    assert all(not t.is_cuda for t in pk.values() if torch.is_tensor(t))
    if name == "all_equal":
        assert M == len(lens) * lens[0]
    # the lengths as a list, an int32 tensor and a numpy array give the same descriptors
    for other in (lens, ln.to(torch.int32), np.asarray(lens)):
        got = K.pack_captions(ids, context, lens=other)
        assert all(torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v for k, v in pk.items())


def test_lengths_are_checked():
    ids, ln = _tokenizer([5, 9])
    with pytest.raises(ValueError, match="lens"):
        K.pack_captions(ids, lens=ln[:1])
    with pytest.raises(ValueError, match="lens"):
        K.pack_captions(ids, lens=[5, 10])      # longer than the id matrix
    with pytest.raises(ValueError, match="lens"):
        K.pack_captions(ids, lens=[0, 9])
    with pytest.raises(ValueError, match="context"):
        K.pack_captions(ids, 8, lens=ln)


@pytest.mark.parametrize("name", list(CASES))
def test_default_is_the_clip_rule_unchanged(name):
    """without `lens` the EOT token is the row's largest id: the descriptors of tests/test_text_packed_cpu.py's inputs, key by key
    (cls_rows is the one addition)"""
    lens = CASES[name]
    ids = _ids(lens, seed=len(lens))
    pk = K.pack_captions(ids)
    flat, starts = _loop(ids)
    assert pk["ids"].tolist() == flat and pk["seq_start"].tolist() == starts and pk["max_len"] == max(lens)
    assert pk["eot_rows"].tolist() == [s - 1 for s in starts[1:]] and pk["cls_rows"].tolist() == starts[:-1]
    same = K.pack_captions(ids, lens=[b - a for a, b in zip(starts, starts[1:])])
    assert set(pk) == set(same) == {"ids", "seq_start", "eot_rows", "cls_rows", "max_len", "tok_order", "tok_seg", "pos_order", "pos_seg"}
    for k, v in pk.items():
        assert torch.equal(same[k], v) if torch.is_tensor(v) else same[k] == v, k


# ------------------------------------------------------------------------------------------------ refusals
def _engine_init(a):
    """Engine.__init__'s option checks without a store or a device: the constructor reads the arch dict first"""
    from tvts_amd.engine import Engine
    eng = Engine.__new__(Engine)
    store = types.SimpleNamespace(arch=a, device=torch.device("cpu"))
    try:
        Engine.__init__(eng, store)
    except (ValueError, NotImplementedError):
        raise
    except Exception:  # whatever the constructor needs behind its option checks (buffers, a device) is not this test's subject
        pass
    return eng


def test_text_unpadded_is_refused_on_a_v2_arch():
    with pytest.raises(ValueError, match="text_packed"):
        _engine_init(dict(A.small_arch(), text_unpadded=True))
    _engine_init(dict(A.small_arch(), text_unpadded=False))  # absent or false: nothing to refuse


def test_text_packed_stays_refused_on_v1_with_its_message():
    with pytest.raises(ValueError, match="text_packed: the v1 text tower masks padded keys, it is not causal"):
        _engine_init(dict(A.small_arch_v1(), text_packed=True))
    assert _engine_init(dict(A.small_arch_v1(), text_unpadded=True)).text_unpadded is True


def test_a_caption_longer_than_80_tokens_is_refused():
    """EngineV1.prepare_batch names the limit before anything is packed or copied"""
    from tvts_amd.engine_v1 import EngineV1
    eng = EngineV1.__new__(EngineV1)
    eng.arch = dict(A.small_arch_v1(), max_pos=512)
    ids, ln = _tokenizer([81, 5])
    text = {"input_ids": ids, "attention_mask": (torch.arange(81)[None] < ln[:, None]).to(torch.int64)}
    with pytest.raises(ValueError, match="80"):
        eng._prepare_unpadded(text, dict(B=1, NT=2, S=3), 5)
    assert EngineV1.MAX_UNPADDED == 80
