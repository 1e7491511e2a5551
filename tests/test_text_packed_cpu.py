"""hip.pack_captions: the host half of the packed text tower of the training step (no GPU, no kernel library): the descriptors it
hands the kernels against a plain Python loop, and its two sort plans against their definitions."""
import numpy as np
import pytest
import torch

from tvts_amd import hip as K

CONTEXT, EOT, SOT = 77, 999, 998


def _ids(lens, seed=0, width=CONTEXT, vocab_body=50):
    """[N, width] int64 captions as clip.tokenize makes them: start token, body, end token (the row's largest id), zeros behind it.
    A small body vocabulary, so that ids repeat (runs of more than one row, and with enough captions of more than 64)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), width, dtype=torch.int64)
    for r, n in enumerate(lens):
        if n > 1:
            ids[r, 0] = SOT
            ids[r, 1:n - 1] = torch.randint(1, vocab_body, (n - 2,), generator=g)
        ids[r, n - 1] = EOT
    return ids


def _loop(ids):
    """the same descriptors from a plain Python loop"""
    flat, starts = [], [0]
    for row in ids.tolist():
        n = max(range(len(row)), key=lambda j: (row[j], -j)) + 1  # first position of the largest id (argmax)
        flat += row[:n]
        starts.append(starts[-1] + n)
    return flat, starts


CASES = {
    "len_1_and_77": [1, 77],
    "mixed": [5, 1, 77, 16, 17, 2, 33, 77, 1],
    "all_equal": [24] * 7,
    "one_caption": [9],
    "one_caption_of_1": [1],
    "many_short": [3 + i % 9 for i in range(150)],  # the start / end tokens and small body ids make runs of more than 64 rows
}


@pytest.mark.parametrize("name", list(CASES))
def test_pack_captions_descriptors(name):
    lens = CASES[name]
    ids = _ids(lens, seed=len(lens))
    pk = K.pack_captions(ids)
    flat, starts = _loop(ids)
    assert pk["ids"].dtype == torch.int32 and pk["ids"].tolist() == flat
    assert pk["seq_start"].dtype == torch.int32 and pk["seq_start"].tolist() == starts
    assert pk["eot_rows"].dtype == torch.int32 and pk["eot_rows"].tolist() == [s - 1 for s in starts[1:]]
    assert pk["max_len"] == max(lens) and isinstance(pk["max_len"], int)
    assert [b - a for a, b in zip(starts, starts[1:])] == lens
    assert all(not t.is_cuda for t in pk.values() if torch.is_tensor(t))


@pytest.mark.parametrize("name", list(CASES))
def test_token_plan_is_token_sort_of_the_packed_ids(name):
    lens = CASES[name]
    pk = K.pack_captions(_ids(lens, seed=len(lens)))
    order, seg = K.token_sort(pk["ids"])
    assert torch.equal(pk["tok_order"], order) and torch.equal(pk["tok_seg"], seg)
    M = pk["ids"].numel()
    assert pk["tok_order"].numel() == M and pk["tok_seg"].numel() == M + 1
    # and what that means: every row once, every run one id with its rows ascending
    assert sorted(pk["tok_order"].tolist()) == list(range(M))
    seg_l, ids_l, ord_l = pk["tok_seg"].tolist(), pk["ids"].tolist(), pk["tok_order"].tolist()
    seen = set()
    for a, b in zip(seg_l, seg_l[1:]):
        if a >= b:
            continue
        rows = ord_l[a:b]
        assert rows == sorted(rows) and len({ids_l[r] for r in rows}) == 1
        assert ids_l[rows[0]] not in seen  # one run per id
        seen.add(ids_l[rows[0]])
    if name == "many_short":
        runs = [b - a for a, b in zip(seg_l, seg_l[1:])]
        assert max(runs) > 64 and runs[0] > 64  # the long runs exist and come first


@pytest.mark.parametrize("name", list(CASES))
def test_position_plan_is_a_stable_grouping(name):
    lens = CASES[name]
    pk = K.pack_captions(_ids(lens, seed=len(lens)))
    M = pk["ids"].numel()
    po, ps, ss = pk["pos_order"].tolist(), pk["pos_seg"].tolist(), pk["seq_start"].tolist()
    assert pk["pos_order"].dtype == torch.int32 and pk["pos_seg"].dtype == torch.int32
    assert sorted(po) == list(range(M))  # every row once
    assert len(ps) == CONTEXT + 1 and ps[0] == 0 and ps[-1] == M and ps == sorted(ps)
    pos_of = {}
    for i in range(len(lens)):
        for r in range(ss[i], ss[i + 1]):
            pos_of[r] = r - ss[i]
    for l in range(CONTEXT):
        rows = po[ps[l]:ps[l + 1]]
        assert all(pos_of[r] == l for r in rows)
        assert rows == sorted(rows)  # stable: row order inside a position
        assert len(rows) == sum(1 for n in lens if n > l)


def test_context_smaller_than_the_id_matrix_and_the_boundary():
    """prepare_batch refuses an id matrix wider than the context before it packs (IndexError, its existing check); pack_captions holds
    the same line for callers that come another way: a caption that ENDS inside the context packs, one token more is refused."""
    ids = _ids([77, 5], width=80)
    pk = K.pack_captions(ids, context=77)
    assert pk["max_len"] == 77 and pk["pos_seg"].numel() == 78
    with pytest.raises(ValueError, match="context"):
        K.pack_captions(_ids([78, 5], width=80), context=77)
    with pytest.raises(ValueError, match="context"):
        K.pack_captions(_ids([17], width=20), context=16)
    assert K.pack_captions(_ids([16], width=20), context=16)["max_len"] == 16


def test_accepts_the_step_dtypes_and_a_non_contiguous_matrix():
    ids = _ids(CASES["mixed"])
    want = K.pack_captions(ids)
    for other in (ids.to(torch.int32), torch.cat([ids, ids], 1)[:, :CONTEXT]):
        got = K.pack_captions(other)
        for k, v in want.items():
            assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, k


def test_pack_captions_needs_no_kernel_library(monkeypatch):
    from tvts_amd import _lib

    def boom():
        raise AssertionError("pack_captions loaded the kernel library")
    monkeypatch.setattr(_lib, "load", boom)
    K.pack_captions(_ids([3, 9]))
    assert np.asarray(K.pack_captions(_ids([3, 9]))["seq_start"]).tolist() == [0, 3, 12]
