"""The packed variable-length text encoder: its kernels (tvts_text_embed_packed, tvts_attn_fwd_packed and its last-row form) against
torch / float64 torch per sequence, and TVTSv2Base.encode_text(packed=True) / zero_shot.class_embeddings(packed=True) against the
oracle and against the rectangular pass on the same captions."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402
from oracle import tvts_oracle as O  # noqa: E402  (checker only)

DEV = "cuda:0"
OUT_TOL = 7e-3  # test_kernels_gpu.py ATTN_ROW_TOL["out"], as test_attn_infer_gpu.py
EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 76, 77]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def _rand_lens(n, lo, hi, seed):
    return torch.randint(lo, hi + 1, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def _shuffled(lens, seed):
    return [lens[i] for i in torch.randperm(len(lens), generator=torch.Generator().manual_seed(seed)).tolist()]


LENGTH_SETS = {
    "edges_sorted": sorted(EDGES),
    "edges_unsorted": _shuffled(EDGES * 3, 1),
    "edges_descending": sorted(EDGES, reverse=True),
    "all_equal_24": [24] * 50,
    "all_equal_77": [77] * 9,
    "all_equal_1": [1] * 7,
    "one_of_1": [1],
    "one_of_20": [20],
    "one_of_77": [77],
    "ssv2_like_sorted_2784": sorted(_rand_lens(2784, 6, 24, 2)),
    "any_unsorted_3000": _rand_lens(3000, 1, 77, 3),
}


def _seq_start(lens):
    s = torch.zeros(len(lens) + 1, dtype=torch.int32)
    s[1:] = torch.tensor(lens).cumsum(0)
    return s.to(DEV)


def _ref_packed(qkv, lens, heads):
    """float64 causal softmax attention inside every sequence (sequences of one length evaluated together) -> [M, W]"""
    M, W = qkv.shape[0], qkv.shape[1] // 3
    dh = W // heads
    lt = torch.tensor(lens, device=DEV)
    start = torch.cumsum(lt, 0) - lt
    ref = torch.empty(M, W, dtype=torch.float64, device=DEV)
    for L in sorted(set(lens)):
        rows = (start[lt == L].view(-1, 1) + torch.arange(L, device=DEV)).reshape(-1)
        x = qkv[rows].double().view(-1, L, 3, heads, dh).permute(2, 0, 3, 1, 4)  # [3, n, heads, L, dh]
        s = x[0] @ x[1].transpose(-1, -2) / dh ** 0.5
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
        ref[rows] = (torch.softmax(s, -1) @ x[2]).permute(0, 2, 1, 3).reshape(-1, W)
    return ref


@pytest.mark.parametrize("heads", [8, 16])
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_attn_fwd_packed(K, name, heads):
    lens = LENGTH_SETS[name]
    N, M, W = len(lens), sum(lens), heads * 64
    qkv = torch.randn(M, 3 * W, generator=torch.Generator(device=DEV).manual_seed(N + heads), device=DEV).bfloat16()
    ss = _seq_start(lens)
    ref = _ref_packed(qkv, lens, heads)
    outs = []
    for _ in range(2):
        buf, out = KB.guarded(M, W, torch.bfloat16, DEV)
        K.attn_fwd_packed(qkv, ss, out, N=N, heads=heads, max_len=max(lens))
        torch.cuda.synchronize()
        KB.check_guards(buf, M, W, "packed attention out")
        outs.append(out)
    what = f"packed attention [{name}, {heads} heads]"
    worst = KB.assert_rows_within(outs[0], ref, OUT_TOL, groups=heads, what=what, out_dtype=torch.bfloat16)
    print(f"{what}: worst per-(row, head) relative error {worst:.3e} (gate {OUT_TOL})")
    KB.assert_equal_bits(outs[1], outs[0], what + ": second run")
    # a max_len above the longest sequence launches more tile classes and changes nothing
    if max(lens) <= 48:
        buf, out = KB.guarded(M, W, torch.bfloat16, DEV)
        K.attn_fwd_packed(qkv, ss, out, N=N, heads=heads, max_len=77)
        torch.cuda.synchronize()
        KB.assert_equal_bits(out, outs[0], what + ": max_len 77")


@pytest.mark.parametrize("heads", [8, 16])
@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_attn_fwd_packed_last_row(K, name, heads):
    lens = LENGTH_SETS[name]
    N, M, W = len(lens), sum(lens), heads * 64
    qkv = torch.randn(M, 3 * W, generator=torch.Generator(device=DEV).manual_seed(7 * N + heads), device=DEV).bfloat16()
    ss = _seq_start(lens)
    last = (ss[1:] - 1).long()
    ref = _ref_packed(qkv, lens, heads)[last]
    outs = []
    for _ in range(2):
        buf, out = KB.guarded(M, W, torch.bfloat16, DEV)
        K.attn_fwd_packed(qkv, ss, out, N=N, heads=heads, max_len=max(lens), last_only=True)
        torch.cuda.synchronize()
        KB.check_guards(buf, M, W, "packed last-row attention out")
        outs.append(out)
    what = f"packed last-row attention [{name}, {heads} heads]"
    worst = KB.assert_rows_within(outs[0][last], ref, OUT_TOL, groups=heads, what=what, out_dtype=torch.bfloat16)
    print(f"{what}: worst per-(row, head) relative error {worst:.3e} (gate {OUT_TOL})")
    other = torch.ones(M, dtype=torch.bool, device=DEV)
    other[last] = False
    assert bool(torch.isnan(outs[0][other]).all()), what + ": a row that is no sequence's last one was written"
    KB.assert_equal_bits(outs[1], outs[0], what + ": second run")


def test_attn_fwd_packed_refuses_long_sequences(K):
    lens = [81, 4]
    qkv = torch.zeros(sum(lens), 3 * 128, device=DEV).bfloat16()
    out = torch.zeros(sum(lens), 128, device=DEV).bfloat16()
    for last_only in (False, True):
        with pytest.raises(K.HipError, match="-22"):
            K.attn_fwd_packed(qkv, _seq_start(lens), out, N=2, heads=2, max_len=81, last_only=last_only)


@pytest.mark.parametrize("name", ["edges_unsorted", "all_equal_24", "one_of_77", "ssv2_like_sorted_2784"])
@pytest.mark.parametrize("Wt", [512, 1024])
def test_text_embed_packed(K, name, Wt):
    lens = LENGTH_SETS[name]
    N, M, vocab = len(lens), sum(lens), 1000
    g = torch.Generator(device=DEV).manual_seed(M + Wt)
    emb = torch.randn(vocab, Wt, generator=g, device=DEV)
    pos = torch.randn(77, Wt, generator=g, device=DEV)
    ids = torch.randint(0, vocab, (M,), generator=g, device=DEV, dtype=torch.int32)
    p = torch.cat([torch.arange(n) for n in lens]).to(DEV)
    buf, x = KB.guarded(M, Wt, torch.float32, DEV)
    K.text_embed_packed(ids, _seq_start(lens), emb, pos, x, N=N)
    torch.cuda.synchronize()
    KB.check_guards(buf, M, Wt, "packed text embedding")
    KB.assert_equal_bits(x.contiguous(), emb[ids.long()] + pos[p], f"packed text embedding [{name}, {Wt}]")


# ------------------------------------------------------------------------------------------------ the encoder
def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def cos_rows(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return torch.nn.functional.cosine_similarity(a, b, dim=1)


def _captions(arch, lens, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), arch["context"], dtype=torch.int64)
    for r, n in enumerate(lens):
        ids[r, 0] = arch["vocab"] - 2
        if n > 2:
            ids[r, 1:n - 1] = torch.randint(1, arch["vocab"] - 408, (n - 2,), generator=g)
        ids[r, n - 1] = arch["vocab"] - 1
    return ids


@pytest.fixture(scope="module", params=["B_16", "H_14"])
def model_and_params(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    name = request.param
    mod = importlib.import_module(f"tvts_amd.downstream.model_TVTSv2_ViT_{name}")
    m = getattr(mod, f"TVTSv2_{name}")(load_checkpoint=None, pretrained=False)
    arch = dict(O.ARCHS[name], mask_ratio=0.0, sort_head=False)
    P = O.synth_params(arch, seed=0)
    m.load_state_dict(P, strict=True)
    P = {k: v for k, v in P.items() if k.startswith("text_")}
    yield name, m, arch, P
    del m
    torch.cuda.empty_cache()


RAGGED = {"both_sides_of_32": [5, 12, 31, 32, 33, 40, 77, 20, 2, 16, 17], "short": [6, 9, 24, 13, 7, 18],
          "all_equal_16": [16] * 6, "one_caption": [9]}


@pytest.mark.parametrize("batch", list(RAGGED))
def test_encode_text_packed_against_the_oracle(model_and_params, batch):
    name, m, arch, P = model_and_params
    ids = _captions(arch, RAGGED[batch], seed=len(batch))
    with torch.no_grad():
        want = O.text_tower(P, ids, arch)
    got = m.encode_text(ids, packed=True)
    rect = m.encode_text(ids)
    assert got.shape == want.shape == rect.shape
    e, c = rel(got, want), float(cos_rows(got, want).min())
    er, cr = rel(rect, want), float(cos_rows(rect, want).min())
    print(f"encode_text [{name}, {batch}]: packed rel {e:.3e} cos {c:.6f} | rectangular rel {er:.3e} cos {cr:.6f}")
    assert e < 0.02 and c > 0.9995, (e, c)
    again = m.encode_text(ids, packed=True)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


def test_encode_text_packed_validates_like_encode_text(model_and_params):
    name, m, arch, P = model_and_params
    with pytest.raises(ValueError):
        m.encode_text(torch.zeros(0, 77, dtype=torch.int64), packed=True)
    with pytest.raises(IndexError):
        m.encode_text(torch.full((2, 77), arch["vocab"], dtype=torch.int64), packed=True)


def test_class_embeddings_packed(model_and_params):
    from tvts_amd.downstream import zero_shot as Z
    name, m, arch, P = model_and_params
    classes = [_captions(arch, [cl] * n, seed=10 + c) for c, (n, cl) in enumerate(((3, 9), (2, 9), (4, 14), (1, 6), (2, 35)))]
    want = Z.class_embeddings(m, classes)
    got = Z.class_embeddings(m, classes, packed=True)
    assert got.shape == want.shape
    for c in range(len(classes)):
        assert rel(got[c], want[c].cpu()) < 0.02, (c, rel(got[c], want[c].cpu()))
