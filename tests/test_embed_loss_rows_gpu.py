"""Per-element checks of the kernels around the stacks (run with -m gpu): embed.hip (patch gathers, token assembles, the text
embedding, the caption mean, the sort-head input and all their backwards), loss.hip (l2norm_rows, InfoNCE, cross entropy) and the
AdamW kernel of optim.hip, at the launch edges their one-shape whole-tensor tests never reached.

Exact outputs (gathers, one fp32 add, a bf16 rounding) are compared bit for bit with torch doing the same fp32 operations in the
same order.  Ordered sums are held per element to kernel_bounds.sum_bound against float64, start from non-zero accumulators (every
kernel here adds into its output) and must give the same bits on a second run.  The losses and AdamW are held to the bounds derived
in kernel_bounds (l2norm_check, infonce_check, ce_check, adamw_check).  Outputs live in guarded buffers (NaN rows under them, NaN
columns right of them where the entry point takes a leading dimension).  Every case prints its worst |err| / bound ("BOUND" lines)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_bounds as KB  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16
F32 = torch.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed, scale=1.0):
    """fp32 N(0, scale^2) drawn on the host: the same values on every machine"""
    return torch.randn(*shape, generator=gen(seed)) * scale


def wide(t, pad=4):
    """a device copy of the 2-D t as a view of a wider NaN-filled matrix: leading dimension = columns + pad"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def guarded_from(t, cols=8):
    """(buffer, view) of KB.guarded holding t: a non-zero accumulator with guard rows (and columns) around it"""
    t2 = t if t.dim() == 2 else t[None, :]
    buf, view = KB.guarded(t2.shape[0], t2.shape[1], t.dtype, DEV, cols=cols)
    view.copy_(t2.to(DEV))
    return buf, (view if t.dim() == 2 else view[0])


def guards_ok(buf, t, what):
    t2 = t if t.dim() == 2 else t[None, :]
    KB.check_guards(buf, t2.shape[0], t2.shape[1], what)


def keep_lists(rows, n, ppf, seed, first_last=True):
    """int32 [rows, n]: unsorted distinct patch indices per row; row 0 holds the last and the first index (in that order)"""
    g = gen(seed)
    k = torch.stack([torch.randperm(ppf, generator=g)[:n] for _ in range(rows)])
    if first_last and n >= 2:
        rest = [i for i in torch.randperm(ppf, generator=g).tolist() if i not in (0, ppf - 1)][:n - 2]
        k[0] = torch.tensor([ppf - 1, 0] + rest)
    return k.to(torch.int32)


# ================================================================================================ 2. exact outputs
@pytest.mark.parametrize("p,img,B,T,n,ldo", [(16, 32, 2, 2, 3, 768), (32, 64, 1, 2, 3, 3072), (8, 32, 2, 2, 3, 192), (14, 56, 2, 2, 3, 640)],
                         ids=["p16", "p32_two_trips", "p8_24_threads", "p14_any_padded"])
def test_patch_gather_bits(K, p, img, B, T, n, ldo):
    """the vector kernel at one trip (p 16), two trips of c8 += 2048 (p 32, K 3072) and 24 busy threads (p 8), the any-patch kernel
    with zero pad columns (p 14, ldo 640); unsorted keep lists holding the first and the last patch index"""
    g = img // p
    Kc = 3 * p * p
    video = rnd(B, T, 3, img, img, seed=p)
    keep = keep_lists(B, n, g * g, seed=100 + p)
    M = B * T * n
    buf, out = KB.guarded(M, ldo, BF16, DEV, cols=0)  # the row stride IS the width here (the vector path asks for it)
    K.patch_gather(video.to(DEV), keep.to(DEV), out, B=B, T=T, n=n, img=img, patch=p)
    pix = video.reshape(B, T, 3, g, p, g, p).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, T, g * g, Kc)
    ref = torch.gather(pix, 2, keep.long()[:, None, :, None].expand(B, T, n, Kc)).reshape(M, Kc).bfloat16()
    want = torch.zeros(M, ldo, dtype=BF16)
    want[:, :Kc] = ref
    KB.assert_equal_bits(out.cpu(), want, f"patch_gather p={p}")
    KB.check_guards(buf, M, ldo, f"patch_gather p={p}")


def test_patch_gather_tube_bits(K):
    """tubelet 2, p 16: columns in (c, t, py, px) order, one keep list per tube"""
    B, tubes, tb, n, img, p = 2, 2, 2, 3, 32, 16
    g, Kc = img // p, 3 * tb * p * p
    video = rnd(B, tubes * tb, 3, img, img, seed=7)
    keep = keep_lists(B * tubes, n, g * g, seed=8).view(B, tubes, n)
    M = B * tubes * n
    buf, out = KB.guarded(M, Kc, BF16, DEV, cols=0)
    K.patch_gather_tube(video.to(DEV), keep.to(DEV), out, B=B, tubes=tubes, tubelet=tb, n=n, img=img, patch=p)
    pix = video.reshape(B, tubes, tb, 3, g, p, g, p).permute(0, 1, 4, 6, 3, 2, 5, 7).reshape(B, tubes, g * g, Kc)
    ref = torch.gather(pix, 2, keep.long()[..., None].expand(B, tubes, n, Kc)).reshape(M, Kc).bfloat16()
    KB.assert_equal_bits(out.cpu(), ref, "patch_gather_tube")
    KB.check_guards(buf, M, Kc, "patch_gather_tube")


@pytest.mark.parametrize("per_frame", [False, True], ids=["keep_Bn", "keep_BTn"])
@pytest.mark.parametrize("W", [4, 260, 1028])
def test_vit_assemble_bits(K, W, per_frame):
    """(patch + pos[1 + keep]) + temporal[f] and cls + pos[0], fp32, in that order; one thread (W 4), a ragged first trip (260), a
    second trip of c += 1024 (1028); the patch matrix has ldp > W, the tokens ldt > W"""
    B, T, n, ppf = 2, 3, 5, 12
    patch, cls, pos, tmp = rnd(B * T * n, W, seed=1), rnd(W, seed=2), rnd(ppf + 1, W, seed=3), rnd(T + 1, W, seed=4)
    keep = keep_lists(B * T if per_frame else B, n, ppf, seed=5)
    keep = keep.view(B, T, n) if per_frame else keep
    S = 1 + T * n
    buf, tok = KB.guarded(B * S, W, F32, DEV)
    K.vit_assemble(wide(patch), cls.to(DEV), pos.to(DEV), tmp.to(DEV), keep.to(DEV), tok, B=B, T=T, n=n)
    kp = keep.long() if per_frame else keep.long()[:, None, :].expand(B, T, n)
    body = (patch.view(B, T, n, W) + pos[1 + kp]) + tmp[:T][None, :, None, :]
    want = torch.cat([(cls + pos[0]).expand(B, 1, W), body.reshape(B, T * n, W)], 1).reshape(B * S, W)
    KB.assert_equal_bits(tok.cpu(), want, f"vit_assemble W={W}")
    KB.check_guards(buf, B * S, W, f"vit_assemble W={W}")


def test_text_embed_bits_with_wide_ids(K):
    """ids [N, context] read at ld_ids = context > L"""
    N, L, ctx, V, Wt = 5, 7, 12, 50, 260
    ids = torch.randint(0, V, (N, ctx), generator=gen(34), dtype=torch.int32)
    emb, pos = rnd(V, Wt, seed=35), rnd(ctx, Wt, seed=36)
    buf, x = KB.guarded(N * L, Wt, F32, DEV)
    K.text_embed(ids.to(DEV), emb.to(DEV), pos.to(DEV), x, N=N, L=L)
    KB.assert_equal_bits(x.cpu(), (emb[ids[:, :L].long()] + pos[:L]).reshape(N * L, Wt), "text_embed")
    KB.check_guards(buf, N * L, Wt, "text_embed")


def test_text_embed_packed_bits_and_untouched_rows(K):
    """N = 5 captions of lengths {1, 7, 1, 3, 12}; a token id past the vocabulary and the positions past the context (10) leave
    their rows as they were (NaN here)"""
    lens, V, ctx, Wt = [1, 7, 1, 3, 12], 40, 10, 132
    M = sum(lens)
    ids = torch.randint(0, V, (M,), generator=gen(60), dtype=torch.int32)
    ids[4], ids[9] = V, -1
    start = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
    emb, pos = rnd(V, Wt, seed=61), rnd(ctx, Wt, seed=62)
    buf, x = KB.guarded(M, Wt, F32, DEV)
    K.text_embed_packed(ids.to(DEV), start.to(DEV), emb.to(DEV), pos.to(DEV), x, N=len(lens))
    want = torch.full((M, Wt), float("nan"))
    for i, ln in enumerate(lens):
        for l in range(ln):
            r = int(start[i]) + l
            if l < ctx and 0 <= int(ids[r]) < V:
                want[r] = emb[int(ids[r])] + pos[l]
    assert int(torch.isnan(want[:, 0]).sum()) == 4  # two bad ids, two positions past the context
    KB.assert_equal_bits(x.cpu(), want, "text_embed_packed")
    KB.check_guards(buf, M, Wt, "text_embed_packed")


@pytest.mark.parametrize("E", [4, 1028])
def test_sort_assemble_bits(K, E):
    """off = 1 (the CLS row is skipped), S = 34, Sv = 33, NT = 4"""
    B, S, off, Sv, NT = 2, 34, 1, 33, 4
    tok, txt, ty = rnd(B * S, E, seed=40), rnd(B, NT, E, seed=41), rnd(2, E, seed=42)
    buf, xs = KB.guarded(B * (Sv + NT), E, F32, DEV)
    K.sort_assemble(wide(tok), txt.to(DEV), ty.to(DEV), xs, B=B, S=S, off=off, Sv=Sv, NT=NT)
    want = torch.cat([tok.view(B, S, E)[:, off:off + Sv] + ty[0], txt + ty[1]], 1).reshape(-1, E)
    KB.assert_equal_bits(xs.cpu(), want, f"sort_assemble E={E}")
    KB.check_guards(buf, B * (Sv + NT), E, f"sort_assemble E={E}")


@pytest.mark.parametrize("NT", [1, 4])
def test_text_mean_copy_bits_and_values(K, NT):
    """the [B, NT, E] `before` copy bit for bit; the mean as an ordered sum of NT addends (and its division)"""
    B, E = 3, 132
    t = rnd(NT * B, E, seed=38)
    bm, mean = KB.guarded(B, E, F32, DEV, cols=0)
    bb, before = KB.guarded(B * NT, E, F32, DEV, cols=0)
    K.text_mean(t.to(DEV), mean, before.view(B, NT, E), NT=NT, B=B)
    t3 = t.view(NT, B, E)
    KB.assert_equal_bits(before.cpu(), t3.permute(1, 0, 2).reshape(B * NT, E).contiguous(), "text_mean before")
    w = KB.assert_within(mean.cpu(), t3.double().mean(0), KB.sum_bound(t3.double().abs().sum(0) / NT, NT), "text_mean mean")
    KB.bound_line(f"text_mean NT={NT} mean", w)
    KB.check_guards(bm, B, E, "text_mean mean")
    KB.check_guards(bb, B * NT, E, "text_mean before")
    mean2 = torch.empty(B, E, device=DEV)
    K.text_mean(t.to(DEV), mean2, None, NT=NT, B=B)
    KB.assert_equal_bits(mean2, mean.contiguous(), "text_mean without the copy")


@pytest.mark.parametrize("NT", [1, 4])
def test_text_mean_bwd_bits(K, NT):
    B, E = 3, 132
    dmean = rnd(B, E, seed=39)
    buf, dt = KB.guarded(NT * B, E, F32, DEV, cols=0)
    K.text_mean_bwd(dmean.to(DEV), dt, NT=NT, B=B)
    KB.assert_equal_bits(dt.cpu(), (dmean / float(NT)).repeat(NT, 1), "text_mean_bwd")
    KB.check_guards(buf, NT * B, E, "text_mean_bwd")


# ================================================================================================ 3. ordered sums
def vit_bwd_case(K, B, T, n, W, n_pos, per_frame, seed, dup=False, same_bits=True):
    """one vit_assemble_bwd shape: dpatch = bf16(dtok) bit for bit, dcls / dpos / dtemporal per element under sum_bound, from
    non-zero accumulators, twice"""
    S = 1 + T * n
    TT = max(T, 4) + 1  # the temporal table is longer than the clip
    dtok = rnd(B * S, W, seed=seed)
    keep = keep_lists(B * T if per_frame else B, n, n_pos, seed=seed + 1)
    if dup:
        keep[1, 3] = keep[1, 7]  # a malformed mask: clip 1 holds one position twice, both slots are added
    keep = keep.view(B, T, n) if per_frame else keep
    init = dict(dcls=rnd(W, seed=seed + 2), dpos=rnd(n_pos + 1, W, seed=seed + 3), dtmp=rnd(TT, W, seed=seed + 4))
    d = dtok.double().view(B, S, W)
    cls, pt = d[:, 0], d[:, 1:].reshape(B, T, n, W)
    kp = (keep.long() if per_frame else keep.long()[:, None, :].expand(B, T, n)).reshape(-1)
    ref, Sab, cnt = {}, {}, {}
    ref["dcls"], Sab["dcls"], cnt["dcls"] = cls.sum(0), cls.abs().sum(0), B
    rp, sp, cp = (torch.zeros(n_pos + 1, W, dtype=torch.float64) for _ in range(3))
    rp[1:].index_add_(0, kp, pt.reshape(-1, W)); sp[1:].index_add_(0, kp, pt.reshape(-1, W).abs()); cp[1:].index_add_(0, kp, torch.ones(kp.numel(), W, dtype=torch.float64))
    rp[0], sp[0], cp[0] = cls.sum(0), cls.abs().sum(0), B
    ref["dpos"], Sab["dpos"], cnt["dpos"] = rp, sp, cp
    rt, st = torch.zeros(TT, W, dtype=torch.float64), torch.zeros(TT, W, dtype=torch.float64)
    rt[:T], st[:T] = pt.sum((0, 2)), pt.abs().sum((0, 2))
    ref["dtmp"], Sab["dtmp"], cnt["dtmp"] = rt, st, B * n
    runs, worst = [], 0.0
    for _ in range(2):
        bufs = {k: guarded_from(v, cols=0) for k, v in init.items()}
        bp, dpatch = KB.guarded(B * T * n, W, BF16, DEV)
        K.vit_assemble_bwd(wide(dtok), keep.to(DEV), dpatch, bufs["dcls"][1], bufs["dpos"][1], bufs["dtmp"][1], B=B, T=T, n=n)
        want = dtok.view(B, S, W)[:, 1:].reshape(B * T * n, W).bfloat16()
        KB.assert_equal_bits(dpatch.cpu(), want, "vit_assemble_bwd dpatch")
        KB.check_guards(bp, B * T * n, W, "vit_assemble_bwd dpatch")
        for k in init:
            got = bufs[k][1].cpu()
            guards_ok(bufs[k][0], init[k], f"vit_assemble_bwd {k}")
            b = KB.sum_bound(Sab[k], cnt[k], init=init[k])
            worst = max(worst, KB.assert_within(got, ref[k] + init[k].double(), b, f"vit_assemble_bwd {k}"))
        KB.assert_equal_bits(bufs["dtmp"][1][T:].cpu(), init["dtmp"][T:], "vit_assemble_bwd dtemporal rows past T")
        runs.append({k: bufs[k][1].cpu().clone() for k in init})
    if same_bits:
        for k in init:
            KB.assert_equal_bits(runs[1][k], runs[0][k], f"vit_assemble_bwd {k}, second run")
    return worst


@pytest.mark.parametrize("B,T,n,W,n_pos,same_bits", [
    (3, 2, 15, 8, 20, True),     # two slot groups, the last with one slot
    (18, 1, 29, 8, 40, True),    # 18 x 3 = 54 partials: four trips of the p += 16 loop, a ragged last one
    (258, 1, 2, 8, 6, True),     # a second 256-clip chunk of the positional rows
    (2, 16, 3, 260, 9, True),    # T == ASM_MAXT, a second column block with a ragged tail
    (2, 17, 3, 8, 9, False),     # T = 17: the per-frame kernel with fp32 atomics (order not fixed: no same-bits assertion)
    (2, 2, 3, 1028, 9, True),    # a second trip of the c += 1024 column loop
], ids=["two_groups", "54_partials", "258_clips", "T16_W260", "T17_atomics", "W1028"])
def test_vit_assemble_bwd_tube_sums(K, B, T, n, W, n_pos, same_bits):
    KB.bound_line(f"vit_assemble_bwd tube B={B} T={T} n={n} W={W}", vit_bwd_case(K, B, T, n, W, n_pos, False, seed=200 + B + T, same_bits=same_bits))


@pytest.mark.parametrize("B,T,n,W,n_pos", [(2, 3, 5, 8, 12), (65, 4, 2, 8, 6)], ids=["6_lists", "260_lists"])
def test_vit_assemble_bwd_per_frame_sums(K, B, T, n, W, n_pos):
    """keep [B, T, n] (v1): the (clip, frame) pairs are the gather's clips; B * T = 260 takes the second chunk"""
    KB.bound_line(f"vit_assemble_bwd per-frame B={B} T={T}", vit_bwd_case(K, B, T, n, W, n_pos, True, seed=300 + B))


def test_vit_assemble_bwd_position_held_twice(K):
    """a malformed tube mask with one position in two slots of a clip: both slots are added (the more[] path)"""
    KB.bound_line("vit_assemble_bwd duplicated keep index", vit_bwd_case(K, 3, 2, 15, 8, 20, False, seed=400, dup=True))


RUNS = [1, 15, 16, 17, 64, 65, 300]


def tok_bwd_case(K, ids, Wt, V, seed, sort=True):
    """text_embed_bwd on ids [N, L]: demb rows and dpos rows per element under sum_bound, from non-zero accumulators, twice"""
    N, L = ids.shape
    ctx = L + 2
    idw = torch.zeros(N, ctx, dtype=torch.int32)
    idw[:, :L] = ids  # ld_ids > L
    dx = rnd(N * L, Wt, seed=seed)
    init_e, init_p = rnd(V, Wt, seed=seed + 1), rnd(ctx, Wt, seed=seed + 2)
    d = dx.double()
    flat = ids.reshape(-1).long()
    re, se, ce = (torch.zeros(V, Wt, dtype=torch.float64) for _ in range(3))
    re.index_add_(0, flat, d); se.index_add_(0, flat, d.abs()); ce.index_add_(0, flat, torch.ones_like(d))
    rp, sp = torch.zeros(ctx, Wt, dtype=torch.float64), torch.zeros(ctx, Wt, dtype=torch.float64)
    rp[:L], sp[:L] = d.view(N, L, Wt).sum(0), d.view(N, L, Wt).abs().sum(0)
    ts = None
    if sort:
        order, seg = K.token_sort(ids.contiguous())
        ts = (order.to(DEV), seg.to(DEV))
    runs, worst = [], 0.0
    for _ in range(2 if sort else 1):
        be, demb = guarded_from(init_e, cols=0)
        bp, dpos = guarded_from(init_p, cols=0)
        K.text_embed_bwd(wide(dx), idw.to(DEV)[:, :L], demb, dpos, N=N, L=L, tok_sort=ts)
        guards_ok(be, init_e, "text_embed_bwd demb"); guards_ok(bp, init_p, "text_embed_bwd dpos")
        worst = max(worst, KB.assert_within(demb.cpu(), re + init_e.double(), KB.sum_bound(se, ce, init=init_e), f"text_embed_bwd demb Wt={Wt}"))
        worst = max(worst, KB.assert_within(dpos.cpu(), rp + init_p.double(), KB.sum_bound(sp, N, init=init_p), f"text_embed_bwd dpos Wt={Wt}"))
        runs.append((demb.cpu().clone(), dpos.cpu().clone()))
    if sort:
        KB.assert_equal_bits(runs[1][0], runs[0][0], "text_embed_bwd demb, second run")
        KB.assert_equal_bits(runs[1][1], runs[0][1], "text_embed_bwd dpos, second run")
    return worst


def run_ids(lens, L, seed):
    """[N, L] ids: token k + 1 appears lens[k] times, in a shuffled row order"""
    flat = torch.cat([torch.full((ln,), k + 1, dtype=torch.int32) for k, ln in enumerate(lens)])
    assert flat.numel() % L == 0
    return flat[torch.randperm(flat.numel(), generator=gen(seed))].view(-1, L)


@pytest.mark.parametrize("Wt", [8, 192, 768, 1028])
def test_text_embed_bwd_sorted_run_lengths(K, Wt):
    """runs of 1, 15, 16, 17, 64, 65 and 300 rows (478 rows, N = 239, L = 2): 65 and 300 go to the long-run kernel, 64 and less stay
    with the short one.  Wt 8: 128 thread groups; 192: G = 5 (16 G = 80: every run ends in clamped loads); 768: G = 1 with threads
    192..255 idle; 1028: Wt / 4 >= 256, a second c0 trip of one busy thread"""
    ids = run_ids(RUNS, 2, seed=70)
    order, seg = K.token_sort(ids)
    lens = torch.diff(seg[:len(RUNS) + 1].long()).tolist()
    assert lens[:2] == [65, 300] or lens[:2] == [300, 65], lens  # the long runs come first
    KB.bound_line(f"text_embed_bwd sorted Wt={Wt}", tok_bwd_case(K, ids, Wt, V=len(RUNS) + 2, seed=500 + Wt))


def test_text_embed_bwd_long_runs_past_slot_64(K):
    """70 distinct ids of 65 rows each: the first 64 runs belong to the long-run kernel, runs 64..69 must fall back to the short one"""
    ids = run_ids([65] * 70, 13, seed=71)
    KB.bound_line("text_embed_bwd 70 runs of 65", tok_bwd_case(K, ids, 8, V=72, seed=600))


@pytest.mark.parametrize("N", [1, 16, 17])
def test_text_embed_bwd_positions(K, N):
    """dpos[l] over N captions: one group busy, all 16 once, a second trip of the nn += 16 loop"""
    ids = torch.randint(0, 9, (N, 3), generator=gen(72 + N), dtype=torch.int32)
    KB.bound_line(f"text_embed_bwd dpos N={N}", tok_bwd_case(K, ids, 68, V=9, seed=700 + N))


def test_text_embed_bwd_atomic_form(K):
    """without tok_sort: fp32 atomics, the bound only"""
    KB.bound_line("text_embed_bwd atomics", tok_bwd_case(K, run_ids(RUNS, 2, seed=70), 192, V=len(RUNS) + 2, seed=800, sort=False))


@pytest.mark.parametrize("B,S,off,E", [(17, 33, 1, 8), (2, 64, 0, 260), (3, 5, 0, 128)], ids=["34_partials_off1", "two_chunks_W260", "one_chunk"])
def test_sort_assemble_bwd_sums(K, B, S, off, E):
    """dout = bf16 of one fp32 add, bit for bit; dtype[0] / dtype[1] per element under sum_bound, from non-zero accumulators, twice.
    (17, 33, 1, 8): two row chunks (the second with one row) and B * chunks = 34 > 16 partials; (2, 64, 0, 260): S % 32 == 0, a
    second trip of c += 256"""
    NT, Sv = 4, S - off
    So = Sv + NT
    dxs, dvid, init = rnd(B * So, E, seed=43 + B), rnd(B, E, seed=44), rnd(2, E, seed=45)
    d3 = dxs.view(B, So, E)
    full = torch.zeros(B, S, E)
    full[:, off:] = d3[:, :Sv]
    full[:, 0] += dvid
    want = full.reshape(B * S, E).bfloat16()
    ref = torch.stack([d3[:, :Sv].double().sum((0, 1)), d3[:, Sv:].double().sum((0, 1))]) + init.double()
    Sab = torch.stack([d3[:, :Sv].double().abs().sum((0, 1)), d3[:, Sv:].double().abs().sum((0, 1))])
    cnt = torch.tensor([[B * Sv], [B * NT]], dtype=torch.float64)
    runs = []
    for _ in range(2):
        bo, dout = KB.guarded(B * S, E, BF16, DEV)
        bt, dty = guarded_from(init, cols=0)
        K.sort_assemble_bwd(wide(dxs), dvid.to(DEV), dout, dty, B=B, S=S, off=off, Sv=Sv, NT=NT)
        KB.assert_equal_bits(dout.cpu(), want, "sort_assemble_bwd dout")
        KB.check_guards(bo, B * S, E, "sort_assemble_bwd dout"); guards_ok(bt, init, "sort_assemble_bwd dtype")
        w = KB.assert_within(dty.cpu(), ref, KB.sum_bound(Sab, cnt, init=init), "sort_assemble_bwd dtype")
        runs.append(dty.cpu().clone())
    KB.assert_equal_bits(runs[1], runs[0], "sort_assemble_bwd dtype, second run")
    KB.bound_line(f"sort_assemble_bwd B={B} S={S} off={off} E={E}", w)


def test_sort_assemble_bwd_without_dxs_and_without_dtype(K):
    """dxs = None: dout is the CLS-row gradient alone; dtype = None (dxs given): dout as before, no sum is written anywhere"""
    B, S, off, E, NT = 3, 5, 0, 128, 4
    So = S + NT
    dxs, dvid = rnd(B * So, E, seed=46), rnd(B, E, seed=47)
    bo, dout = KB.guarded(B * S, E, BF16, DEV)
    K.sort_assemble_bwd(None, dvid.to(DEV), dout, None, B=B, S=S, off=off, Sv=S, NT=NT)
    full = torch.zeros(B, S, E)
    full[:, 0] = dvid
    KB.assert_equal_bits(dout.cpu(), full.reshape(B * S, E).bfloat16(), "sort_assemble_bwd dxs=None")
    KB.check_guards(bo, B * S, E, "sort_assemble_bwd dxs=None")
    bo, dout = KB.guarded(B * S, E, BF16, DEV)
    K.sort_assemble_bwd(wide(dxs), dvid.to(DEV), dout, None, B=B, S=S, off=off, Sv=S, NT=NT)
    full = dxs.view(B, So, E)[:, :S].clone()
    full[:, 0] += dvid
    KB.assert_equal_bits(dout.cpu(), full.reshape(B * S, E).bfloat16(), "sort_assemble_bwd dtype=None")
    KB.check_guards(bo, B * S, E, "sort_assemble_bwd dtype=None")


# ================================================================================================ 4. losses
EPS = 1e-8


def l2_rows(R, E, seed):
    """fp32 [R, E]: row 0 exactly zero, row 1 of norm 1e-10 (clamped), row 2 of norm exactly fp32(eps), rows 3 / 4 of norm 1e-3 /
    1e3 next to them (R >= 5); every other row N(0, 1)"""
    x = rnd(R, E, seed=seed)
    if R >= 5:
        unit = x[:5].double() / x[:5].double().norm(dim=1, keepdim=True)
        x[0] = 0.0
        x[1] = (unit[1] * 1e-10).float()
        x[2] = 0.0
        x[2, E // 2] = KB.f32_const(EPS)
        x[3] = (unit[3] * 1e-3).float()
        x[4] = (unit[4] * 1e3).float()
    return x


@pytest.mark.parametrize("E", [1, 64, 65, 512])
@pytest.mark.parametrize("R", [1, 5, 9])
def test_l2norm_rows_and_backward_direct(K, R, E):
    """l2norm_rows / l2norm_rows_bwd called directly: one wave of a block busy (R 1), a second block with one row (5, 9), a lane
    loop of one element, one full trip, a second ragged trip, eight trips (E 1, 64, 65, 512); the clamped rows give dx = dxn / eps"""
    x = l2_rows(R, E, seed=900 + R + E)
    bx, xn = KB.guarded(R, E, F32, DEV, cols=0)
    bi, inv = KB.guarded(1, R, F32, DEV)
    inv = inv[0]
    K.l2norm_rows(x.to(DEV), xn, inv, EPS)
    KB.check_guards(bx, R, E, "l2norm_rows xn"); KB.check_guards(bi, 1, R, "l2norm_rows inv")
    w = KB.l2norm_check(x, EPS, xn.cpu(), inv.cpu(), what=f"l2norm_rows R={R} E={E}")
    if R >= 5:
        assert bool((inv[:2] < 0).all()) and bool((inv[3:] > 0).all()), inv  # zero and 1e-10 rows clamped, 1e-3 / 1e3 / N(0, 1) rows not
        print(f"l2norm_rows R={R} E={E}: the row of norm exactly eps came out {'clamped' if float(inv[2]) < 0 else 'not clamped'}")
    dxn = rnd(R, E, seed=950 + R + E)
    bd, dx = KB.guarded(R, E, F32, DEV, cols=0)
    xn_c, inv_c = xn.contiguous(), inv.contiguous()
    K.l2norm_rows_bwd(dxn.to(DEV), xn_c, inv_c, dx)
    KB.check_guards(bd, R, E, "l2norm_rows_bwd dx")
    w2 = KB.l2norm_bwd_check(dxn, xn_c.cpu(), inv_c.cpu(), dx.cpu(), what=f"l2norm_rows_bwd R={R} E={E}")
    if R >= 5:  # the clamped rows: dx = dxn / eps, one rounding
        want = dxn[:2].double() / KB.f32_const(EPS)
        KB.assert_within(dx[:2].cpu(), want, 3 * KB.U32 * want.abs() + 1e-45, "l2norm_rows_bwd clamped rows")
    KB.bound_line(f"l2norm_rows R={R} E={E}", w)
    KB.bound_line(f"l2norm_rows_bwd R={R} E={E}", w2)


def infonce_x(G, seed):
    """x [G, G] uniform in [-20, 20] (cosines over the temperature 0.05); where G allows: row 0 has its maximum on the diagonal,
    row 1 an off-diagonal entry 30 above its diagonal, column 2 is constant"""
    x = (torch.rand(G, G, generator=gen(seed)) * 40.0 - 20.0)
    x[0, 0] = 21.0
    if G >= 2:
        x[1, 0] = x[1, 1] + 30.0
    if G >= 3:
        x[:, 2] = 3.0
    return x


@pytest.mark.parametrize("G", [1, 2, 3, 5, 63, 64, 65, 257])
def test_infonce_per_element(K, G):
    """lse, dx and the loss per element on an x built here: G < 4 leaves waves of the column kernel without rows, 63 / 64 / 65 sit
    around its 64-column block, 257 gives a thread of the loss kernel a second term; with and without dx; the loss adds into 0.75"""
    x = infonce_x(G, seed=1000 + G)
    xd = x.to(DEV)
    worst = {}
    for with_dx in (True, False):
        bl, lse = KB.guarded(1, 2 * G, F32, DEV)
        bd, dx = KB.guarded(G, G, F32, DEV, cols=0)
        loss = torch.full((1,), 0.75, device=DEV)
        K.infonce(xd, lse[0], dx if with_dx else None, loss)
        KB.check_guards(bl, 1, 2 * G, "infonce lse")
        if with_dx:
            KB.check_guards(bd, G, G, "infonce dx")
        else:
            assert bool(torch.isnan(dx).all()), "infonce wrote dx without being asked to"
        res = KB.infonce_check(x, lse[0].cpu(), dx.cpu() if with_dx else None, loss.cpu(), loss0=0.75, what=f"infonce G={G}")
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        KB.bound_line(f"infonce G={G} {k}", v)


@pytest.mark.parametrize("C", [1, 4, 7])
@pytest.mark.parametrize("R", [1, 255, 256, 257, 768])
def test_cross_entropy_per_element(K, R, C):
    """one block walks the rows: one thread, one short of a trip, one full trip, one row in the second trip, three trips (the step's
    R); random labels with a run of one label; scale 2; with and without dlogits; the loss adds into 0.25"""
    logits = rnd(R, C, seed=1100 + R + C, scale=3.0)
    labels = torch.randint(0, C, (R,), generator=gen(1200 + R + C), dtype=torch.int32)
    labels[R // 4:R // 2] = C - 1
    worst = {}
    for with_d in (True, False):
        bd, dl = KB.guarded(R, C, F32, DEV, cols=0)
        loss = torch.full((1,), 0.25, device=DEV)
        K.cross_entropy(logits.to(DEV), labels.to(DEV), 2.0, dl if with_d else None, loss)
        if with_d:
            KB.check_guards(bd, R, C, "cross_entropy dlogits")
        res = KB.ce_check(logits, labels, 2.0, dl.cpu() if with_d else None, loss.cpu(), loss0=0.25, what=f"cross_entropy R={R} C={C}")
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        KB.bound_line(f"cross_entropy R={R} C={C} {k}", v)


def test_contrastive_head_rows_at_65(K):
    """LossHead.contrastive at G = 65, E = 64: dv / dt per row against float64 autograd.  The tolerance is the per-row norm of the
    composed element bounds (kernel_bounds.contrastive_bound) over the row norm assert_rows_within divides by"""
    from tvts_amd.engine import LossHead
    G, E = 65, 64
    v, t = rnd(G, E, seed=45), rnd(G, E, seed=46)
    loss_ref, dv_ref, dt_ref, e_dv, e_dt = KB.contrastive_bound(v, t, 0.05, EPS)
    head = LossHead(torch.device(DEV))
    loss, dv, dt = head.contrastive(v.to(DEV), t.to(DEV))
    for nm, got, ref, e in (("dv", dv, dv_ref, e_dv), ("dt", dt, dt_ref, e_dt)):
        den = ref.norm(dim=1)
        tol = float((e.norm(dim=1) / torch.maximum(den, 0.05 * den.mean())).max())
        w = KB.assert_rows_within(got.cpu(), ref, tol, what=f"contrastive {nm} (tol {tol:.3g})")
        we = KB.assert_within(got.cpu(), ref, e, f"contrastive {nm} per element")
        print(f"contrastive G=65 {nm}: worst row {w:.3g} of tol {tol:.3g}")
        KB.bound_line(f"contrastive G=65 {nm} (per-row rel / tol)", w / tol)
        KB.bound_line(f"contrastive G=65 {nm} (per element)", we)
    assert abs(float(loss) - loss_ref) < 2e-5 * max(1.0, abs(loss_ref))


# ================================================================================================ 5. AdamW
CH = 1024
GROUPS = [0, 1, 2, 3, 255, 7]
LR4, WD4 = [1e-2, 3e-3, 1e-4, 1e-3], [0.05, 0.0, 0.01, 0.0]


def adam_state(seed):
    """fp32 p, g, m, v over six 1024-element chunks; chunk 0 carries the special elements: g = m = v = 0 (0..7), |g| = 1e-12
    (8..15, m = v = 0), |p| = 1e4 (16)"""
    n = CH * len(GROUPS)
    p, g = rnd(n, seed=seed), rnd(n, seed=seed + 1, scale=0.1)
    m, v = rnd(n, seed=seed + 2, scale=0.05), torch.rand(n, generator=gen(seed + 3)) * 1e-2
    g[:8], m[:16], v[:16] = 0.0, 0.0, 0.0
    g[8:16] = torch.tensor([1e-12, -1e-12] * 4)
    p[16] = -1e4
    return p, g, m, v


def adam_run(K, state, step, *, lr4=LR4, wd4=WD4, step_dev=None, hyper_dev=None, grad_scale=0.5):
    p, g, m, v = (t.to(DEV).clone() for t in state)
    sh = torch.full((p.numel(),), -3.0, dtype=BF16, device=DEV)
    K.adamw_hf(p, g, m, v, sh, torch.tensor(GROUPS, dtype=torch.uint8, device=DEV), lr4, wd4, step, grad_scale=grad_scale,
               step_dev=step_dev, hyper_dev=hyper_dev)
    return p.cpu(), m.cpu(), v.cpu(), sh.cpu()


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adamw_per_element(K, step):
    """groups {0, 1, 2, 3, 255, 7} over six chunks (wd > 0 in groups 0 and 2): p, m, v per element (adamw_check), the shadow bit for
    bit; the chunks of groups 255 and 7 keep every bit"""
    st = adam_state(seed=1300)
    p1, m1, v1, sh = adam_run(K, st, step)
    worst = 0.0
    for ci, grp in enumerate(GROUPS):
        sl = slice(ci * CH, (ci + 1) * CH)
        if grp > 3:
            for nm, got, was in (("p", p1, st[0]), ("m", m1, st[2]), ("v", v1, st[3])):
                KB.assert_equal_bits(got[sl], was[sl], f"adamw group {grp}: {nm} must stay")
            KB.assert_equal_bits(sh[sl], torch.full((CH,), -3.0, dtype=BF16), f"adamw group {grp}: shadow must stay")
            continue
        worst = max(worst, KB.adamw_check(st[0][sl], st[1][sl], st[2][sl], st[3][sl], p1[sl], m1[sl], v1[sl], sh[sl], lr=LR4[grp],
                                          wd=WD4[grp], step=step, grad_scale=0.5, what=f"adamw step {step} group {grp}"))
    KB.bound_line(f"adamw step={step}", worst)


def test_adamw_hyper_dev_table(K):
    """lr | wd read from device memory: the host arrays hold other values, the result equals the step_dev run given the table's
    values on the host, bit for bit"""
    st = adam_state(seed=1400)
    sd = torch.tensor([5], dtype=torch.int32, device=DEV)
    hd = torch.tensor(LR4 + WD4, dtype=F32, device=DEV)
    a = adam_run(K, st, 0, lr4=[9.0, 9.0, 9.0, 9.0], wd4=[0.5, 0.5, 0.5, 0.5], step_dev=sd, hyper_dev=hd)
    b = adam_run(K, st, 0, step_dev=sd)
    for nm, x, y in zip(("p", "m", "v", "shadow"), a, b):
        KB.assert_equal_bits(x, y, f"adamw hyper_dev: {nm}")
    assert not torch.equal(b[0][:4 * CH], st[0][:4 * CH])


@pytest.mark.parametrize("step", [1, 2, 7, 1000, 100000])
def test_adamw_host_step_equals_device_step(K, step):
    """the kernel comment's claim: the host-step and the device-step call give the same bits in p, m, v and the shadow"""
    st = adam_state(seed=1500)
    a = adam_run(K, st, step)
    b = adam_run(K, st, 0, step_dev=torch.tensor([step], dtype=torch.int32, device=DEV))
    for nm, x, y in zip(("p", "m", "v", "shadow"), a, b):
        KB.assert_equal_bits(x, y, f"adamw host step vs device step {step}: {nm}")
