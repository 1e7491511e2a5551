"""arch["text_unpadded"] (DESIGN.md 8b "v1"): the v1 training step with its DistilBERT tower over M = sum(len_i) packed rows, against
the v1 oracle at the gates of tests/test_v1_gpu.py's padded step tests and against the padded step on the same seed and batch (the
1.25 rule of DESIGN.md 8a: e_unpadded <= 1.25 e_padded + 1e-4 for every gated distance to the oracle), plus the exact statements the
dead-row argument makes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tvts_v1_oracle as V  # noqa: E402  (checker only)
from test_v1_gpu import build, check_grads, engine_step, min_cos, rel, small  # noqa: E402  (the padded step tests' own helpers and gates)

DEV = "cuda:0"
M64 = (1 << 64) - 1
# The longest caption of the ragged batches: 17, the smallest batch that holds the forced lengths 2, 16, 17 (both sides of the 16-row
# tile edge) and the one closest to the captions of up to 13 tokens the gates of tests/test_v1_gpu.py were set on.  Those gates are no
# property of a batch-independent kind: the PADDED step's own distance to the oracle moves with the batch (measured on ragged batches
# with a longest caption of 17 / 20 / 24 / 33, n_trans 4: |loss1 - oracle| 8.9e-3 / 5.9e-3 / 1.02e-2 / 1.01e-2 against the gate 1e-2,
# gradient norm 1.2e-3 / 1.1e-2 / 9.7e-3 / 1.3e-3 against 1e-2), and at these lengths the unpadded step reproduces the padded step's
# distances digit for digit.  The 33-48 and 49-80 tile classes are the kernel tests' (tests/test_attention_packed_bidir_gpu.py).
LONGEST = 17


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tvts_amd import hip
    return hip


def ragged_batch(oa, nt, seed=6, forced=(LONGEST, 2, 16, 17), equal=None):
    """the synthetic v1 batch with caption lengths forced to include 2, 16, 17 and the longest (or all equal to `equal`)"""
    batch = V.synth_batch(oa, B=4, T=6, seed=seed, n_trans=nt, caption_len=LONGEST if equal is None else equal)
    ids, mask = batch["text"]["input_ids"], batch["text"]["attention_mask"]
    lens = mask.sum(-1).tolist()
    if equal is None:
        lens[:len(forced)] = forced
    else:
        lens = [equal] * len(lens)
    g = torch.Generator().manual_seed(seed + 100)
    cls_id, sep_id = int(ids[0, 0]), int(ids[0, LONGEST - 1 if equal is None else equal - 1])
    for r, n in enumerate(lens):
        ids[r], mask[r] = 0, 0
        ids[r, :n] = torch.randint(1, oa["vocab"] - 2, (n,), generator=g)
        ids[r, 0], ids[r, n - 1], mask[r, :n] = cls_id, sep_id, 1
    assert mask.sum(-1).tolist() == lens and int(mask.sum(-1).max()) == ids.shape[1]
    return batch


def grad_dist(store, grads):
    """the two distances check_grads gates: |global norm - oracle's| / oracle's, and 1 - the worst per-tensor cosine"""
    tot_ref = sum(float(g.norm()) ** 2 for g in grads.values()) ** 0.5
    tot, worst = 0.0, 1.0
    for k, g in grads.items():
        mine = store.g(k).detach().cpu()
        tot += float(mine.norm()) ** 2
        if float(g.norm()) > 1e-3 * tot_ref:
            worst = min(worst, float(torch.nn.functional.cosine_similarity(mine.double().flatten(), g.double().flatten(), dim=0)))
    return abs(tot ** 0.5 - tot_ref) / tot_ref, 1.0 - worst


_ORACLE = {}


def oracle_step(oa, P, batch, key, drop):
    """the oracle's step on a batch, once per case"""
    if key not in _ORACLE:
        leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        r1, r2, rte, rve, rpred = V.step_losses(leaves, batch, oa, drop=drop)
        (r1 + r2).backward()
        _ORACLE[key] = (float(r1), float(r2), rte.detach(), rve.detach(), None if rpred is None else rpred.detach(),
                        {k: v.grad for k, v in leaves.items() if v.grad is not None})
    return _ORACLE[key]


def distances(m, out, ref):
    l1, l2, te, ve, pred = out
    r1, r2, rte, rve, rpred, grads = ref
    gn, gc = grad_dist(m.store, grads)
    d = {"text rel": rel(te, rte), "text 1-cos": 1 - min_cos(te, rte), "video rel": rel(ve, rve), "video 1-cos": 1 - min_cos(ve, rve),
         "loss1": abs(l1 - r1), "loss2": abs(l2 - r2), "grad norm": gn, "grad 1-cos": gc}
    if pred is not None:
        d["pred rel"] = rel(pred.view_as(rpred), rpred)
    return d


@pytest.mark.parametrize("p", [0.1, 0.0])
@pytest.mark.parametrize("nt", [4, 1])
def test_unpadded_step_against_the_oracle_and_the_padded_step(K, nt, p):
    """One training step, unpadded and padded on the same seed and batch.  Measured distances to the oracle (unpadded / padded):
    see DESIGN.md 8b "v1", "Parity"."""
    a, oa = small()
    P = V.synth_params(oa, seed=5)
    batch = ragged_batch(oa, nt)
    lens = batch["text"]["attention_mask"].sum(-1)
    assert {2, 16, 17, LONGEST} <= set(lens.tolist()) and int(lens.max()) == LONGEST
    mu, mp = build(dict(a, text_unpadded=True), P, dropout=p), build(a, P, dropout=p)
    assert mu.engine.text_unpadded and not mp.engine.text_unpadded
    seed0 = int(mu.engine.drop_seed.item()) & M64
    assert seed0 == int(mp.engine.drop_seed.item()) & M64
    seed1 = (seed0 + mu.engine.DROP_STEP_STRIDE) & M64
    ref = oracle_step(oa, P, batch, (nt, p), dict(p=p, seed=seed1) if p > 0 else None)
    r1, r2, rte, rve, rpred, grads = ref
    out_u, out_p = engine_step(mu, batch), engine_step(mp, batch)
    pb = mu.engine.ctx
    assert pb["M"] == int(lens.sum()) and pb["ids"].numel() == pb["M"] and pb["L"] == LONGEST
    assert mu.engine.buf["txt.x0"].shape[0] == pb["M"] and mp.engine.buf["txt.x0"].shape[0] == len(lens) * LONGEST  # no padding rows
    if p > 0:
        assert (int(mu.engine.drop_seed.item()) & M64) == seed1
    du, dp_ = distances(mu, out_u, ref), distances(mp, out_p, ref)
    for k in du:
        print(f"DIST nt {nt} p {p} {k}: unpadded {du[k]:.3e} padded {dp_[k]:.3e}")
    # --- the gates of tests/test_v1_gpu.py::test_small_v1_forward_backward / _training_mode_dropout
    l1, l2, te, ve, pred = out_u
    assert min_cos(te, rte) > 0.9995 and rel(te, rte) < 0.02, (min_cos(te, rte), rel(te, rte))
    assert min_cos(ve, rve) > 0.9995 and rel(ve, rve) < 0.02, (min_cos(ve, rve), rel(ve, rve))
    if nt == 1:
        assert pred is None and rpred is None
    else:
        assert rel(pred.view_as(rpred), rpred) < 0.03
    assert abs(l1 - r1) < (1e-2 if nt == 4 else 2e-2) and abs(l2 - r2) < 1e-2, (l1, r1, l2, r2)
    check_grads(mu.store, grads, gn_tol=0.01 if nt == 4 else 0.03)
    # --- against the padded step: e_unpadded <= 1.25 e_padded + 1e-4 for every distance gated above
    bad = {k: (du[k], dp_[k]) for k in du if not du[k] <= 1.25 * dp_[k] + 1e-4}
    assert not bad, bad
    # --- exact statements: no padded row exists, so nothing can reach a position behind the longest caption or the pad id
    gpos = mu.store.g("text_model.embeddings.position_embeddings.weight")
    assert float(gpos[LONGEST:].abs().max()) == 0.0 and float(gpos[:LONGEST].abs().max()) > 0.0
    assert float(mu.store.g("text_model.embeddings.word_embeddings.weight")[0].abs().max()) == 0.0
    assert int((batch["text"]["input_ids"] == 0).sum()) > 0  # (the pad id is in the batch's rectangle)


def test_equal_lengths_keep_every_row(K):
    """a batch whose captions all have length L: M == N * L, and the step is the padded step's within the same gates"""
    a, oa = small()
    P = V.synth_params(oa, seed=5)
    batch = ragged_batch(oa, 4, equal=12)
    N = batch["text"]["input_ids"].shape[0]
    mu, mp = build(dict(a, text_unpadded=True), P, dropout=0.1), build(a, P, dropout=0.1)
    seed1 = ((int(mu.engine.drop_seed.item()) & M64) + mu.engine.DROP_STEP_STRIDE) & M64
    ref = oracle_step(oa, P, batch, "equal", dict(p=0.1, seed=seed1))
    out_u, out_p = engine_step(mu, batch), engine_step(mp, batch)
    assert mu.engine.ctx["M"] == N * 12 and mu.engine.ctx["max_len"] == 12 and mu.engine.ctx["L"] == 12
    du, dp_ = distances(mu, out_u, ref), distances(mp, out_p, ref)
    bad = {k: (du[k], dp_[k]) for k in du if not du[k] <= 1.25 * dp_[k] + 1e-4}
    assert not bad, bad
    check_grads(mu.store, ref[5])


def test_two_identical_steps_give_identical_bits(K):
    a, oa = small()
    P = V.synth_params(oa, seed=5)
    batch = ragged_batch(oa, 4)
    m = build(dict(a, text_unpadded=True), P, dropout=0.1)
    seed0 = m.engine.drop_seed.clone()
    engine_step(m, batch)
    g1 = m.store.grad.clone()
    m.engine.drop_seed.copy_(seed0)
    engine_step(m, batch)
    assert torch.equal(g1.view(torch.int32), m.store.grad.view(torch.int32)), "the whole flat gradient, bit for bit"
    assert float(g1.abs().max()) > 0.0


def test_encode_text_packed(K):
    """TVTS.encode_text(text, packed=True) against the default: both within the 1.25 rule of the oracle's eval-mode tower, the
    default's bits untouched by the option, drop_seed untouched by either"""
    a, oa = small()
    P = V.synth_params(oa, seed=5)
    text = ragged_batch(oa, 4)["text"]
    m = build(a, P, dropout=0.1)
    seed0 = m.engine.drop_seed.clone()
    with torch.no_grad():
        _, want = V.compute_text(P, text, oa)
    padded = m.encode_text(text)
    packed = m.encode_text(text, packed=True)
    again = m.encode_text(text, packed=False)
    assert torch.equal(padded.view(torch.int32), again.view(torch.int32))
    assert torch.equal(m.engine.drop_seed, seed0)
    assert packed.shape == padded.shape == want.shape
    eu, ep = rel(packed, want), rel(padded, want)
    cu, cp = 1 - min_cos(packed, want), 1 - min_cos(padded, want)
    print(f"DIST encode_text rel: packed {eu:.3e} padded {ep:.3e}; 1 - min cos: packed {cu:.3e} padded {cp:.3e}")
    assert eu < 0.02 and 1 - cu > 0.9995
    assert eu <= 1.25 * ep + 1e-4 and cu <= 1.25 * cp + 1e-4, (eu, ep, cu, cp)
    with pytest.raises(ValueError, match="80"):
        m.encode_text({"input_ids": torch.ones(2, 81, dtype=torch.int64), "attention_mask": torch.ones(2, 81, dtype=torch.int64)}, packed=True)


def test_three_steps_track_the_padded_run(K):
    """three optimizer steps, drop_seed advancing, the engine's seed sequence handed to the oracle step by step (as
    tests/test_v1_gpu.py::test_v1_training_curve_with_dropout_tracks_oracle does): at every step both losses of the unpadded run are
    within that test's gate of the oracle's, and within 1.25 x the padded run's distance + 1e-4; such batches step eagerly under
    GraphReplay"""
    from oracle import tvts_oracle as O
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import GraphReplay, StepRunner
    a, oa = small()
    P = V.synth_params(oa, seed=7)
    batch = ragged_batch(oa, 4, seed=8)
    curves = {}
    for name, arch in (("unpadded", dict(a, text_unpadded=True)), ("padded", a)):
        m = build(arch, P, dropout=0.1)
        opt = FusedHFAdamW([dict(params=list(m.parameters()), lr=3e-4, weight_decay=0.0)], m.store, model=m)
        run = StepRunner(m, opt)
        if name == "unpadded":
            run = GraphReplay(run)
        seed0 = int(m.engine.drop_seed.item()) & M64
        rows = []
        for _ in range(3):
            out = run.step(batch)
            rows.append([float(out["loss1"]), float(out["loss2"])])
        curves[name] = np.array(rows)
        assert (int(m.engine.drop_seed.item()) & M64) == (seed0 + 3 * m.engine.DROP_STEP_STRIDE) & M64
        if name == "unpadded":
            assert run.replays == 0 and run.captures == 0 and run.eager == 3
    Pr = {k: v.clone() for k, v in P.items()}
    st = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in Pr.items()}
    seed, ref = seed0, []
    for step in range(1, 4):
        seed = (seed + m.engine.DROP_STEP_STRIDE) & M64
        leaves = {k: v.clone().requires_grad_(True) for k, v in Pr.items()}
        r1, r2, *_ = V.step_losses(leaves, batch, oa, drop=dict(p=0.1, seed=seed))
        (r1 + r2).backward()
        ref.append([float(r1), float(r2)])
        for k in Pr:
            gk = leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(Pr[k])
            O.hf_adamw_step(Pr[k], gk, st[k][0], st[k][1], step, 3e-4, 0.0)
    ref = np.array(ref)
    eu, ep = np.abs(curves["unpadded"] - ref), np.abs(curves["padded"] - ref)
    print("DIST three steps |loss - oracle| (loss1, loss2 per step): unpadded", eu.tolist(), "padded", ep.tolist())
    assert len({tuple(r) for r in curves["unpadded"].tolist()}) == 3  # (new masks and new weights every step)
    tot_u, tot_r = curves["unpadded"].sum(1), ref.sum(1)
    assert np.all(np.abs(tot_u - tot_r) < 0.02 * np.abs(tot_r) + 1e-2), (curves["unpadded"], ref)
    assert np.all(eu <= 1.25 * ep + 1e-4), (eu, ep)
