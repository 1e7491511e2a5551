"""CPU side of the micro-batched pretraining step (StepRunner(micro_batches=n)): split_batch, the embedding-cache
schedule restated on the oracle (tests/micro_batch_ref.py) against the oracle's unsplit step, the chunk-local negative control, the
option's refusals and the config key (no GPU needed)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import micro_batch_ref as R  # noqa: E402

from oracle import tvts_oracle as O  # noqa: E402

GPU_GATE = 2e-2  # the parameter gate of the GPU step tests (test_training_curve_tracks_oracle); the control must clear 10x this


@pytest.fixture(scope="module")
def tiny():
    from tvts_amd import arch as A
    a = A.small_arch()
    oarch = O.tiny_arch(**a)
    return a, oarch, O.synth_params(oarch, seed=31)


@pytest.fixture(scope="module")
def unsplit(tiny):
    """the oracle's unsplit step of every case, computed once: {case: (batch, loss1, loss2, grads)}"""
    _, oarch, P = tiny
    out = {}
    for B, n, seed in R.CASES:
        batch = O.synth_batch(oarch, B=B, T=2, seed=seed, caption_len=8)
        out[(B, n, seed)] = (batch,) + R.unsplit_grads(P, batch, oarch)
    return out


@pytest.mark.parametrize("B,n", [(4, 2), (4, 4), (6, 3)])
def test_split_batch_keeps_every_pair(tiny, B, n):
    """the oracle's per-chunk embeddings, concatenated, are its full-batch embeddings (fp32 rounding: a row's GEMM products are summed
    in another blocking at another batch size); with the text rows sliced contiguously they are not"""
    from tvts_amd.step import split_batch
    _, oarch, P = tiny
    batch = O.synth_batch(oarch, B=B, T=2, seed=44, caption_len=8)
    with torch.no_grad():
        te, ve, _ = O.model_forward(P, batch, oarch)
        chunks = split_batch(batch, n)
        got = [O.model_forward(P, c, oarch)[:2] for c in chunks]
        bad = [O.model_forward(P, c, oarch)[:2] for c in R.contiguous_split(batch, n)]
    assert len(chunks) == n and all(c["video"].shape[0] == B // n and c["text"].shape[0] == oarch["n_trans"] * (B // n) for c in chunks)
    assert torch.allclose(torch.cat([g[0] for g in got]), te, rtol=1e-5, atol=1e-6)
    assert torch.allclose(torch.cat([g[1] for g in got]), ve, rtol=1e-5, atol=1e-6)
    assert torch.allclose(torch.cat([g[1] for g in bad]), ve, rtol=1e-5, atol=1e-6)      # (the clips are sliced alike)
    assert not torch.allclose(torch.cat([g[0] for g in bad]), te, rtol=1e-2, atol=1e-3)  # ... the captions are the wrong ones
    # the fields: labels and masks by clip, the text rows transcript-major
    NT, b = oarch["n_trans"], B // n
    for k, c in enumerate(chunks):
        assert torch.equal(c["keep_ind"], batch["keep_ind"][k * b:(k + 1) * b]) and torch.equal(c["label"], batch["label"][k * b:(k + 1) * b])
        for t in range(NT):
            assert torch.equal(c["text"][t * b:(t + 1) * b], batch["text"][t * B + k * b:t * B + (k + 1) * b])


@pytest.mark.parametrize("case", R.CASES)
def test_schedule_is_the_unsplit_step_and_chunk_local_is_not(tiny, unsplit, case):
    from tvts_amd.step import split_batch
    _, oarch, P = tiny
    B, n, seed = case
    batch, l1, l2, grads = unsplit[case]
    chunks = split_batch(batch, n)
    s1, s2, sg = R.schedule_grads(P, chunks, oarch)
    assert sorted(sg) == sorted(grads) and len(grads) > 50
    assert abs(s1 - l1) < 1e-5 and abs(s2 - l2) < 1e-5, (s1, l1, s2, l2)
    worst = max((R.rel(sg[k], grads[k]), k) for k in grads if float(grads[k].norm()) > 0)
    total = R.rel(R.flat(sg), R.flat(grads))
    # fp32 rounding only: the same products summed in another order.  A reordered fp32 sum of N terms moves by ~sqrt(N) eps of the
    # terms' size; N <= B * tokens * width ~ 1e4 ... 1e5 here and eps = 6e-8 give ~2e-5, through a few layers of cancellation 1e-4
    # per tensor -- three orders under what a tensor that received one chunk's share only would show (1 - 1 / n >= 0.5)
    assert worst[0] < 1e-4 and total < 1e-4, (worst, total)
    for k in grads:
        if float(grads[k].norm()) == 0:
            assert float(sg[k].norm()) == 0, k
    c1, c2, cg = R.chunk_local_grads(P, chunks, oarch)
    far = R.rel(R.flat(cg), R.flat(grads))
    print(f"   [B {B} chunks {n} seed {seed}] full-batch loss1 {l1:.4f}, chunk-local mean loss1 {c1:.4f}, gradient rel-L2 between the two "
          f"{far:.2f}; schedule against unsplit: total {total:.1e}, worst tensor {worst[0]:.1e}")
    assert far >= 10 * GPU_GATE, far
    assert abs(c1 - l1) > 1.0 and abs(c2 - l2) < 1e-5, (c1, l1, c2, l2)  # the sorting loss is a per-sample mean: it agrees


def test_split_batch_fields_and_refusals(tiny):
    from tvts_amd.step import split_batch
    _, oarch, _ = tiny
    batch = O.synth_batch(oarch, B=4, T=2, seed=45, caption_len=8)
    meta = {"paths": ["a", "b", "c", "d"]}
    for bad in (3, 8):
        with pytest.raises(ValueError, match=f"micro_batches {bad} does not divide the batch of 4 clips"):
            split_batch(batch, bad)
    for bad in (0, -2, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="must be an int >= 1"):
            split_batch(batch, bad)
    with pytest.raises(ValueError, match="text .* expected n_trans \\* 4 token rows"):
        split_batch(dict(batch, text=batch["text"][:6]), 2)
    with pytest.raises(ValueError, match="label .* is not per clip"):
        split_batch(dict(batch, label=batch["label"][:3]), 2)
    one = split_batch(batch, 1)
    assert len(one) == 1 and all(torch.equal(one[0][k], batch[k]) for k in batch)
    # uint8 wire format with crop / resize, a shared tube mask, meta
    u8 = dict(video=torch.randint(0, 255, (4, 2, 40, 48, 3), dtype=torch.uint8), text=batch["text"], label=batch["label"],
              keep_ind=batch["keep_ind"][:1], crop=torch.arange(8).reshape(4, 2), resize=36, meta=meta)
    for k, c in enumerate(split_batch(u8, 2)):
        assert c["video"].dtype == torch.uint8 and torch.equal(c["video"], u8["video"][2 * k:2 * k + 2])
        assert torch.equal(c["crop"], u8["crop"][2 * k:2 * k + 2]) and c["resize"] == 36 and c["meta"] is meta
        assert c["keep_ind"] is u8["keep_ind"] and "sample_offset" not in c and "mask_seed" not in c


def test_device_drawn_masks_number_the_samples_globally(tiny):
    """mask_seed is kept and sample_offset moves by the chunk's first clip, so that the chunks' draws are the rows of the unsplit
    batch's (the oracle's tube_mask restates the kernel's draw)"""
    from tvts_amd.step import split_batch
    _, oarch, _ = tiny
    batch = O.synth_batch(oarch, B=6, T=2, seed=46, caption_len=8)
    del batch["keep_ind"]
    ppf, nk = O.patches_per_frame(oarch), O.n_keep(oarch)
    for off in (None, 0, 1000):
        data = dict(batch, mask_seed=77)
        if off is not None:
            data["sample_offset"] = off
        chunks = split_batch(data, 3)
        assert [c["mask_seed"] for c in chunks] == [77] * 3
        assert [c["sample_offset"] for c in chunks] == [(off or 0) + lo for lo in (0, 2, 4)]
        whole = torch.as_tensor(O.tube_mask(77, off or 0, 6, ppf, nk))
        parts = torch.cat([torch.as_tensor(O.tube_mask(c["mask_seed"], c["sample_offset"], 2, ppf, nk)) for c in chunks])
        assert torch.equal(parts, whole)


def test_option_refusals_and_config_key():
    from tvts_amd.base.base_trainer import micro_batch_config
    from tvts_amd.step import micro_batch_option
    assert micro_batch_option(1) == 1 and micro_batch_option(4) == 4
    assert micro_batch_option(1, fused=False, ranged=True, family="v1") == 1  # 1 is the step of today: nothing to refuse
    for bad in (0, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="micro_batches .* must be an int >= 1"):
            micro_batch_option(bad)
    with pytest.raises(RuntimeError, match=r"StepRunner\(micro_batches=2\) cannot be combined with adamw_ranges / TVTS_ADAMW_RANGES=1"):
        micro_batch_option(2, ranged=True)
    with pytest.raises(RuntimeError, match=r"StepRunner\(micro_batches=2\) needs the fused optimizer .* got AdamW"):
        micro_batch_option(2, fused=False, optimizer="AdamW")
    with pytest.raises(NotImplementedError, match="not built for the v1 engine: its text dropout seed advances"):
        micro_batch_option(2, family="v1")
    base = dict(epochs=1, save_period=1, verbosity=2)
    assert micro_batch_config(base) == 1 and micro_batch_config(dict(base, micro_batches=4)) == 4
    for bad in (0, -3, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match=r"config\['trainer'\]\['micro_batches'\]"):
            micro_batch_config(dict(base, micro_batches=bad))
