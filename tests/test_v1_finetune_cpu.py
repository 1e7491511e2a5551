"""CPU checks of the v1 fine-tuning step's host side: the grouping rule, the test-side reference (tests/v1_finetune_ref.py) against
the fixture the reference's own classes produced (tests/golden/v1_finetune.npz), and the integer restatement of the draw."""
import numpy as np
import pytest
import torch

import v1_downstream_synth as S
import v1_finetune_ref as R

F = R.FX


class _Named:
    """what param_groups reads of the downstream class, without a GPU: named parameters of the class's shapes, the skip list, the
    trainable map and the depth"""

    def __init__(self, kw, classes):
        self.arch = dict(layers=kw["depth"])
        self._p = {k: torch.nn.Parameter(torch.zeros(v.shape), requires_grad=False) for k, v in S.synth_state(kw, 1, classes).items()}

    def named_parameters(self):
        return list(self._p.items())

    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def set_trainable(self, trainable="all"):
        return {n: trainable == "all" or n.startswith("head.") for n in self._p}


def _fixture_groups(f, which):
    names, member_group = [str(s) for s in f[which + "_names"]], f[which + "_member_group"]
    members = [str(s) for s in f[which + "_members"]]
    return [(n, float(f[which + "_wds"][i]), float(f[which + "_scales"][i]), [m for m, g in zip(members, member_group) if g == i])
            for i, n in enumerate(names)]


@pytest.mark.parametrize("which", ["all", "head"])
def test_param_groups_equal_reference(golden, which):
    from tvts_amd.downstream.finetune_v1 import param_groups
    f = golden("v1_finetune")
    want = _fixture_groups(f, which)
    m = _Named(S.TINY, F["classes"])
    got = param_groups(m, F["weight_decay"], F["layer_decay"], trainable=which)
    assert [(g["name"], g["weight_decay"], g["lr_scale"], g["param_names"]) for g in got] == want
    params = dict(m.named_parameters())
    for g in got:
        assert all(p is params[n] for p, n in zip(g["params"], g["param_names"]))
    # the quirk of get_num_layer_for_vit: temporal_embed, norm.*, head.* share the LAST layer id, the embeddings layer 0
    by = {n: g["name"] for g in param_groups(m, F["weight_decay"], F["layer_decay"]) for n in g["param_names"]}
    last = S.TINY["depth"] + 1
    assert by["temporal_embed"] == f"layer_{last}_decay" and by["norm.weight"] == f"layer_{last}_no_decay"
    assert by["head.weight"] == f"layer_{last}_decay" and by["cls_token"] == "layer_0_no_decay" and by["patch_embed.proj.weight"] == "layer_0_decay"
    # the test-side restatement agrees too
    shapes = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    assert R.group_rule(shapes, F["weight_decay"], F["layer_decay"], S.TINY["depth"], trainable=which) == want
    # without layer decay the script assigns no layer ids (run_class_finetuning.py:372-376)
    assert [g["name"] for g in param_groups(m, 0.05, 1.0)] == ["no_decay", "decay"]


def test_vit_b_layer_decay_makes_28_groups():
    from tvts_amd.downstream.finetune_v1 import MAX_GROUPS, param_groups
    m = _Named(dict(S.TINY, depth=12), 5)
    g = param_groups(m, 0.05, 0.75)
    assert len(g) == 28 <= MAX_GROUPS and abs(g[0]["lr_scale"] - 0.75 ** 13) < 1e-15


@pytest.fixture(scope="module")
def helper_run(golden):
    f = golden("v1_finetune")
    sd = R.state()
    clip, targets = S.synth_clip(S.TINY, F["B"], F["T"], F["clip_seed"]), R.soft_targets(F["B"], F["classes"], F["target_seed"])
    tables = [torch.from_numpy(t) for t in f["tables"]]
    steps, final = R.train_run(sd, clip, targets, tables, clip_grad=float(f["clip_grad"]))
    return f, sd, steps, final


def test_helper_forward_loss_grads_equal_fixture(helper_run):
    f, sd, steps, final = helper_run
    names = [str(s) for s in f["param_names"]]
    assert names == list(sd.keys())
    for k, st in enumerate(steps):
        assert np.abs(st["logits"].numpy() - f["logits"][k]).max() < 1e-5 * max(1.0, np.abs(f["logits"][k]).max())
        assert abs(st["loss"] - f["loss"][k]) < 1e-5 * max(1.0, abs(f["loss"][k]))
        assert abs(st["grad_norm"] - f["grad_norm"][k]) < 1e-4 * f["grad_norm"][k]
        gn = np.array([float(st["grads"][n].double().norm()) for n in names])
        assert np.all(np.abs(gn - f["tensor_grad_norms"][k]) <= 1e-4 * f["tensor_grad_norms"][k] + 1e-7), k
    for n in R.FULL_GRADS:
        ref = f["grad." + n]
        assert np.abs(steps[0]["grads"][n].numpy() - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-7, n
    dn = np.array([float(R.delta_for_compare(n, final[n].double() - sd[n].double()).norm()) for n in names])
    for n in names:  # what delta_for_compare leaves out really is noise: the key bias gradient next to the query / value ones
        if n.endswith("attn.qkv.bias"):
            g = steps[0]["grads"][n]
            assert float(g[128:256].norm()) < 1e-5 * float(g.norm()), n
    assert np.all(np.abs(dn - f["delta_norms"]) <= 1e-4 * f["delta_norms"] + 1e-8)
    assert float(f["clip_grad"]) < f["grad_norm"][0]  # the clip binds in step 1


def test_fixture_tables_come_from_the_draw(golden):
    f = golden("v1_finetune")
    assert int(f["drop_seed"]) == F["drop_seed"]
    rates = R.site_rates(F["drop_path_rate"], S.TINY["depth"])
    for k in range(F["steps"]):
        t = R.draw_table(R.step_seed(F["drop_seed"], k + 1), rates, F["B"])
        assert t.tobytes() == f["tables"][k].tobytes()
    t1 = f["tables"][0][2:]
    assert (t1 == 0).any() and (t1 > 1).any() and (f["tables"][:, :2] == 1).all()


def test_integer_draw_properties():
    seed = R.step_seed(F["drop_seed"], 1)
    a = [R.draw_bits(seed, R.FT_SITE_BASE + 3, b) for b in range(64)]
    assert a == [R.draw_bits(seed, R.FT_SITE_BASE + 3, b) for b in range(64)]          # deterministic
    assert a != [R.draw_bits(seed, R.FT_SITE_BASE + 2, b) for b in range(64)]          # differs per site
    assert len(set(a)) == 64                                                           # ... and per sample
    assert a != [R.draw_bits(R.step_seed(F["drop_seed"], 2), R.FT_SITE_BASE + 3, b) for b in range(64)]  # ... and per step
    n = 4096
    for site in (0, 1, 23):
        kept = sum(R.draw_bits(seed, R.FT_SITE_BASE + site, b) >= 2 ** 31 for b in range(n))
        assert abs(kept / n - 0.5) <= 4 * 0.5 / n ** 0.5, (site, kept)                 # 4 standard deviations of a fair coin
    t = R.draw_table(seed, [0.0, 0.5], 16)
    assert (t[0] == 1.0).all() and set(np.unique(t[1])) <= {0.0, 2.0}
