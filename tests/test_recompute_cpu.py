"""Activation recomputation: what needs no device -- the mode validation and the e4m3 refusals (tvts_amd/arch.py), the mapping of
set_grad_checkpointing's argument and of the `grad_checkpointing` entry of the reference's args to a mode, and the slot naming."""
import types

import pytest
import torch

from tvts_amd import arch as A


def test_modes_and_the_argument_of_set_grad_checkpointing():
    assert A.RECOMPUTE_MODES == ("none", "mlp", "block")
    assert A.recompute_mode(True) == "block" and A.recompute_mode(False) == "none" and A.recompute_mode(None) == "none"
    for mode in A.RECOMPUTE_MODES:
        assert A.recompute_mode(mode) == mode
    for bad in ("blocks", "", "full", 1, 0, 2.0, ("block",)):
        with pytest.raises(ValueError, match="recompute mode"):
            A.recompute_mode(bad)
    with pytest.raises(ValueError, match="'attention'"):  # the unknown mode by name
        A.recompute_mode("attention")


def test_missing_key_is_none_and_unknown_modes_are_refused():
    a = A.small_arch()
    assert "recompute" not in a and A.check_recompute(a) == "none"
    assert A.check_recompute(dict(a, recompute="none")) == "none"
    assert A.check_recompute(dict(a, recompute="mlp")) == "mlp"
    assert A.check_recompute(dict(a, recompute="block")) == "block"
    assert A.check_recompute(dict(a, recompute=True)) == "block"
    assert A.check_recompute(a, "mlp") == "mlp" and "recompute" not in a  # (an explicit mode: the dict is only read)
    with pytest.raises(ValueError, match="'layer'"):
        A.check_recompute(dict(a, recompute="layer"))
    with pytest.raises(ValueError, match="'layer'"):
        A.check_recompute(a, "layer")


@pytest.mark.parametrize("key", ["fp8", "fp8_dgrad", "fp8_wgrad"])
@pytest.mark.parametrize("mode", ["mlp", "block"])
def test_e4m3_architectures_are_refused_by_name(key, mode):
    a = A.small_arch_h(**{key: True})
    assert A.check_recompute(a) == "none" and A.check_recompute(dict(a, recompute="none")) == "none"
    with pytest.raises(ValueError, match=key):
        A.check_recompute(dict(a, recompute=mode))
    with pytest.raises(ValueError, match=key):  # ... and when the mode arrives later (set_grad_checkpointing)
        A.check_recompute(a, mode)
    assert A.check_recompute(dict(a, **{key: False}), mode) == mode


def test_engine_refuses_at_construction():
    """Engine.__init__ runs the same check (a store on the CPU is enough to get there; fp8_wgrad switches the other two on)"""
    from tvts_amd.engine import Engine, ParamStore
    for over, word in ((dict(recompute="columns"), "'columns'"), (dict(recompute="block", fp8=True), "fp8"),
                       (dict(recompute="mlp", fp8_dgrad=True), "fp8_dgrad"), (dict(recompute="block", fp8_wgrad=True), "fp8")):
        with pytest.raises(ValueError, match=word):
            Engine(ParamStore(A.small_arch(layers=1, text_layers=1, **over), torch.device("cpu")))
    eng = Engine(ParamStore(A.small_arch(layers=1, text_layers=1, recompute="mlp"), torch.device("cpu")))
    assert eng.recompute == "mlp" and eng.recompute_count == 0 and eng.workspace_bytes() == 0
    eng.set_recompute("block")
    assert eng.recompute == "block" and eng.arch["recompute"] == "block"
    with pytest.raises(ValueError, match="'both'"):
        eng.set_recompute("both")
    assert eng.recompute == "block"
    assert Engine(ParamStore(A.small_arch(layers=1, text_layers=1), torch.device("cpu"))).recompute == "none"


def test_grad_checkpointing_of_the_reference_args():
    a = A.small_arch()
    ns = types.SimpleNamespace
    assert A.recompute_from_args(ns(local_rank=0), a) == "none"
    assert A.recompute_from_args(None, a) == "none"
    assert A.recompute_from_args({}, a) == "none"
    assert A.recompute_from_args(ns(grad_checkpointing=True), a) == "block"
    assert A.recompute_from_args(ns(grad_checkpointing=False), a) == "none"
    assert A.recompute_from_args(ns(grad_checkpointing="mlp"), a) == "mlp"
    assert A.recompute_from_args({"grad_checkpointing": True, "n_gpu": 8}, a) == "block"
    assert A.recompute_from_args({"grad_checkpointing": "mlp"}, a) == "mlp"
    assert A.recompute_from_args(ns(args={"grad_checkpointing": True}), a) == "block"  # the namespace that carries arch.args
    # an explicit arch["recompute"] wins
    assert A.recompute_from_args(ns(grad_checkpointing=True), dict(a, recompute="none")) == "none"
    assert A.recompute_from_args({"grad_checkpointing": False}, dict(a, recompute="mlp")) == "mlp"
    with pytest.raises(ValueError, match="'yes'"):
        A.recompute_from_args(ns(grad_checkpointing="yes"), a)


def test_slot_names():
    """"block": every tensor of a block in the shared slot; "mlp": the MLP pair alone; one slot per layer parity beside the side stream"""
    from tvts_amd.engine import Engine
    tags = Engine._rc_tags
    assert tags("vit", 4, "none") == ("vit4", "vit4") == tags("vit", 4, "none", parity=True)
    assert tags("vit", 4, "block") == ("vit.rc", "vit.rc") == tags("vit", 5, "block")
    assert tags("ft", 4, "mlp") == ("ft4", "ft.rc")
    assert tags("vit", 4, "block", parity=True) == ("vit.rc0", "vit.rc0") and tags("vit", 5, "block", parity=True)[0] == "vit.rc1"
    assert tags("vit", 3, "mlp", parity=True) == ("vit3", "vit.rc1")
