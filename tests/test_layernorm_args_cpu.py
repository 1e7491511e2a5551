"""CPU-side checks of the LayerNorm entry points' argument validation: every call of tests/ln_cases.py::REFUSALS is one valid
baseline (BASELINES, each launched once by tests/test_layernorm_edges_gpu.py) with exactly ONE argument changed, and is refused with
-22 before any HIP call (no GPU is present here; the pointers are dummy host buffers no refused call reads).  A leading dimension
shorter than the row makes rows overlap: a silent wrong answer or an out-of-bounds access; a missing mean / rstd / dbeta is a
kernel's read or atomic through a null pointer."""
import pytest

import ln_cases as LC
from tvts_amd import _lib

ENTRY_POINTS = ("tvts_layernorm_fwd", "tvts_layernorm_fwd_fp8", "tvts_layernorm_fwd_cls", "tvts_layernorm_bwd", "tvts_layernorm_bwd_fp8",
                "tvts_layernorm_bwd_cls")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _alloc(keep):
    def alloc(m):
        p = m.dummy()
        keep.append(p)
        return p
    return alloc


def test_the_table_covers_every_entry_point_and_changes_one_argument():
    protos = _lib.parse_header()
    assert {n for n in protos if n.startswith("tvts_layernorm")} == set(ENTRY_POINTS)
    covered = {LC.BASELINES[name][0] for name, _, _, _ in LC.REFUSALS}
    assert covered == set(ENTRY_POINTS), covered ^ set(ENTRY_POINTS)
    assert {fn for fn, _ in LC.BASELINES.values()} == set(ENTRY_POINTS)
    for name, (fn, base) in LC.BASELINES.items():
        assert list(base) + ["stream"] == protos[fn][2], (name, list(base), protos[fn][2])  # the header's arguments, in its order
    seen = set()
    for name, arg, value, why in LC.REFUSALS:
        base = LC.BASELINES[name][1]
        assert arg in base and base[arg] != value and base[arg] is not value, (name, arg, value)
        assert (name, arg, value) not in seen, (name, arg, value)
        seen.add((name, arg, value))


@pytest.mark.parametrize("name,arg,value,why", LC.REFUSALS, ids=[f"{n}-{a}={v}" for n, a, v, _ in LC.REFUSALS])
def test_layernorm_entry_points_refuse(lib, name, arg, value, why):
    keep = []
    rc = LC.call(lib, _lib.prototypes(), name, _alloc(keep), **{arg: value})
    assert rc == -22, f"{LC.BASELINES[name][0]} ({name}) with {arg} = {value!r} returned {rc}: {why}"


def test_every_shorter_than_its_row_refusal_is_below_the_row_and_its_baseline_is_not():
    """table sanity: a refusal given as `ld < W` changes the leading dimension to a value below the width of the baseline, whose
    own leading dimension is not; every leading dimension of every entry point has one, wherever its matrix is given"""
    short = set()
    for name, arg, value, why in LC.REFUSALS:
        if " < W" not in why:
            continue
        base = LC.BASELINES[name][1]
        assert value < base["W"] <= base[arg] and value % 4 == 0, (name, arg, value)
        short.add((LC.BASELINES[name][0], arg))
    protos = _lib.parse_header()
    want = {(fn, a) for fn in ENTRY_POINTS for a in protos[fn][2] if a.startswith("ld")}
    assert short == want, short ^ want


def test_the_new_refusals_need_the_new_checks():
    """each refusal that is not a pin has a reason no pinned check gives: its value passes the % 4 rule"""
    for name, arg, value, why in LC.REFUSALS:
        if not why.startswith("pin") and arg.startswith("ld"):
            assert value % 4 == 0, (name, arg, value)
