"""CPU-side checks of the GEMM entry points' argument validation: every call of tests/gemm_cases.py::REFUSALS is one valid baseline
(BASELINES, each launched once by tests/test_gemm_edges_gpu.py) with exactly ONE argument changed, and is refused with -22 before
any HIP call (no GPU is present here; the pointers are dummy host buffers no refused call reads).  A wrong leading dimension that
is not refused is a silent wrong answer or an out-of-bounds access."""
import pytest

import gemm_cases as GC
from tvts_amd import _lib

ENTRY_POINTS = ("tvts_gemm_nt_bf16", "tvts_gemm_nt_fp8", "tvts_gemm_nt_fp8_gate", "tvts_gemm_tn_bf16", "tvts_gemm_tn_fp8",
                "tvts_rows_linear_bf16", "tvts_colsum_bf16")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _alloc(lib, keep):
    def alloc(m):
        if m == GC.NT_WS:
            p = GC.Mat(1, 1, GC.U8).dummy()
            keep.append(p)
            return p, lib.tvts_gemm_nt_workspace_bytes()
        p = m.dummy()
        keep.append(p)
        return p
    return alloc


def test_the_table_covers_every_entry_point_and_changes_one_argument():
    protos = _lib.parse_header()
    covered = {GC.BASELINES[name][0] for name, _, _, _ in GC.REFUSALS}
    assert covered == set(ENTRY_POINTS), covered ^ set(ENTRY_POINTS)
    for name, (fn, base) in GC.BASELINES.items():
        assert list(base) + ["stream"] == protos[fn][2], (name, list(base), protos[fn][2])  # the header's arguments, in its order
    seen = set()
    for name, arg, value, why in GC.REFUSALS:
        base = GC.BASELINES[name][1]
        assert arg in base and base[arg] != value and base[arg] is not value, (name, arg, value)
        assert (name, arg, value) not in seen, (name, arg, value)
        seen.add((name, arg, value))


@pytest.mark.parametrize("name,arg,value,why", GC.REFUSALS, ids=[f"{n}-{a}={v}" for n, a, v, _ in GC.REFUSALS])
def test_gemm_entry_points_refuse(lib, name, arg, value, why):
    keep = []
    rc = GC.call(lib, _lib.prototypes(), name, _alloc(lib, keep), **{arg: value})
    assert rc == -22, f"{GC.BASELINES[name][0]} ({name}) with {arg} = {value!r} returned {rc}: {why}"


def test_every_shorter_than_its_row_refusal_is_below_the_row_and_its_baseline_is_not():
    """table sanity: a refusal given as `ld < width` changes the leading dimension to a value below that width of the baseline,
    whose own leading dimension is not"""
    for name, arg, value, why in GC.REFUSALS:
        if " < " not in why:
            continue
        base = GC.BASELINES[name][1]
        width = why.split(" < ")[1].split()[0]
        if width not in base:  # (`workspace_elems < 0`: a sign, not a row)
            continue
        limit = base[width]
        assert value < limit <= base[arg], (name, arg, value, limit)
