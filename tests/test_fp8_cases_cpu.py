"""CPU-side checks of tests/fp8_cases.py: the independent e4m3 encoder against torch's own cast at every code, midpoint and
neighbour, the claims of the value ladder, and the argument validation of the quantiser entry points -- every call of REFUSALS is
one valid baseline (BASELINES, each launched once by tests/test_fp8_copies_gpu.py) with exactly ONE argument changed, and is
refused with -22 before any HIP call (no GPU is present here; the pointers are dummy host buffers no refused call reads)."""
import pytest
import torch

import fp8_cases as FC
from tvts_amd import _lib

BF16, F32, U8 = FC.BF16, FC.F32, FC.U8
ENTRY_POINTS = ("tvts_amax", "tvts_quant_fp8", "tvts_quant_fp8_rows", "tvts_quant_fp8_multi", "tvts_fp8_update_scales")


def _torch_bytes(x, inv=1.0):
    return (x.float() * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(U8)


def _both_signs(vals, dtype):
    t = torch.tensor(vals, dtype=torch.float64).to(dtype)
    assert bool((t.double() == torch.tensor(vals, dtype=torch.float64)).all())
    return torch.cat([t, -t])


# ------------------------------------------------------------------------------------------------ the encoder
def test_every_finite_code_encodes_to_itself_and_matches_torch():
    codes = torch.arange(256, dtype=torch.int64)
    codes = codes[(codes & 0x7F) != 0x7F].to(U8)                       # the 254 finite codes, both zeros included
    assert codes.numel() == 254
    vals = codes.view(torch.float8_e4m3fn).float()
    for dtype in (BF16, F32):
        x = vals.to(dtype)
        assert torch.equal(x.float(), vals)                             # 4 significand bits: exact in bf16
        got = FC.encode_e4m3(x, 1.0)
        assert torch.equal(got, codes), "a code does not encode to itself"
        assert torch.equal(got, _torch_bytes(x))
    assert [FC.decode_code(b) for b in range(0x7F)] == vals[:0x7F].double().tolist()


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_midpoints_round_to_the_even_code_and_their_neighbours_to_the_odd_one(dtype):
    p = FC.ladder_parts(dtype)
    mids = _both_signs(p["mids"], dtype)
    got = FC.encode_e4m3(mids, 1.0)
    assert torch.equal(got, _torch_bytes(mids)), "midpoints against torch"
    assert bool((got % 2 == 0).all()), "a midpoint did not round to the even code"
    lo = torch.arange(126, dtype=torch.int64)                           # midpoint i lies between the codes i and i + 1
    even = torch.where(lo % 2 == 0, lo, lo + 1)
    assert torch.equal(got[:126].long(), even) and torch.equal(got[126:].long(), even + 128)
    for name in ("below", "above"):
        nb = _both_signs(p[name], dtype)
        g = FC.encode_e4m3(nb, 1.0)
        assert torch.equal(g, _torch_bytes(nb)), name + " against torch"
        want = (lo if name == "below" else lo + 1).repeat(len(p[name]) // 126)
        assert torch.equal(g[:len(p[name])].long(), want) and torch.equal(g[len(p[name]):].long(), want + 128), name
    # the subnormal edges by name
    e = FC.encode_e4m3(torch.tensor([2.0 ** -10, p["above"][0], 3 * 2.0 ** -10, -2.0 ** -10, 0.0, -0.0, 2.0 ** -130, -2.0 ** -130],
                                    dtype=torch.float64).to(dtype), 1.0)
    assert e.tolist() == [0x00, 0x01, 0x02, 0x80, 0x00, 0x80, 0x00, 0x80]


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("s", FC.SCALES)
def test_the_encoder_matches_torch_on_the_ladder_under_every_scale(dtype, s):
    x = FC.scaled(FC.ladder(dtype), s)
    inv = FC.inv_of(s)
    got = FC.encode_e4m3(x, inv)
    assert torch.equal(got, _torch_bytes(x, torch.tensor(inv, dtype=F32)))
    assert 0x7F not in got.tolist() and 0xFF not in got.tolist()
    if s in FC.POW2_SCALES:                                             # x * inv is exact: the bytes of the ladder itself
        ok = x.double().abs() < float(torch.finfo(dtype).max)           # (but for products that stopped at the type's maximum)
        assert torch.equal(got[ok], FC.encode_e4m3(FC.ladder(dtype), 1.0)[ok])


def test_values_past_the_range_and_non_finite_values_saturate():
    for dtype in (BF16, F32):
        past = _both_signs(FC.ladder_parts(dtype)["past"], dtype)
        got = FC.encode_e4m3(past, 1.0)
        assert got.tolist() == [0x7E] * 5 + [0xFE] * 5
        assert torch.equal(got, _torch_bytes(past))
        nf = torch.tensor([float("inf"), float("-inf"), float("nan")], dtype=dtype)
        assert FC.encode_e4m3(nf, 1.0).tolist() == [0x7E, 0xFE, FC.NAN_BYTE]
        assert FC.encode_e4m3(nf, FC.inv_of(0.05)).tolist() == [0x7E, 0xFE, FC.NAN_BYTE]


def test_per_row_reciprocals_broadcast():
    x, k = FC.row_ladders(9, 16)
    inv = torch.exp2(-k.double()).float()[:, None]
    got = FC.encode_e4m3(x, inv)
    assert torch.equal(got, _torch_bytes(x, inv))
    for r in range(9):
        assert torch.equal(got[r], FC.encode_e4m3(x[r], float(inv[r])))


# ------------------------------------------------------------------------------------------------ the ladder
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_the_ladder_covers_every_finite_code_and_every_edge(dtype):
    lad = FC.ladder(dtype)
    assert lad.numel() % 8 == 0 and 1000 <= lad.numel() <= 2100 and lad.dtype == dtype
    b = FC.encode_e4m3(lad, 1.0)
    seen = set(b.tolist())
    want = {c for c in range(256) if c & 0x7F != 0x7F}
    assert seen == want, sorted(want - seen)                            # each of the 254 finite codes at least once, never a NaN code
    signs = torch.signbit(lad)
    assert bool((lad[signs] == 0).any()) and bool((lad[~signs] == 0).any())  # both zeros
    assert bool(((lad.double().abs() > 0) & (lad.double().abs() < 2.0 ** -126)).any())  # a bf16 subnormal
    for v in (464.0, 480.0, float(torch.finfo(BF16).max)):
        assert bool((lad.double() == v).any()) and bool((lad.double() == -v).any())
    inr = FC.ladder(dtype, past=False)
    assert float(inr.double().abs().max()) == 448.0 and inr.numel() % 8 == 0
    assert set(FC.encode_e4m3(inr, 1.0).tolist()) == want


def test_row_ladders_carry_their_scale_exactly():
    for rows, cols in ((1, 8), (5, 8), (4, 5128)):
        x, k = FC.row_ladders(rows, cols, zero_row=2 if rows > 2 else None)
        am = x.double().abs().amax(1)
        want = 448.0 * torch.exp2(k.double())
        if rows > 2:
            want[2] = 0.0
        assert torch.equal(am, want)
        assert [FC.scale_of(a) for a in am.tolist()] == [2.0 ** int(e) for e in k.tolist()]
    x, _ = FC.row_ladders(150, 8)
    inv = torch.exp2(-(torch.arange(150) % 7 - 3).double()).float()[:, None]
    assert len(set(FC.encode_e4m3(x, inv).flatten().tolist())) == 254


def test_fill_cyclic_starts_the_ladder_off_a_lane_boundary():
    lad = FC.ladder(BF16)
    m = FC.fill_cyclic(3, 1056, lad, offset=3)
    flat = m.flatten()
    assert torch.equal(flat[:3], torch.zeros(3, dtype=BF16)) and torch.equal(flat[3:3 + lad.numel()].view(torch.int16), lad.view(torch.int16))
    assert torch.equal(flat[3 + lad.numel():3 + lad.numel() + 5].view(torch.int16), lad[:5].view(torch.int16))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _alloc(keep):
    def alloc(m):
        p = FC.Mat(1, 1, U8).dummy() if isinstance(m, str) else m.dummy()
        keep.append(p)
        return p
    return alloc


def test_the_table_covers_every_entry_point_and_changes_one_argument():
    protos = _lib.parse_header()
    covered = {FC.BASELINES[name][0] for name, _, _, _ in FC.REFUSALS}
    assert covered == set(ENTRY_POINTS), covered ^ set(ENTRY_POINTS)
    assert {fn for fn, _ in FC.BASELINES.values()} == set(ENTRY_POINTS)
    for name, (fn, base) in FC.BASELINES.items():
        assert list(base) + ["stream"] == protos[fn][2], (name, list(base), protos[fn][2])  # the header's arguments, in its order
    seen = set()
    for name, arg, value, why in FC.REFUSALS:
        base = FC.BASELINES[name][1]
        assert arg in base and base[arg] != value and base[arg] is not value, (name, arg, value)
        assert (name, arg, value) not in seen, (name, arg, value)
        seen.add((name, arg, value))
        if " < cols" in why:
            assert value < base["cols"] <= base[arg] and value % 8 == 0, (name, arg, value)  # (passes the alignment rule)


@pytest.mark.parametrize("name,arg,value,why", FC.REFUSALS, ids=[f"{n}-{a}={v}" for n, a, v, _ in FC.REFUSALS])
def test_quantiser_entry_points_refuse(lib, name, arg, value, why):
    keep = []
    rc = FC.call(lib, _lib.prototypes(), name, _alloc(keep), **{arg: value})
    assert rc == -22, f"{FC.BASELINES[name][0]} ({name}) with {arg} = {value!r} returned {rc}: {why}"
