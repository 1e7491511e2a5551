"""Shared cases of the e4m3 copy tests (a plain helper module, imported by the tests): an independent encoder that states the
kernels' contract, a fixed ladder of values at every rounding edge of the format, the scale kinds the ladder is used under, and
one table of valid baseline calls of the quantiser entry points with the single-argument changes each must refuse.

The contract of every e4m3-producing site (pack4_e4m3 of csrc/common.h, Q8Out::emit8 and the two CLS kernels of attention.hip,
patch_readout of gemm_nt256.h): v = fl32(x * inv) with inv = fl32(1 / scale), clamped to [-448, 448], rounded to nearest-even onto
OCP e4m3 (torch.float8_e4m3fn bit patterns: 4 exponent bits, bias 7, 3 mantissa bits, subnormals below 2^-6 in steps of 2^-9, no
infinities, 0x7F / 0xFF the NaNs).  Zero keeps its sign (-0 is 0x80).  The clamp is fminf(fmaxf(v, -448), 448): +-Inf give
+-448 (0x7E / 0xFE) and a NaN gives -448 (0xFE: fmaxf(NaN, -448) is -448), so no site ever writes 0x7F or 0xFF.

tests/test_fp8_cases_cpu.py holds the encoder to torch's own cast and the ladder to its claims without a GPU;
tests/test_fp8_copies_gpu.py holds every producer to the encoder byte for byte."""
import numpy as np
import torch

from gemm_cases import BF16, F32, U8, Mat

E4M3_MAX = 448.0
NAN_BYTE = 0xFE  # what the clamp makes of a NaN (see the module docstring)


# ------------------------------------------------------------------------------------------------ the encoder
def fl32(v):
    """a Python number rounded to fp32, as a Python float"""
    return float(np.float32(v))


def inv_of(scale):
    """fl32(1 / scale) as the kernels form it (a correctly rounded fp32 division); a scale <= 0 stands for 1.0"""
    s = np.float32(scale)
    if not s > 0:
        return 1.0
    return float(np.float32(1.0) / s)


def scale_of(amax):
    """fl32(amax / 448): the scale a quantiser or tvts_fp8_update_scales derives from a maximum (1.0 for a zero maximum)"""
    a = np.float32(amax)
    if not a > 0:
        return 1.0
    return float(np.float32(a) / np.float32(448.0))


def encode_e4m3(x, inv):
    """uint8 e4m3 bytes (on the CPU, x's shape) of the bf16 / fp32 tensor x under `inv` (a number, or an fp32-valued tensor that
    broadcasts against x: one reciprocal scale per row).  Integer and float64 arithmetic only: the product of two fp32 values is
    exact in float64 (48 significand bits), one rounding to fp32 makes it fl32(x * inv); the grid index is an exact float64 quotient
    by a power of two, rounded half to even by hand."""
    xd = x.detach().cpu().double()
    invd = inv.detach().cpu().double() if isinstance(inv, torch.Tensor) else torch.tensor(float(inv), dtype=torch.float64)
    assert bool((invd.float().double() == invd).all()), "inv must be an fp32 value"
    v = (xd * invd).float().double()                    # fl32(x * inv)
    nan = torch.isnan(v)
    neg = torch.signbit(v) | nan                        # the clamp turns a NaN into -448
    a = torch.where(nan, torch.full_like(v, E4M3_MAX), v.abs()).clamp(max=E4M3_MAX)
    _, e = torch.frexp(a)                               # a = m * 2^e, 0.5 <= m < 1: floor(log2 a) = e - 1
    E = torch.where(a < 2.0 ** -6, torch.full_like(e, -6), e - 1).long()  # binade of the grid (below 2^-6: the subnormal grid)
    q = a * torch.exp2((3 - E).double())                # a / 2^(E - 3): exact
    n = torch.floor(q)
    frac = q - n
    n = n.long()
    n = n + ((frac > 0.5) | ((frac == 0.5) & (n % 2 == 1))).long()
    code = (E + 7) * 8 + n - 8                          # n = 16 rolls into the next binade by itself; E = -6: code = n
    assert int(code.min()) >= 0 and int(code.max()) <= 0x7E
    return (code + 128 * neg.long()).to(U8)


def decode_code(b):
    """value of one finite e4m3 code 0x00 .. 0x7E (no sign bit), as a Python float"""
    assert 0 <= b <= 0x7E
    ex, man = b >> 3, b & 7
    return man * 2.0 ** -9 if ex == 0 else (8 + man) * 2.0 ** (ex - 10)


# ------------------------------------------------------------------------------------------------ the ladder
def _ulp_neighbours(vals, dtype):
    """the next value of `dtype` below and above each (positive) value"""
    it = {BF16: torch.int16, F32: torch.int32}[dtype]
    t = torch.tensor(vals, dtype=torch.float64).to(dtype)
    assert bool((t.double() == torch.tensor(vals, dtype=torch.float64)).all()), "not exact in " + str(dtype)
    bits = t.view(it)
    return (bits - 1).view(dtype).double().tolist(), (bits + 1).view(dtype).double().tolist()


def ladder_parts(dtype):
    """the positive half of the ladder by kind -> dict of lists of Python floats (all exact in dtype):
    codes      the 126 positive finite code values (0x01 .. 0x7E)
    mids       the 126 midpoints between neighbouring codes 0x00 .. 0x7E (2^-10, the first, is the tie that rounds to 0;
               3 * 2^-10 the one that rounds to 0x02)
    below / above   each midpoint minus / plus one ulp of dtype (for fp32 also minus / plus one bf16 ulp)
    tiny       a bf16 subnormal (2^-130)
    past       values beyond the range: 464 (the midpoint of 448 and the 480 the format has no code for), one ulp above it, 480, 1e4,
               the maximum of bf16"""
    codes = [decode_code(b) for b in range(1, 0x7F)]
    grid = [0.0] + codes
    mids = [(a + b) / 2 for a, b in zip(grid, grid[1:])]
    below, above = _ulp_neighbours(mids, dtype)
    if dtype == F32:
        b16, a16 = _ulp_neighbours(mids, BF16)
        below, above = below + b16, above + a16
    past = [464.0, _ulp_neighbours([464.0], dtype)[1][0], 480.0, float(torch.tensor(1e4).to(dtype)), float(torch.finfo(BF16).max)]
    return dict(codes=codes, mids=mids, below=below, above=above, tiny=[2.0 ** -130], past=past)


def ladder(dtype, past=True):
    """the fixed value ladder in both signs, a 1-D tensor of dtype padded with zeros to a multiple of 8 (about 1 050 values; see
    ladder_parts; +0 and -0 included).  past=False: without the values beyond +-448 (rows of the per-row mode, whose scale comes
    from their own maximum)"""
    p = ladder_parts(dtype)
    pos = p["codes"] + p["mids"] + p["below"] + p["above"] + p["tiny"] + (p["past"] if past else [])
    vals = [0.0, -0.0] + pos + [-v for v in pos]
    vals += [0.0] * (-len(vals) % 8)
    t = torch.tensor(vals, dtype=torch.float64)
    out = t.to(dtype)
    assert bool((out.double() == t).all()), "a ladder value is not exact in " + str(dtype)
    return out


# Scale kinds.  Under a power of two x * inv is exact, so the expected byte of ladder * s under the scale s is the byte of the ladder
# value itself and cannot be argued with; the two others exercise the fp32 reciprocal and the rounding of the fp32 product.
POW2_SCALES = [1.0, 2.0 ** -3, 2.0 ** 5]
ODD_SCALES = [fl32(0.05), fl32(3.3)]
SCALES = POW2_SCALES + ODD_SCALES


def scaled(t, s):
    """ladder values times the scale s in t's dtype: exact for a power of two (asserted), rounded once otherwise; a product past the
    type's range stays at the type's maximum (it saturates like every other value past 448 s)"""
    fmax = float(torch.finfo(t.dtype).max)
    d = (t.double() * s).clamp(-fmax, fmax)
    out = d.to(t.dtype)
    if s in POW2_SCALES:
        ok = (out.double() == d) | (d.abs() == fmax)
        assert bool(ok.all()), "a power-of-two scaling is not exact"
    return out


def fill_cyclic(rows, cols, vals, offset=0):
    """[rows, cols] of vals' dtype: vals repeated row-major, the first one at flat position `offset` (zeros before it) -- with an
    offset that is no multiple of 8 the ladder's groups straddle the 16-byte pieces a lane converts"""
    n = rows * cols
    flat = torch.zeros(n, dtype=vals.dtype)
    k = max(0, n - offset)
    reps = -(-k // vals.numel())
    flat[offset:] = vals.repeat(reps)[:k]
    return flat.view(rows, cols)


def row_ladders(rows, cols, dtype=BF16, zero_row=None):
    """rows for the per-row mode: the in-range ladder repeated row-major, row r times 2^k_r (k_r = r % 7 - 3), one element of every
    row set to +-448 * 2^k_r so that the row's scale is exactly 2^k_r and its reciprocal exact; zero_row: that row all zero
    (scale 1, zero bytes).  -> (x, k) with k the exponents as a LongTensor"""
    base = fill_cyclic(rows, cols, ladder(dtype, past=False), offset=3).double()
    r = torch.arange(rows)
    k = r % 7 - 3
    base[r, (5 * r + 1) % cols] = E4M3_MAX * (1.0 - 2.0 * (r % 2).double())
    x = base * torch.exp2(k.double())[:, None]
    if zero_row is not None:
        x[zero_row] = 0.0
        k[zero_row] = 0
    out = x.to(dtype)
    assert bool((out.double() == x).all())
    return out, k


# ------------------------------------------------------------------------------------------------ baselines and refusals
# One valid call per entry point (launched once each by tests/test_fp8_copies_gpu.py) and the single-argument changes that must
# come back with -22 before any launch (tests/test_fp8_cases_cpu.py calls them without a GPU).
TABLE = "table"  # stands for a device table of tvts_quant_fp8_multi records


def _amax(**kw):
    d = dict(x=Mat(5, 24, BF16), is_f32=0, ld=24, rows=5, cols=16, amax=Mat(1, 1, F32))
    d.update(kw)
    return d


def _quant(**kw):
    d = dict(x=Mat(5, 24, BF16), is_f32=0, ld=24, rows=5, cols=16, amax=Mat(1, 1, F32, 3.0), out=Mat(5, 24, U8, "zero"), ldo=24,
             scale_out=Mat(1, 1, F32))
    d.update(kw)
    return d


def _rows(**kw):
    d = dict(x=Mat(5, 24, BF16), ld=24, rows=5, cols=16, out=Mat(5, 24, U8, "zero"), ldo=24, row_scale=Mat(1, 5, F32), tscale=None,
             amax_acc=None)
    d.update(kw)
    return d


BASELINES = {
    "amax": ("tvts_amax", _amax()),
    "amax_f32": ("tvts_amax", _amax(x=Mat(5, 24, F32), is_f32=1, cols=12)),
    "quant": ("tvts_quant_fp8", _quant()),
    "quant_f32": ("tvts_quant_fp8", _quant(x=Mat(5, 24, F32), is_f32=1, cols=12)),
    "rows": ("tvts_quant_fp8_rows", _rows()),
    "rows_tensor": ("tvts_quant_fp8_rows", _rows(row_scale=None, tscale=Mat(1, 1, F32, 0.5), amax_acc=Mat(1, 1, F32, "zero"))),
    "multi": ("tvts_quant_fp8_multi", dict(table=TABLE, n=2)),
    "update": ("tvts_fp8_update_scales", dict(amax=Mat(1, 3, F32, 2.0), scale=Mat(1, 3, F32, 1.0), n=3)),
}

REFUSALS = [
    # ---- tvts_amax
    ("amax", "cols", 12, "cols % 8 (bf16)"), ("amax_f32", "cols", 6, "cols % 4 (fp32)"), ("amax", "cols", 0, "cols <= 0"),
    ("amax", "ld", 20, "ld off a 16-byte multiple (bf16)"), ("amax_f32", "ld", 18, "ld off a 16-byte multiple (fp32)"),
    ("amax", "ld", 8, "ld < cols"), ("amax", "rows", 0, "rows <= 0"), ("amax", "rows", -1, "rows <= 0"),
    ("amax", "x", None, "null x"), ("amax", "amax", None, "null amax"),
    # ---- tvts_quant_fp8
    ("quant", "cols", 12, "cols % 8 (bf16)"), ("quant_f32", "cols", 6, "cols % 4 (fp32)"), ("quant", "cols", 0, "cols <= 0"),
    ("quant", "ld", 20, "ld off a 16-byte multiple (bf16)"), ("quant_f32", "ld", 18, "ld off a 16-byte multiple (fp32)"),
    ("quant", "ldo", 20, "ldo off an 8-byte multiple"), ("quant", "ld", 8, "ld < cols"), ("quant", "ldo", 8, "ldo < cols"),
    ("quant", "rows", 0, "rows <= 0"), ("quant", "rows", -1, "rows <= 0"), ("quant", "x", None, "null x"), ("quant", "out", None, "null out"),
    ("quant", "amax", None, "null amax"),
    # ---- tvts_quant_fp8_rows
    ("rows", "cols", 12, "cols % 8"), ("rows", "cols", 0, "cols <= 0"), ("rows", "ld", 20, "ld off a 16-byte multiple"),
    ("rows", "ldo", 20, "ldo off an 8-byte multiple"), ("rows", "ld", 8, "ld < cols"), ("rows", "ldo", 8, "ldo < cols"),
    ("rows", "rows", 0, "rows <= 0"), ("rows", "rows", -1, "rows <= 0"), ("rows", "x", None, "null x"), ("rows", "out", None, "null out"),
    ("rows", "row_scale", None, "neither row_scale nor tscale"), ("rows_tensor", "tscale", None, "neither row_scale nor tscale"),
    # ---- tvts_quant_fp8_multi
    ("multi", "table", None, "null table"), ("multi", "n", 0, "n <= 0"), ("multi", "n", -1, "n <= 0"),
    # ---- tvts_fp8_update_scales
    ("update", "n", 0, "n <= 0"), ("update", "n", -1, "n <= 0"), ("update", "amax", None, "null amax"), ("update", "scale", None, "null scale"),
]


def call(lib, protos, name, alloc, stream=None, **change):
    """the baseline `name` with the arguments of `change` replaced -> the entry point's return code.  alloc(Mat) -> a pointer,
    alloc(TABLE) -> a pointer to a table of the baseline's n records"""
    fn, base = BASELINES[name]
    args = dict(base)
    bad = set(change) - set(args)
    assert not bad, (name, bad)
    args.update(change)
    vals = []
    for an in protos[fn][2]:
        if an == "stream":
            vals.append(stream)
            continue
        v = args[an]
        vals.append(alloc(v) if isinstance(v, Mat) or (isinstance(v, str) and v == TABLE) else v)
    return getattr(lib, fn)(*vals)
