"""MXFP8 on the host: a float64 reference of the quantiser that owes nothing to torch's float8 type, the boundary inputs that the GPU
tests (test_gpu_mx8.py) feed to the HIP quantiser, the oracle against that reference on those inputs, and the refusals of gemm_mx8 /
quantize_mx8 in front of their first HIP call.

Reference (ref_quantize_mx8): the 127 finite non-negative e4m3fn magnitudes decoded from their bytes (exponent 0: m 2^-9, else
(8 + m) 2^(e - 10)); per block of 32 the scale byte is the smallest sb >= 0 with amax <= 448 2^(sb - 127), found by comparing amax with
the 256 thresholds in float64 (all exact); an element is x 2^(127 - sb) (exact in float64), saturated at 448, rounded to the nearest
magnitude by comparing with the midpoint of its two neighbours (exact), a tie going to the even code; the sign bit is kept, so -0.0
gives 0x80.  Non-finite inputs are outside the format's contract (oracle/mx_oracle.py) and the reference refuses them.

Boundary inputs.  Rounding (boundary_rows): the 127 magnitudes, the 126 midpoints between neighbours and each midpoint's two neighbours
in the input type (fp32 or bf16), both signs: 1010 points, 31 to a block beside one element that pins the block's scale (448, or the
largest finite value of the type where 448 2^(sb - 127) overflows), the pin at position b mod 32 of block b (33 blocks: every lane and
slot carries the amax), the pin's sign alternating; one row of 33 blocks per scale byte in SBS, the whole row times 2^(sb - 127).  A
point whose scaled value is not exactly an fp32 (bf16) number - at sb 0 and 1 the subnormal range cuts bits, at 247 the large ones
overflow - becomes 0; float64 arithmetic alone decides.  Scale (scale_rows): for every biased exponent 1..254 and mantissa 0, 0x600000,
0x600001, 0x7FFFFF (all finite) and for exponent 0 with mantissa 1, 0x400000, 0x600001, 0x7FFFFF one block whose amax is that fp32
value, at position b mod 32 with alternating sign, the other elements amax 2^-j, j = 1..31 (rounded to fp32)."""
import time

import pytest
import torch

from test_gpu_resid_ln import DUMMY, L_cpu, _refused  # noqa: F401  (L_cpu is a fixture)

SBS = (0, 1, 8, 119, 127, 135, 200, 246, 247)


@pytest.fixture(autouse=True)
def _timed(request):
    t = time.perf_counter()
    yield
    print(f"time {request.node.name}: {time.perf_counter() - t:.2f} s")


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def e4m3_table():
    """the 127 finite non-negative e4m3fn magnitudes in code order (float64), decoded from the bytes 0..126"""
    b = torch.arange(127)
    e, m = b >> 3, (b & 7).double()
    return torch.where(e == 0, m * 2.0 ** -9, (8 + m) * torch.exp2((e - 10).double()))


def _pow2(k):
    """2^k in float64 for an integer tensor k in the normal range, built from its bits"""
    assert int(k.min()) > -1022 and int(k.max()) < 1024
    return ((k.long() + 1023) << 52).view(torch.float64)


def ref_quantize_mx8(x):
    """x [..., K] fp32 or bf16, finite -> (e4m3 bytes [..., K], e8m0 bytes [..., K/32]), uint8; see the module docstring"""
    x = torch.as_tensor(x)
    assert x.dtype in (torch.float32, torch.bfloat16) and bool(torch.isfinite(x).all())
    K = x.shape[-1]
    blk = x.double().reshape(*x.shape[:-1], K // 32, 32)
    amax = blk.abs().amax(-1)
    fits = 448.0 * _pow2(torch.arange(256) - 127)                     # fits[sb] = 448 2^(sb - 127), exact
    sb = torch.searchsorted(fits, amax.contiguous())                  # the first sb with amax <= fits[sb]
    assert int(sb.max()) <= 254
    y = (blk * _pow2(127 - sb)[..., None]).abs().clamp_max(448.0)
    T = e4m3_table()
    hi = torch.searchsorted(T, y.contiguous()).clamp_min(1)           # T[hi - 1] <= y <= T[hi] (y = 0: codes 0 and 1)
    lo = hi - 1
    mid = (T[lo] + T[hi]) / 2                                         # at most 5 significant bits: exact
    code = torch.where(y > mid, hi, torch.where(y < mid, lo, torch.where(lo % 2 == 0, lo, hi)))
    code = code + 128 * torch.signbit(blk).long()
    return code.to(torch.uint8).reshape(x.shape), sb.to(torch.uint8)


# ---- boundary inputs ---------------------------------------------------------------------------------------------------------------------
def _neighbours(v, dtype):
    """the numbers of `dtype` next below and above the positive values v (exact in dtype)"""
    it = torch.int32 if dtype == torch.float32 else torch.int16
    bits = v.to(dtype).view(it)
    assert torch.equal(v.to(dtype).double(), v) and bool((v > 0).all())
    return (bits - 1).view(dtype).double(), (bits + 1).view(dtype).double()


def rounding_points(dtype):
    T = e4m3_table()
    mid = (T[:-1] + T[1:]) / 2
    below, above = _neighbours(mid, dtype)
    p = torch.cat([T, mid, below, above])
    p = torch.cat([p, -p])
    assert p.numel() == 1010
    return p


def boundary_rows(dtype):
    """[len(SBS), 33 * 32] of `dtype`: row i holds the rounding points at scale byte SBS[i] (module docstring)"""
    p = rounding_points(dtype)
    nb = -(-p.numel() // 31)
    assert nb == 33
    big = float(torch.finfo(dtype).max)
    rows = []
    for sb in SBS:
        scale = 2.0 ** (sb - 127)
        blocks = torch.zeros(nb, 32, dtype=torch.float64)
        pts = torch.cat([p, torch.zeros(nb * 31 - p.numel(), dtype=torch.float64)]).reshape(nb, 31) * scale
        exact = torch.isfinite(pts.to(dtype)) & (pts.to(dtype).double() == pts)
        pts = torch.where(exact, pts, torch.zeros_like(pts))
        for b in range(nb):
            pos = b % 32
            pin = min(448.0 * scale, big) * (-1.0 if b % 2 else 1.0)
            blocks[b] = torch.cat([pts[b, :pos], torch.tensor([pin], dtype=torch.float64), pts[b, pos:]])
        assert bool((blocks.abs().amax(-1) == abs(pin)).all())
        rows.append(blocks.reshape(-1))
    x = torch.stack(rows)
    assert torch.equal(x.to(dtype).double(), x)
    return x.to(dtype)


SCALE_MANTISSAS = (0, 0x600000, 0x600001, 0x7FFFFF)
SUBNORMAL_MANTISSAS = (1, 0x400000, 0x600001, 0x7FFFFF)


def scale_rows():
    """[255, 128] fp32: 1020 blocks whose amax walks the scale rule's boundaries (module docstring)"""
    bits = [(e << 23) | m for e in range(1, 255) for m in SCALE_MANTISSAS] + list(SUBNORMAL_MANTISSAS)
    amax = torch.tensor(bits, dtype=torch.int32).view(torch.float32).double()
    assert bool(torch.isfinite(amax).all()) and amax.numel() == 1020
    rest = (amax[:, None] * _pow2(-torch.arange(1, 32))[None, :]).float().double()      # amax 2^-j, rounded to fp32
    blocks = torch.empty(1020, 32, dtype=torch.float64)
    for b in range(1020):
        pos = b % 32
        blocks[b] = torch.cat([rest[b, :pos], amax[b:b + 1], rest[b, pos:]]) * (-1.0 if b % 2 else 1.0)
    x = blocks.reshape(255, 128)
    assert torch.equal(x.float().double(), x)
    return x.float()


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------
def test_reference_table_and_hand_cases():
    """the decoded table against torch's decoding of the same bytes (a widening, no rounding), and roundings worked by hand"""
    T = e4m3_table()
    assert torch.equal(T, torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).double())
    assert float(T[126]) == 448.0 and float(T[1]) == 2.0 ** -9 and float(T[8]) == 2.0 ** -6 and bool((T[1:] > T[:-1]).all())
    x = torch.zeros(32)
    x[0] = 448.0                                                      # scale byte 127: the elements are their own scaled values
    x[1:10] = torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, 432.0, 400.0, -0.0, -2.0 ** -10, 1.0, 1.0625, 1.1875])
    q, s = ref_quantize_mx8(x)
    # 2^-10 ties between codes 0 and 1 -> 0; 3 2^-10 between 1 and 2 -> 2; 432 between 125 and 126 -> 126; 400 between 124 (384) and
    # 125 (416) -> 124; 1.0625 between 0x38 (1.0) and 0x39 (1.125) -> 0x38; 1.1875 between 0x39 and 0x3A -> 0x3A
    assert int(s[0]) == 127 and q[:10].tolist() == [126, 0, 2, 126, 124, 0x80, 0x80, 0x38, 0x38, 0x3A]
    for amax, want in ((448.0, 127), (448.0 * (1 + 2.0 ** -23), 128), (449.0, 128), (224.0, 126), (2.0 ** -126, 0), (0.0, 0),
                       (448.0 * 2.0 ** -127, 0), (480.0 * 2.0 ** -127, 1), (3.4028234663852886e38, 247)):
        y = torch.zeros(32)
        y[5] = amax
        assert int(ref_quantize_mx8(y)[1][0]) == want, amax
    q, s = ref_quantize_mx8(torch.tensor([500.0] + [0.0] * 31))       # scale byte 128: 250 rounds to 256 (0x78), nothing saturates
    assert int(s[0]) == 128 and int(q[0]) == 0x78


def test_boundary_sets_are_what_they_claim():
    for dtype in (torch.float32, torch.bfloat16):
        x = boundary_rows(dtype)
        assert x.shape == (len(SBS), 1056)
        _, s = ref_quantize_mx8(x)
        assert torch.equal(s, torch.tensor(SBS, dtype=torch.uint8)[:, None].expand(-1, 33))
        kept = (x.double() != 0).sum(-1)
        print(f"{dtype}: non-zero elements per scale byte {dict(zip(SBS, kept.tolist()))}")
        assert bool((kept[3:-1] == 1008 + 33).all())                  # from 119 to 246: every point but +0 and -0, and the pins
        assert int(kept.min()) >= 600                                 # (sb 0, 1, 8: the subnormal range cuts neighbours; 247: |p| >= 256)
        b = torch.arange(33)
        blocks = x.double().abs().reshape(len(SBS), 33, 32)
        assert torch.equal(blocks[:, b, b % 32], blocks.amax(-1))     # the pin sits at b mod 32 (the point 448 may equal it elsewhere)
    x = scale_rows()
    _, s = ref_quantize_mx8(x)
    assert int(s.min()) == 0 and int(s.max()) == 247 and torch.unique(s).numel() == 248
    assert torch.equal(x.abs().reshape(1020, 32).argmax(-1), torch.arange(1020) % 32)


# ---- A1: the oracle against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_oracle_equals_reference_on_rounding_boundaries(dtype):
    from oracle import mx_oracle as MX
    x = boundary_rows(dtype)
    q, s = MX.quantize_mx8(x.float())
    qr, sr = ref_quantize_mx8(x)
    assert torch.equal(s, sr)
    bad = (q != qr).nonzero()
    assert bad.numel() == 0, [(SBS[i], float(x[i, j]), int(q[i, j]), int(qr[i, j])) for i, j in bad[:8].tolist()]


def test_oracle_equals_reference_on_scale_boundaries_and_random_data():
    from oracle import mx_oracle as MX
    from rald_amd import synth
    for x in (scale_rows(), synth.normal([64, 512], 300) * torch.logspace(-6, 6, 64)[:, None]):
        q, s = MX.quantize_mx8(x)
        qr, sr = ref_quantize_mx8(x)
        assert torch.equal(s, sr) and torch.equal(q, qr)


# ---- D: refusals in front of the first HIP call ------------------------------------------------------------------------------------------
def test_gemm_mx8_and_quantize_mx8_refuse_before_any_launch(L_cpu):
    """fake aligned pointers (the checks are numeric): every refusal names its constraint"""
    L, d = L_cpu, DUMMY

    def gemm(M=256, N=256, K=256, lda=None, ldb=None, ldc=None, A=d, B=d, Cp=d, epi=1, batch=1):
        lda, ldb, ldc = K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc
        return L.rald_op_gemm_mx8(A, d, lda, 0, 0, B, d, ldb, 0, 0, Cp, ldc, 0, None, M, N, K, batch, 1.0, epi, None, 1 << 30)

    _refused(L, gemm(K=96), "K must be a multiple of 128")
    _refused(L, gemm(K=192), "K must be a multiple of 128")
    _refused(L, gemm(N=258), "N must be a multiple of 4")
    _refused(L, gemm(lda=240), "lda/ldb", ">= K")
    _refused(L, gemm(ldb=128), "lda/ldb", ">= K")
    _refused(L, gemm(lda=264), "lda/ldb", "multiples of 16")
    _refused(L, gemm(ldb=260), "lda/ldb", "multiples of 16")
    _refused(L, gemm(A=d + 8), "16-byte aligned")
    _refused(L, gemm(B=d + 4), "16-byte aligned")
    _refused(L, gemm(Cp=d + 8), "16-byte aligned")
    _refused(L, gemm(ldc=252), "ldc must be >= N")
    _refused(L, gemm(ldc=258), "multiple of 4")
    _refused(L, gemm(M=1 << 25, K=2048), "scale index overflow")
    _refused(L, gemm(N=1 << 25, K=2048, ldc=1 << 25), "scale index overflow")
    _refused(L, gemm(epi=4), "bad epilogue")
    _refused(L, gemm(epi=-1), "bad epilogue")
    _refused(L, gemm(M=4096, N=4096, epi=7), "bad epilogue")          # the 256-tile route has the same switch
    _refused(L, gemm(batch=0), "empty problem")
    _refused(L, gemm(A=None), "null")

    def quant(K=64, ld_in=None, ld_q=None, x=d, q=d, rows=4, bf16=0):
        return L.rald_op_quantize_mx8(x, bf16, K if ld_in is None else ld_in, q, K if ld_q is None else ld_q, d, rows, K, None)

    _refused(L, quant(K=48), "multiple of 32")
    _refused(L, quant(K=0), "multiple of 32")
    _refused(L, quant(ld_in=68), "multiples of 8")
    _refused(L, quant(ld_q=76), "multiples of 8")
    _refused(L, quant(ld_in=32), ">= K")
    _refused(L, quant(x=d + 8), "misaligned")
    _refused(L, quant(x=d + 8, bf16=1), "misaligned")
    _refused(L, quant(q=d + 4), "misaligned")
    assert quant(rows=0) == 0                                         # nothing to do is no error and no launch


def test_gemm_mx8_tile_rule():
    """rald_op_gemm_mx8_tile reports gemm_mx8's own choice (one function serves both): full 256 x 256 tiles and at least 256 of them over
    the batch take the 256 x 256 kernel, everything else 128 x 128.  The GPU tests assert it for every shape they launch."""
    from rald_amd._lib import lib
    tile = lib().rald_op_gemm_mx8_tile
    assert [tile(256, 256, 255), tile(256, 256, 256), tile(4096, 4096, 1), tile(4096, 3840, 1), tile(4096 - 128, 4096 + 256, 1)] == [128, 256, 256, 128, 128]
    assert [tile(512, 4096, 1), tile(11264, 1536, 1), tile(32768, 512, 1), tile(768, 768, 29), tile(768, 768, 28), tile(384, 1024, 3)] == [128, 256, 256, 256, 128, 128]
