"""The MXFP8 quantiser (quantize_mx8_kernel / mx8_block, csrc/mx8.h) and GEMM (gemm_mx8_kernel, csrc/gemm_fp8.hip, main loop Mx8Loop in
csrc/gemm_tile.h) per element at their edges.  The float64 quantiser reference and the boundary inputs are test_mx8_host.py's (which
also holds the oracle against that reference and the refusals); helpers are test_gpu_resid_ln.py's.

Quantiser, bit for bit against the reference, outputs in guarded buffers:
  rounding boundaries (every e4m3 magnitude, midpoint and midpoint neighbour, both signs, at scale bytes 0 .. 247, the amax in every
      lane and slot), fp32 and bf16 input                    test_quantize_rounding_boundaries_bit_exact
  scale boundaries (every fp32 exponent x mantissa 0, 1.75, 1.75 + ulp, all ones; fp32-subnormal blocks, which must not flush)
                                                             test_quantize_scale_boundaries_bit_exact
  rows 1, 3, 4, 5, 1023 x K 32 .. 2048 (partial passes of the 512-element row loop) x fp32 / bf16 x contiguous / a column slice of a
      NaN-filled tensor with ld_q > K; zero row, zero blocks  test_quantize_geometry
  +-Inf against the oracle; a NaN leaves the other blocks and the guards alone (both outside the contract, see oracle/mx_oracle.py)
                                                             test_quantize_non_finite_inputs

GEMM, exact: operands are built as bytes on the CPU (the HIP quantiser is not in the loop): elements are integers -4 .. 4 (-1 .. 1 under
the bf16 epilogue, whose results must be exact in bf16), block scale bytes = 127 + a base exponent per row of A / per column of the product
(from [-40, 40]) + a per-block delta in [-3, 3] (0 under the bf16 epilogue); row m of A carries m mod 5 and column n carries (n div 16) mod
5 and n mod 4 (all three mod 2 under the bf16 epilogue) on top of that, so a wrong tile, row, k-step or scale byte is a wrong number.  Every product of one dot product is a multiple
of 2^-6 below 2^10 in units of the row and column base (the envelope tests/test_fp8.py established for the scaled MFMA), every sum is
exact in fp32, and the result equals the float64 product of the oracle-dequantised operands under torch.equal.  With a bias or the
accumulating epilogue the bases of A stay in [0, 3] ([0, 0] for bf16) and bias / C carry the column's base, so those sums are exact too.
The LDS is poisoned before every launch, lda / ldb padding holds 0x7F (an e4m3 NaN), the scale arrays end in 0xFF (the e8m0 NaN), ldc padding
and the gaps between batch entries hold NaN, and a sentinel tail follows.  rald_op_gemm_mx8_tile (the dispatcher's own rule) is asserted
for every shape.
  the 128 x 128 route: M 1 .. 384, N 4 .. 1536 (N = 1024: the strip walk), 1, 2, 3, 16 k-steps, epilogues 0 / 1 / 2, bias, alpha,
      alpha_ncols inside N off a tile edge, batch 3 per entry and with shared B, scale bytes 1 .. 7 against 248 .. 254
                                                             test_gemm_128_route_exact
  the 256 x 256 route: 4096 x 4096 (strip walk), 11264 x 1536 with alpha_ncols = 512 (QKV at B = 22), 32768 x 512 (q2 at B = 64),
      768 x 768 x batch 29 with shared B, and 256 x 256 at batch 255 (128 route) / 256 (256 route); epilogues 0 and 1
                                                             test_gemm_256_route_exact
  rows 0 .. 511 of 4096 x 4096 x 512 alone (128 route) = the same rows of the full call (256 route), bit for bit, random data
                                                             test_gemm_routes_give_identical_sums
GEMM, random Gaussian data against the float64 product of the dequantised operands, every element:
      |C - ref| <= k 2^-16 (|A| . |B|^T)  (+ half a bf16 ulp of the result under epilogue 0)
  the scaled MFMA's 128-deep dot product is not an fp32 sum; k is measured (K_MX) and bounded at <= 2.5 x the worst value
                                                             test_gemm_random_per_element
  GEGLU on the 128 route from MXFP8 operands (FF1 of 'fp8_ff1' below B = 8), bound of test_gpu_resid_ln's GEGLU tests
                                                             test_geglu_128_route_mx8_operands"""
import math
import time

import pytest
import torch

from test_gpu_resid_ln import GELU_POLY_ABS, _Checks, _geglu_pack, _geglu_ref, _guard_ok, _guarded, _ratio16
from test_mx8_host import SBS, _pow2, boundary_rows, ref_quantize_mx8, scale_rows

gpu = pytest.mark.gpu

# measured on an MI355X (worst over the cases of the named test); bound <= 2.5 x that, rounded up
K_MX = {128: {1: 1.75, 0: 0.8},               # test_gemm_random_per_element, 1024 x 1536 x 512: epilogue 1 measured 0.700, epilogue 0 measured 0.320
        256: {1: 2.0, 0: 1.0}}                # 4096 x 4096 x 512: epilogue 1 measured 0.818, epilogue 0 measured 0.425
K_GEGLU_128_MX = {128: 400, 384: 110}         # test_geglu_128_route_mx8_operands, in _ratio16's units of 2^-24: measured 163 (K = 128), 44.8 (K = 384)


@pytest.fixture(scope="module")
def H():
    from rald_amd import _handles
    return _handles


@pytest.fixture(autouse=True)
def _timed(request):
    t = time.perf_counter()
    yield
    print(f"time {request.node.name}: {time.perf_counter() - t:.2f} s")


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _g(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _poison():
    from rald_amd._lib import check, lib
    check(lib().rald_debug_poison_lds(_stream()))


def _tile(M, N, batch):
    from rald_amd._lib import lib
    return lib().rald_op_gemm_mx8_tile(M, N, batch)


# ---- quantiser -------------------------------------------------------------------------------------------------------------------------
def _run_quantize(x, ld_q=None):
    """rald_op_quantize_mx8 on the 2-D device view x into guarded buffers (rows of ld_q bytes): (bytes [rows, K], scales) on the CPU"""
    from rald_amd._lib import check, lib
    rows, K = x.shape
    ld_q = K if ld_q is None else ld_q
    nq, ns = rows * ld_q, rows * (K // 32)
    q, s = _guarded(nq, 4096, torch.uint8, 0x7F), _guarded(ns, 256, torch.uint8, 0xFF)
    check(lib().rald_op_quantize_mx8(x.data_ptr(), int(x.dtype == torch.bfloat16), x.stride(0), q.data_ptr(), ld_q, s.data_ptr(), rows, K, _stream()))
    torch.cuda.synchronize()
    assert _guard_ok(q, nq) and _guard_ok(s, ns), "guard bytes overwritten"
    body = q[:nq].view(rows, ld_q).cpu()
    assert bool((body[:, K:] == 0x7F).all()), "bytes between the rows overwritten"
    return body[:, :K].contiguous(), s[:ns].view(rows, K // 32).cpu()


def _quant_diff(x, q, s, qr, sr):
    """'' if (q, s) equals the reference, else the first few mismatches: (row, column, input, got, want)"""
    out = []
    bad = (s != sr).nonzero()
    if bad.numel():
        out.append(f"{bad.shape[0]} scale bytes differ: " + str([(i, j, float(x[i, 32 * j:32 * j + 32].float().abs().max()), int(s[i, j]), int(sr[i, j]))
                                                               for i, j in bad[:6].tolist()]))
    bad = (q != qr).nonzero()
    if bad.numel():
        out.append(f"{bad.shape[0]} element bytes differ: " + str([(i, j, float(x[i, j]), int(s[i, j // 32]), hex(int(q[i, j])), hex(int(qr[i, j])))
                                                                 for i, j in bad[:6].tolist()]))
    return "; ".join(out)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_quantize_rounding_boundaries_bit_exact(dtype):
    """one row of 33 blocks per scale byte in SBS (three passes of the row loop, the last a partial one)"""
    x = boundary_rows(dtype)
    qr, sr = ref_quantize_mx8(x)
    assert sorted(set(sr.flatten().tolist())) == sorted(SBS)
    q, s = _run_quantize(x.cuda())
    assert not _quant_diff(x, q, s, qr, sr)


@gpu
def test_quantize_scale_boundaries_bit_exact():
    """1020 blocks whose amax is each exponent's 1.0, 1.75, 1.75 + ulp and largest mantissa, and four fp32-subnormal amax values: the scale
    byte is the smallest that fits (0 .. 247), and subnormal inputs are quantised, not flushed: at scale byte 0 the unit is 2^-127, so
    the largest subnormal, 2^-126 (1 - 2^-23), is just under 2.0 in the block's units and its block is not zero"""
    x = scale_rows()
    qr, sr = ref_quantize_mx8(x)
    q, s = _run_quantize(x.cuda())
    assert not _quant_diff(x, q, s, qr, sr)
    assert int(q.view(-1, 32)[-1].max()) > 0                          # the last block is subnormal and not all zero


ROWS = (1, 3, 4, 5, 1023)


@gpu
@pytest.mark.parametrize("K", [32, 64, 96, 480, 512, 544, 1024, 2048])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_quantize_geometry(dtype, K):
    """Gaussian rows over ten decades with an all-zero row and all-zero blocks; the first `rows` rows of one array, contiguous and as a
    column slice of a wider NaN-filled tensor (ld_in = K + 24, the slice 8 elements in) with ld_q = K + 8"""
    x = torch.randn(1023, K, generator=_g(4000 + K)) * torch.logspace(-5, 5, 1023)[torch.randperm(1023, generator=_g(1))][:, None]
    x[2] = 0.0
    x[0, :32] = 0.0
    x[4, K - 32:] = 0.0
    x = x.to(dtype)
    qr, sr = ref_quantize_mx8(x)
    xc = x.cuda()
    wide = torch.full((1023, K + 24), float("nan"), dtype=dtype, device="cuda")
    wide[:, 8:8 + K] = xc
    bad = []
    for rows in ROWS:
        for name, xin, ld_q in (("contiguous", xc[:rows], K), ("slice", wide[:rows, 8:8 + K], K + 8)):
            q, s = _run_quantize(xin, ld_q)
            d = _quant_diff(x, q, s, qr[:rows], sr[:rows])
            if d:
                bad.append((rows, name, d))
    assert not bad, bad


@gpu
def test_quantize_non_finite_inputs():
    """Outside the format's contract (oracle/mx_oracle.py says what each side does).  +-Inf: kernel = oracle (scale byte 247, +-448, the rest
    of the block at 2^-120).  NaN: the kernel drops it from amax and writes -448 at the block's scale where the oracle writes 0x7F at scale
    byte 247; pinned here is only that the row's other blocks and the guard bytes are untouched."""
    from oracle import mx_oracle as MX
    x = torch.randn(4, 128, generator=_g(77))
    x[0, 37], x[1, 100], x[2, 70] = float("inf"), float("-inf"), float("nan")
    q, s = _run_quantize(x.cuda())
    qo, so = MX.quantize_mx8(x)
    fin = [0, 1, 3]
    assert torch.equal(q[fin], qo[fin]) and torch.equal(s[fin], so[fin])
    assert int(s[0, 1]) == 247 and int(q[0, 37]) == 0x7E and int(s[1, 3]) == 247 and int(q[1, 100]) == 0xFE
    clean = x[2].clone()
    clean[70] = 0.0
    qr, sr = ref_quantize_mx8(clean[None])
    for blk in (0, 1, 3):
        assert torch.equal(q[2, 32 * blk:32 * blk + 32], qr[0, 32 * blk:32 * blk + 32]) and int(s[2, blk]) == int(sr[0, blk])


# ---- GEMM: operands as bytes ------------------------------------------------------------------------------------------------------------
E4M3_OF_INT = torch.tensor([0xC8, 0xC4, 0xC0, 0xB8, 0x00, 0x38, 0x40, 0x44, 0x48], dtype=torch.uint8)      # -4 .. 4


def _byte_operand(batch, rows, K, seed, lim, delta, base, side, one_base=False):
    """(e4m3 bytes [batch, rows, K], e8m0 bytes [batch, rows, K/32], float64 values, base exponents [batch, rows]): integers -lim .. lim,
    scale byte 127 + base exponent (uniform in base[0] .. base[1] per row and entry, or per row for all entries: a bias is shared by the
    entries) + a block delta in -delta .. delta; side 'A' / 'B' sets the identifying columns"""
    from oracle import mx_oracle as MX
    g = _g(seed)
    v = torch.randint(-lim, lim + 1, (batch, rows, K), generator=g)
    r = torch.arange(rows)
    if side == "A":
        v[..., 0], v[..., 1], v[..., 33] = r % 5 if lim >= 4 else r % 2, 1, 1
    else:
        v[..., 0], v[..., 1], v[..., 33] = 1, (r // 16) % 5 if lim >= 4 else (r // 16) % 2, (r % 4) if lim >= 4 else (r % 2)
    be = torch.randint(base[0], base[1] + 1, (1 if one_base else batch, rows, 1), generator=g).expand(batch, rows, 1)
    e = be + torch.randint(-delta, delta + 1, (batch, rows, K // 32), generator=g)
    q, s = E4M3_OF_INT[v + 4], (127 + e).to(torch.uint8)
    assert 1 <= int(e.min()) + 127 and int(e.max()) + 127 <= 254
    val = (v.double().reshape(batch, rows, K // 32, 32) * _pow2(e)[..., None]).reshape(batch, rows, K)
    assert torch.equal(MX.dequantize_mx8(q, s, torch.float64), val)  # the oracle's dequantisation is what the product is taken of
    return q, s, val, be[..., 0]


def _upload_bytes(q, pad):
    """[batch, rows, K] -> the [.., :K] view of a device array with rows of K + pad bytes, the padding 0x7F"""
    b, rows, K = q.shape
    buf = torch.full((b, rows, K + pad), 0x7F, dtype=torch.uint8)
    buf[..., :K] = q
    return buf.cuda()[..., :K]


def _upload_scales(s):
    """a contiguous device copy followed by 256 bytes of 0xFF"""
    flat = torch.full((s.numel() + 256,), 0xFF, dtype=torch.uint8)
    flat[:s.numel()] = s.flatten()
    return flat.cuda()[:s.numel()].view(s.shape)


def _frame(batch, M, N, dtype):
    """a NaN-filled output frame with ldc > N, a NaN gap between batch entries and a sentinel tail: (buffer, [batch, M, N] view, ldc, sC)"""
    ldc = N + 4 if dtype == torch.float32 else (N + 7) // 8 * 8 + 8
    sC = M * ldc + 64
    buf = _guarded(batch * sC, 4096, dtype)
    return buf, torch.as_strided(buf, (batch, M, N), (sC, ldc, 1)), ldc, sC


def _frame_ok(buf, batch, M, N, ldc, sC):
    body = buf[:batch * sC].view(batch, sC)
    inner = body[:, :M * ldc].reshape(batch, M, ldc)
    return (_guard_ok(buf, batch * sC) and bool(torch.isnan(body[:, M * ldc:]).all()) and bool(torch.isnan(inner[:, :, N:]).all())
            and not bool(torch.isnan(inner[:, :, :N]).any()))


def _exact_problem(M, N, K, batch, epi, bias, alpha, alpha_ncols, shared_b, a_base, b_base, seed, dev):
    """the operands of one exact case as bytes, its bias and initial C (float64, CPU) and the float64 result on `dev`"""
    lim, delta = (1, 0) if epi == 0 else (4, 3)
    if bias or epi == 2:
        a_base = (0, 0) if epi == 0 else (0, 3)
    qa, sa, va, _ = _byte_operand(batch, M, K, 10 * seed + 1, lim, delta, a_base, "A")
    qb, sb, vb, eb = _byte_operand(1 if shared_b else batch, N, K, 10 * seed + 2, lim, delta, b_base, "B", one_base=bias)
    g = _g(10 * seed + 3)
    cb = _pow2(eb)                                                    # [batch or 1, N]: bias and the accumulated C carry the column's base
    bias_v = torch.randint(-4, 5, (N,), generator=g).double() * cb[0] if bias else None
    c0 = torch.randint(-4, 5, (batch, M, N), generator=g).double() * cb[:, None, :] if epi == 2 else None
    al = torch.where(torch.arange(N) < alpha_ncols, alpha, 1.0).double()
    ref = al.to(dev) * (va.to(dev) @ vb.to(dev).transpose(-1, -2))
    if bias:
        ref = ref + bias_v.to(dev)
    if epi == 2:
        ref = ref + c0.to(dev)
    return qa, sa, qb, sb, bias_v, c0, ref


def _exact(H, M, N, K, tile, batch=1, epi=1, bias=False, alpha=1.0, alpha_ncols=1 << 30, shared_b=False, a_base=(-40, 40), b_base=(-40, 40), seed=0):
    """one exact case (module docstring); '' or what went wrong"""
    assert _tile(M, N, batch) == tile, (M, N, batch, _tile(M, N, batch))
    dtype = torch.bfloat16 if epi == 0 else torch.float32
    qa, sa, qb, sb, bias_v, c0, ref = _exact_problem(M, N, K, batch, epi, bias, alpha, alpha_ncols, shared_b, a_base, b_base, seed, "cuda")
    if not torch.equal(ref.to(dtype).double(), ref):
        return "premise: the float64 result is not exact in the output type"
    A8, SA, B8, SB = _upload_bytes(qa, 16), _upload_scales(sa), _upload_bytes(qb, 32), _upload_scales(sb)
    if batch == 1:
        A8, SA = A8[0], SA[0]
    if shared_b or batch == 1:
        B8, SB = B8[0], SB[0]
    buf, out, ldc, sC = _frame(batch, M, N, dtype)
    if epi == 2:
        out.copy_(c0.float())
    _poison()
    H.op_gemm_mx8(A8, SA, B8, SB, bias=bias_v.float().cuda() if bias else None, epilogue=epi, C_inout=out if batch > 1 else out[0], alpha=alpha,
                  alpha_ncols=alpha_ncols)
    torch.cuda.synchronize()
    if not _frame_ok(buf, batch, M, N, ldc, sC):
        return "frame: padding, gap or guard tail overwritten, or NaN in the result"
    got = out.double()
    if not torch.equal(got, ref):
        d = (got != ref).nonzero()
        i = d[0].tolist()
        return f"{d.shape[0]} of {ref.numel()} elements differ, first at (entry, row, column) {i}: got {float(got[tuple(i)])}, want {float(ref[tuple(i)])}"
    return ""


CASES_128 = [
    # M, N, K, then keywords
    (1, 4, 128, dict(epi=1, bias=True)),
    (15, 12, 256, dict(epi=1, alpha=0.25)),
    (17, 124, 384, dict(epi=0, alpha=0.5, alpha_ncols=60)),
    (127, 132, 128, dict(epi=2, bias=True)),
    (129, 260, 2048, dict(epi=1, bias=True, alpha=0.5, alpha_ncols=132)),
    (200, 1024, 256, dict(epi=0, bias=True)),                                     # 8 tiles wide: the strip walk
    (384, 1024, 128, dict(epi=1)),                                                # strip walk, one k-step
    (384, 1536, 384, dict(epi=1, alpha=0.5, alpha_ncols=516)),
    (200, 260, 256, dict(epi=1, bias=True, batch=3)),                             # A, B and their scales per entry
    (129, 132, 384, dict(epi=0, batch=3, shared_b=True)),
    (384, 1024, 2048, dict(epi=2, batch=3, shared_b=True)),
    (129, 132, 256, dict(epi=1, a_base=(-123, -123), b_base=(124, 124))),         # scale bytes 1 .. 7 of A against 248 .. 254 of B
    (200, 260, 128, dict(epi=1, a_base=(124, 124), b_base=(-123, -123), alpha=0.5)),
]


@gpu
@pytest.mark.parametrize("M,N,K,kw", CASES_128, ids=[f"{c[0]}x{c[1]}x{c[2]}" + "".join(f"-{k}{v}" for k, v in c[3].items() if k in ("epi", "batch")) for c in CASES_128])
def test_gemm_128_route_exact(H, M, N, K, kw):
    assert not _exact(H, M, N, K, 128, seed=M + N + K, **kw)


CASES_256 = [
    (4096, 4096, 128, dict()),                                                    # 16 x 16 tiles: the strip walk
    (11264, 1536, 512, dict(alpha=0.5, alpha_ncols=512)),                         # QKV at B = 22: 264 tiles, row-major walk
    (32768, 512, 128, dict()),                                                    # q2 at B = 64: two tiles wide
    (768, 768, 256, dict(batch=29, shared_b=True)),                               # 261 tiles, not a multiple of 8
    (256, 256, 128, dict(batch=256)),                                             # the route rule's 256 side ...
    (256, 256, 128, dict(batch=255, tile=128)),                                   # ... and its 128 side
]


@gpu
@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("M,N,K,kw", CASES_256, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3].get('batch', 1)}" for c in CASES_256])
def test_gemm_256_route_exact(H, M, N, K, kw, epi):
    kw = dict(kw)
    tile = kw.pop("tile", 256)
    assert not _exact(H, M, N, K, tile, epi=epi, seed=M + N + K + epi, **kw)


# ---- GEMM: random data -----------------------------------------------------------------------------------------------------------------
_cache = {}


def _gauss(M, N, K):
    """Gaussian operands quantised by the oracle, on the device as bytes and as float64 values: A, B, and the float64 product and |A|.|B|^T"""
    from oracle import mx_oracle as MX
    key = (M, N, K)
    if key not in _cache:
        g = _g(31 * M + N + K)
        (qa, sa), (qb, sb) = MX.quantize_mx8(torch.randn(M, K, generator=g) * 2), MX.quantize_mx8(torch.randn(N, K, generator=g) / K ** 0.5)
        va, vb = MX.dequantize_mx8(qa, sa).cuda().double(), MX.dequantize_mx8(qb, sb).cuda().double()
        _cache.clear()                                                # one set at a time on the device
        _cache[key] = (qa.cuda(), _upload_scales(sa), qb.cuda(), _upload_scales(sb), va @ vb.t(), va.abs() @ vb.abs().t())
    return _cache[key]


@gpu
@pytest.mark.parametrize("epi", [1, 0])
@pytest.mark.parametrize("M,N,K,tile", [(1024, 1536, 512, 128), (4096, 4096, 512, 256)])
def test_gemm_random_per_element(H, M, N, K, tile, epi):
    chk = _Checks()
    assert _tile(M, N, 1) == tile
    qa, sa, qb, sb, ref, terms = _gauss(M, N, K)
    _poison()
    got = H.op_gemm_mx8(qa, sa, qb, sb, epilogue=epi)
    torch.cuda.synchronize()
    g64 = got.double()
    err = (g64 - ref).abs()
    if epi == 0:                                                      # the fp32 value rounds to `got`: within half an ulp of got's binade
        err = (err - torch.exp2(torch.floor(torch.log2(g64.abs().clamp_min(2.0 ** -126))) - 8)).clamp_min(0)
    r = err / (2.0 ** -16 * terms.clamp_min(2.0 ** -126))
    r = torch.where(torch.isnan(g64), torch.full_like(r, math.inf), r)
    chk.le(f"gemm_mx8 {M}x{N}x{K} tile {tile} epilogue {epi}", float(r.max()), K_MX[tile][epi])
    chk.true("something was computed", float(g64.abs().max()) > 0)
    chk.done()


@gpu
def test_gemm_routes_give_identical_sums(H):
    """k-steps run in ascending order from 0 in every tile, so a sample's sums do not depend on its tile or batch size.  Rows
    0 .. 511 alone are 4 x 32 tiles of 128 x 128; inside the full product they are the first two tile rows of the 256 x 256 kernel."""
    M, N, K = 4096, 4096, 512
    qa, sa, qb, sb, _, _ = _gauss(M, N, K)
    assert _tile(M, N, 1) == 256 and _tile(512, N, 1) == 128
    _poison()
    full = H.op_gemm_mx8(qa, sa, qb, sb, epilogue=1)
    _poison()
    part = H.op_gemm_mx8(qa[:512], sa[:512], qb, sb, epilogue=1)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(part).any()) and float(part.abs().max()) > 0
    d = (full[:512].view(torch.int32) != part.view(torch.int32)).nonzero()
    assert d.numel() == 0, f"{d.shape[0]} elements differ, first at {d[0].tolist()}"


@gpu
@pytest.mark.parametrize("K", [128, 384])
def test_geglu_128_route_mx8_operands(H, K):
    """EPI_GEGLU of gemm_mx8 on 128 x 128 tiles: M = 384, 256 packed rows -> 128 columns, one and three k-steps, LDS poisoned.  Per element
    one bf16 ulp + |x + b_x| 4.5e-5 + k 2^-24 terms, as test_geglu_256x256_mx8_output_equals_quantised_bf16_output."""
    from oracle import mx_oracle as MX
    chk = _Checks()
    M, N = 384, 256
    assert _tile(M, N, 1) == 128
    g = _g(9300 + K)
    (A8, SA), (W8, SW) = MX.quantize_mx8(torch.randn(M, K, generator=g)), MX.quantize_mx8(torch.randn(N, K, generator=g) / K ** 0.5)
    A, W = MX.dequantize_mx8(A8, SA), MX.dequantize_mx8(W8, SW)
    bias = torch.randn(N, generator=g) * 0.1
    Wp, bp = _geglu_pack(W, bias)
    W8p, SWp = MX.quantize_mx8(Wp)                                    # per row: the packed rows' bytes
    assert torch.equal(MX.dequantize_mx8(W8p, SWp), Wp)
    n = M * (N // 2)
    out = _guarded(n, 1024, torch.bfloat16)
    _poison()
    H.op_gemm_geglu_mx8out(bp.cuda(), M, N, K, A8=_upload_bytes(A8[None], 16)[0], SA=_upload_scales(SA), W8=_upload_bytes(W8p[None], 32)[0],
                           SW=_upload_scales(SWp), out=out[:n].view(M, N // 2))
    torch.cuda.synchronize()
    assert _guard_ok(out, n)
    ref, terms, ax = _geglu_ref(A, W, bias)
    chk.le(f"geglu 128 route, MXFP8 operands, K = {K}", _ratio16(out[:n].view(M, N // 2).cpu(), ref, terms, ax * GELU_POLY_ABS), K_GEGLU_128_MX[K])
    chk.done()
