"""The persistent 256 x 256 LDS-DMA GEMM (gemm_nt_persist_kernel, csrc/gemm.hip) against the one-tile kernel it stands beside, through the
test entry rald_op_gemm_nt_256 (which launches either on any full-tile shape, the persistent one on a capped grid).

Shapes: M = 512, N = 768 (2 x 3 tiles) on 1 / 2 / 4 / 6 workgroups (6 / 3 / 2-or-1 / 1 tiles each) and M = 256, N = 2304 (9 n-tiles: more than
one 8-tile strip) on 1 / 2 / 4 / 6 / 9; K = 64, 128, 192, 512 = 1, 2, 3, 8 k-steps (no second stage, no DMA inside the loop, one DMA
iteration, the workload's depth).  Epilogues: bf16 without bias and alpha = 0.5 on the first 256 columns only, bf16 with bias, GEGLU with a
packed bias.  Operands are row slices of wider buffers (lda = K + 8, ldb = K + 16), the output a column slice (ldc = columns + 8) of a
NaN-prefilled buffer with a sentinel guard tail.

Checks per case: the persistent launch equals the one-tile launch bit for bit on random bf16 data (same arithmetic); small integers give the
bf16 epilogues the float64 product exactly (a tile written to the wrong place or built from the wrong stage is an exact mismatch); the columns
past the slice keep their NaNs and the guard tail its sentinel, bit for bit; run, rald_debug_poison_lds, run again is bit-identical (stage
parity, patch and bias-slot reuse)."""
import time

import pytest
import torch

gpu = pytest.mark.gpu
SENT = -12345.5
SHAPES = [(512, 768, g) for g in (1, 2, 4, 6)] + [(256, 2304, g) for g in (1, 2, 4, 6, 9)]
KS = (64, 128, 192, 512)
EPIS = ("bf16_alpha", "bf16_bias", "geglu")
_cache = {}


def _g(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _bits(t):
    return t.view(torch.int16)


@pytest.fixture(scope="module")
def H():
    from rald_amd import _handles
    return _handles


@pytest.fixture(autouse=True)
def _timed(request):
    t = time.perf_counter()
    yield
    print(f"time {request.node.name}: {time.perf_counter() - t:.2f} s")


def _operands(M, N, K, kind):
    """A [M, K], B [N, K] as bf16 row slices of wider device buffers, bias [N] f32; shared by every case of the shape (never written)"""
    key = ("ops", M, N, K, kind)
    if key not in _cache:
        g = _g(1000 * K + N + (7 if kind == "int" else 0))
        if kind == "int":
            A = torch.randint(-3, 4, (M, K), generator=g).float()
            B = torch.randint(-2, 3, (N, K), generator=g).float() + (torch.arange(N) % 3 == 0).float()[:, None]     # asymmetric
            bias = torch.randint(-4, 5, (N,), generator=g).float()
        else:
            A = torch.randn(M, K, generator=g)
            B = torch.randn(N, K, generator=g) / K ** 0.5
            bias = torch.randn(N, generator=g) * 0.1
        Ab = torch.full((M, K + 8), float("nan")).bfloat16()
        Bb = torch.full((N, K + 16), float("nan")).bfloat16()
        Ab[:, :K], Bb[:, :K] = A.bfloat16(), B.bfloat16()
        _cache[key] = (Ab.cuda(), Bb.cuda(), bias.cuda())
    return _cache[key]


def _launch(H, M, N, K, kind, epi, persistent, grid):
    """one call into a fresh guarded buffer; returns the whole buffer (on the CPU) and the [M, ldc] view's geometry"""
    Ab, Bb, bias = _operands(M, N, K, kind)
    nc = N // 2 if epi == "geglu" else N
    ldc = nc + 8
    buf = torch.full((M * ldc + 4096,), SENT, dtype=torch.bfloat16, device="cuda")
    buf[:M * ldc] = float("nan")
    out = buf[:M * ldc].view(M, ldc)[:, :nc]
    H.op_gemm_nt_256(Ab[:, :K], Bb[:, :K], out, bias=None if epi == "bf16_alpha" else bias, epilogue=3 if epi == "geglu" else 0,
                     alpha=0.5 if epi == "bf16_alpha" else 1.0, alpha_ncols=256 if epi == "bf16_alpha" else 1 << 30,
                     persistent=persistent, max_workgroups=grid)
    torch.cuda.synchronize()
    return buf.cpu(), nc, ldc


def _one_tile(H, M, N, K, kind, epi):
    """the one-tile kernel's result for the case: computed once, shared, never written"""
    key = ("ref", M, N, K, kind, epi)
    if key not in _cache:
        _cache[key] = _launch(H, M, N, K, kind, epi, 0, 1)[0]
    return _cache[key]


def _frame_ok(buf, M, nc, ldc):
    """columns past the slice still NaN-filled, guard tail still the sentinel, nothing inside the slice left NaN"""
    body, tail = buf[:M * ldc].view(M, ldc), buf[M * ldc:]
    return (bool(torch.isnan(body[:, nc:].float()).all())
            and bool(torch.equal(_bits(tail), _bits(torch.full_like(tail, SENT)))) and not bool(torch.isnan(body[:, :nc].float()).any()))


@gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N,grid", SHAPES)
def test_persistent_equals_one_tile_kernel_bitwise(H, M, N, grid, K):
    """random bf16 data: persistent = 1 on `grid` workgroups equals persistent = 0 bit for bit, for the three epilogues; frame intact"""
    bad = []
    for epi in EPIS:
        ref = _one_tile(H, M, N, K, "rand", epi)
        got, nc, ldc = _launch(H, M, N, K, "rand", epi, 1, grid)
        if not _frame_ok(ref, M, nc, ldc):
            bad.append((epi, "one-tile frame"))
        if not _frame_ok(got, M, nc, ldc):
            bad.append((epi, "persistent frame"))
        if not torch.equal(_bits(got), _bits(ref)):
            d = (_bits(got) != _bits(ref)).nonzero().flatten()
            bad.append((epi, f"{d.numel()} elements differ, first at flat index {int(d[0])} (row {int(d[0]) // ldc}, column {int(d[0]) % ldc})"))
    assert not bad, bad


@gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N,grid", SHAPES)
def test_persistent_exact_integers(H, M, N, grid, K):
    """small integers: every fp32 sum is exact, so both bf16 epilogues equal the float64 value alpha * A.B^T + bias rounded once to bf16"""
    bad = []
    for epi in ("bf16_alpha", "bf16_bias"):
        key = ("exact", M, N, K, epi)
        if key not in _cache:
            Ab, Bb, bias = _operands(M, N, K, "int")
            y = (Ab[:, :K].double() @ Bb[:, :K].double().t()).cpu()
            if epi == "bf16_alpha":
                y[:, :256] *= 0.5
            else:
                y += bias.cpu().double()
            _cache[key] = y.float().bfloat16()           # (the float64 values are exact in fp32: |y| < 2^24, halves included)
        want = _cache[key]
        got, nc, ldc = _launch(H, M, N, K, "int", epi, 1, grid)
        if not _frame_ok(got, M, nc, ldc):
            bad.append((epi, "frame"))
        res = got[:M * ldc].view(M, ldc)[:, :nc]
        if not torch.equal(_bits(res.contiguous()), _bits(want)):
            d = (res.float() != want.float()).nonzero()
            bad.append((epi, f"{d.shape[0]} elements differ, first at {d[0].tolist()}: {float(res[tuple(d[0])])} != {float(want[tuple(d[0])])}"))
    assert not bad, bad


@gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N,grid", SHAPES)
def test_persistent_results_do_not_depend_on_stale_lds(H, M, N, grid, K):
    """run, poison every CU's LDS, run again: bit-identical (stage-buffer parity, patch and bias-slot reuse), for the three epilogues"""
    from rald_amd._lib import check, lib
    bad = []
    for epi in EPIS:
        first = _launch(H, M, N, K, "rand", epi, 1, grid)[0]
        check(lib().rald_debug_poison_lds(torch.cuda.current_stream().cuda_stream))
        second = _launch(H, M, N, K, "rand", epi, 1, grid)[0]
        if not torch.equal(_bits(first), _bits(second)):
            bad.append(epi)
    assert not bad, bad
