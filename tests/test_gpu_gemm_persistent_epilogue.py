"""The persistent 256 x 256 GEMM's one-barrier epilogue and its batched softmax route (gemm_nt_persist_kernel, csrc/gemm.hip), bit for bit
against the one-tile kernel through the test entries rald_op_gemm_nt_256 and rald_op_gemm_nt_256_batched.  No tolerance anywhere: the
one-tile kernels are pinned against float64 in test_gpu_resid_ln.py and test_gpu_kernels.py.

Hand-off (a store wave's private patch, the DMA waves' patches double-buffered by step parity, one barrier per step): 1 x 9 tiles on 1 / 2 / 9
workgroups, 1 x 16 tiles on 1 workgroup (16 epilogues in a row on one CU), 2 x 3 tiles on 1 / 4 / 6; K = 64, 128, 512; bf16 with alpha on
the first 256 columns, bf16 with bias, GEGLU.  Operands are small integers (every sum exact) with row m of A carrying m mod 61 and column n
of the product carrying its 64-column group: every output row and column group is distinct, so a patch read a step early or late or from the
wrong partner is a wrong row, not noise.  The LDS is poisoned before every persistent launch; outputs are column slices of NaN-filled
buffers with a sentinel tail.  The hand-off is a matter of timing between waves, so the 1 x 16 case is also launched eight times back to back.

Batched softmax: batch 1 / 3 / 8 of 512 x 512 (2 x 2 tiles; 8 entries take the one-tile kernel's XCD dealing) and batch 2 of 256 x 768, K = 64,
128, 512, grids capped at 1 / 3 / 5 and uncapped, strideC with a NaN gap between the entries, B per entry and shared (strideB = 0); all scores
equal gives exactly 1/64.  The refusals are host checks in front of the first HIP call."""
import time

import pytest
import torch

gpu = pytest.mark.gpu
SENT = -12345.5
HANDOFF = [(256, 2304, g) for g in (1, 2, 9)] + [(256, 4096, 1)] + [(512, 768, g) for g in (1, 4, 6)]
KS = (64, 128, 512)
EPIS = ("bf16_alpha", "bf16_bias", "geglu")
UNCAPPED = 1 << 30
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


def _poison():
    from rald_amd._lib import check, lib
    check(lib().rald_debug_poison_lds(torch.cuda.current_stream().cuda_stream))


# ---- part A: hand-off across steps and tiles ---------------------------------------------------------------------------------------------
def _operands(M, N, K):
    """integers: A[m] = (m mod 61, 1, -1/0/1 ...), B[n] = (1, group of n mod 5, -1/0/1 ...): product = m mod 61 + (n // 64) mod 5 + a small sum"""
    key = ("ops", M, N, K)
    if key not in _cache:
        g = _g(1000 * K + N)
        A = torch.randint(-1, 2, (M, K), generator=g).float()
        B = torch.randint(-1, 2, (N, K), generator=g).float()
        A[:, 0], A[:, 1] = (torch.arange(M) % 61).float(), 1.0
        B[:, 0], B[:, 1] = 1.0, ((torch.arange(N) // 64) % 5).float()
        bias = torch.randint(-4, 5, (N,), generator=g).float()
        Ab = torch.full((M, K + 8), float("nan")).bfloat16()
        Bb = torch.full((N, K + 16), float("nan")).bfloat16()
        Ab[:, :K], Bb[:, :K] = A.bfloat16(), B.bfloat16()
        _cache[key] = (Ab.cuda(), Bb.cuda(), bias.cuda())
    return _cache[key]


def _launch(H, M, N, K, epi, persistent, grid, sync=True):
    """one call into a fresh guarded buffer; the whole buffer (on the device if not sync) and the [M, ldc] view's geometry"""
    Ab, Bb, bias = _operands(M, N, K)
    nc = N // 2 if epi == "geglu" else N
    ldc = nc + 8
    buf = torch.full((M * ldc + 4096,), SENT, dtype=torch.bfloat16, device="cuda")
    buf[:M * ldc] = float("nan")
    out = buf[:M * ldc].view(M, ldc)[:, :nc]
    H.op_gemm_nt_256(Ab[:, :K], Bb[:, :K], out, bias=None if epi == "bf16_alpha" else bias, epilogue=3 if epi == "geglu" else 0,
                     alpha=0.5 if epi == "bf16_alpha" else 1.0, alpha_ncols=256 if epi == "bf16_alpha" else 1 << 30,
                     persistent=persistent, max_workgroups=grid)
    if not sync:
        return buf, nc, ldc
    torch.cuda.synchronize()
    return buf.cpu(), nc, ldc


def _one_tile(H, M, N, K, epi):
    key = ("ref", M, N, K, epi)
    if key not in _cache:
        _cache[key] = _launch(H, M, N, K, epi, 0, 1)[0]
    return _cache[key]


def _frame_ok(buf, M, nc, ldc):
    body, tail = buf[:M * ldc].view(M, ldc), buf[M * ldc:]
    return (bool(torch.isnan(body[:, nc:].float()).all())
            and bool(torch.equal(_bits(tail), _bits(torch.full_like(tail, SENT)))) and not bool(torch.isnan(body[:, :nc].float()).any()))


def _diff(got, ref, ldc):
    d = (_bits(got) != _bits(ref)).nonzero().flatten()
    return f"{d.numel()} elements differ, first at flat index {int(d[0])} (row {int(d[0]) // ldc}, column {int(d[0]) % ldc})"


@gpu
def test_operands_make_rows_and_column_groups_distinct(H):
    """the premise of the hand-off cases: in the one-tile result no two rows of a tile column and no two 64-column groups of a row are equal"""
    M, N, K = 256, 2304, 128
    buf = _one_tile(H, M, N, K, "bf16_bias")
    y = buf[:M * (N + 8)].view(M, N + 8)[:, :N].float()
    assert torch.unique(y[:, :256], dim=0).shape[0] == M
    groups = y.view(M, N // 64, 64)
    assert all(torch.unique(groups[m], dim=0).shape[0] == N // 64 for m in range(0, M, 37))


@gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N,grid", HANDOFF)
def test_handoff_equals_one_tile_kernel_bitwise(H, M, N, grid, K):
    """poisoned LDS, then the persistent kernel on `grid` workgroups: bit-identical to the one-tile kernel, frame and guard tail intact"""
    bad = []
    for epi in EPIS:
        ref = _one_tile(H, M, N, K, epi)
        _poison()
        got, nc, ldc = _launch(H, M, N, K, epi, 1, grid)
        if not _frame_ok(ref, M, nc, ldc):
            bad.append((epi, "one-tile frame"))
        if not _frame_ok(got, M, nc, ldc):
            bad.append((epi, "persistent frame"))
        if not torch.equal(_bits(got), _bits(ref)):
            bad.append((epi, _diff(got, ref, ldc)))
    assert not bad, bad


@gpu
@pytest.mark.parametrize("K", KS)
def test_handoff_eight_launches_back_to_back(H, K):
    """1 x 16 tiles on one workgroup, eight launches queued without a wait between them: each equals the one-tile result"""
    M, N = 256, 4096
    bad = []
    for epi in EPIS:
        ref = _one_tile(H, M, N, K, epi)
        _poison()
        runs = [_launch(H, M, N, K, epi, 1, 1, sync=False) for _ in range(8)]
        torch.cuda.synchronize()
        for n, (buf, nc, ldc) in enumerate(runs):
            got = buf.cpu()
            if not torch.equal(_bits(got), _bits(ref)):
                bad.append((epi, n, _diff(got, ref, ldc)))
    assert not bad, bad


# ---- part B: the batched softmax route ---------------------------------------------------------------------------------------------------
SOFTMAX_SHAPES = [(1, 512, 512), (3, 512, 512), (8, 512, 512), (2, 256, 768)]
CAPS = (1, 3, 5, UNCAPPED)
GAP = 64                                                   # elements between two entries' outputs


def _softmax_operands(batch, M, N, K):
    key = ("sm", batch, M, N, K)
    if key not in _cache:
        g = _g(77 * K + 5 * N + batch)
        A = torch.randn(batch, M, K, generator=g).bfloat16().cuda()
        B = torch.randn(batch, N, K, generator=g).bfloat16().cuda()
        _cache[key] = (A, B)
    return _cache[key]


def _softmax_launch(H, batch, M, N, K, shared_b, persistent, cap, zero_a=False):
    A, B = _softmax_operands(batch, M, N, K)
    if zero_a:
        A = torch.zeros_like(A)
    ldc = N + 8
    sC = M * ldc + GAP
    buf = torch.full((batch * sC + 4096,), SENT, dtype=torch.bfloat16, device="cuda")
    buf[:batch * sC] = float("nan")
    out = torch.as_strided(buf, (batch, M, N), (sC, ldc, 1))
    H.op_gemm_nt_256_batched(A, B[0] if shared_b else B, out, epilogue=4, alpha=1.4426950408889634 / K ** 0.5, persistent=persistent,
                             max_workgroups=cap)
    torch.cuda.synchronize()
    return buf.cpu(), sC, ldc


def _softmax_frame_ok(buf, batch, M, N, sC, ldc):
    body, tail = buf[:batch * sC].view(batch, sC), buf[batch * sC:]
    inner = body[:, :M * ldc].reshape(batch, M, ldc)
    return (bool(torch.isnan(body[:, M * ldc:].float()).all()) and bool(torch.isnan(inner[:, :, N:].float()).all())
            and not bool(torch.isnan(inner[:, :, :N].float()).any()) and bool(torch.equal(_bits(tail), _bits(torch.full_like(tail, SENT)))))


@gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("batch,M,N", SOFTMAX_SHAPES)
def test_batched_softmax_equals_one_tile_kernel_bitwise(H, batch, M, N, K):
    """B per entry and shared, every grid cap: the persistent batched launch equals the one-tile batched launch bit for bit, the NaN gaps
    between the entries, the columns past the slice and the guard tail intact"""
    bad = []
    for shared_b in (False, True):
        ref, sC, ldc = _softmax_launch(H, batch, M, N, K, shared_b, 0, 1)
        if not _softmax_frame_ok(ref, batch, M, N, sC, ldc):
            bad.append((shared_b, "one-tile frame"))
        for cap in CAPS:
            _poison()
            got = _softmax_launch(H, batch, M, N, K, shared_b, 1, cap)[0]
            if not _softmax_frame_ok(got, batch, M, N, sC, ldc):
                bad.append((shared_b, cap, "persistent frame"))
            if not torch.equal(_bits(got), _bits(ref)):
                d = (_bits(got) != _bits(ref)).nonzero().flatten()
                i = int(d[0])
                bad.append((shared_b, cap, f"{d.numel()} elements differ, first in entry {i // sC}, row {i % sC // ldc}, column {i % sC % ldc}"))
    assert not bad, bad


@gpu
def test_batched_softmax_rows_sum_to_one_per_group(H):
    """what the bit comparison rests on: the one-tile result is a softmax.  Every 64-column group of every row sums to 1 within the outputs'
    bf16 rounding: each value is off by at most 2^-9 of itself, so the sum by at most 2^-9 of the sum (the fp32 steps add about 1e-6)"""
    batch, M, N, K = 3, 512, 512, 128
    buf, sC, ldc = _softmax_launch(H, batch, M, N, K, False, 0, 1)
    y = torch.as_strided(buf, (batch, M, N), (sC, ldc, 1)).float()
    s = y.reshape(batch, M, N // 64, 64).sum(-1)
    assert float((s - 1).abs().max()) <= 2.0 ** -9 + 1e-5


@gpu
@pytest.mark.parametrize("cap", CAPS)
def test_batched_softmax_equal_scores_give_one_64th(H, cap):
    """A = 0: every score is 0, exp2(0) = 1, the sum 64 and every output exactly 1/64"""
    batch, M, N, K = 8, 512, 512, 64
    buf, sC, ldc = _softmax_launch(H, batch, M, N, K, False, 1, cap, zero_a=True)
    assert _softmax_frame_ok(buf, batch, M, N, sC, ldc)
    y = torch.as_strided(buf, (batch, M, N), (sC, ldc, 1))
    assert torch.equal(_bits(y.contiguous()), _bits(torch.full((batch, M, N), 1.0 / 64).bfloat16()))


def test_batched_entry_refuses_on_the_host():
    """partial tiles, a bias under the softmax epilogue, an inner batch, a bad cap, a batch of bf16 tiles on the persistent engine and outputs
    that overlap: each refused by the host checks, which stand in front of the first HIP call (so this needs no device; the buffers live on
    one if there is one, and are large enough for every case)"""
    from rald_amd._lib import check, lib
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    A = torch.zeros(2, 512, 64, dtype=torch.bfloat16, device=dev)
    B = torch.zeros(2, 512, 64, dtype=torch.bfloat16, device=dev)
    Cc = torch.zeros(2, 512, 512, dtype=torch.bfloat16, device=dev)
    bias = torch.zeros(512, dtype=torch.float32, device=dev)

    def call(M=512, N=512, K=64, batch=2, batch2=1, bias_ptr=None, epi=4, persistent=1, cap=4, sC=512 * 512):
        check(lib().rald_op_gemm_nt_256_batched(A.data_ptr(), 64, 512 * 64, B.data_ptr(), 64, 512 * 64, Cc.data_ptr(), 512, sC, bias_ptr, M, N, K,
                                                batch, batch2, 1.0, 1 << 30, epi, persistent, cap, None))

    for kw, msg in (({"M": 384}, "full tiles"), ({"N": 640}, "full tiles"), ({"K": 96}, "full tiles"), ({"bias_ptr": bias.data_ptr()}, "no bias"),
                    ({"batch2": 2}, "batch2"), ({"cap": 0}, "max_workgroups"), ({"cap": -3}, "max_workgroups"), ({"batch": 0}, "batch"),
                    ({"epi": 0}, "EPI_SOFTMAX64 only"), ({"epi": 1}, "EPI_BF16, EPI_GEGLU or EPI_SOFTMAX64"), ({"sC": 512 * 512 - 8}, "overlap")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
