"""Each training entry point of the library against a plain float64 statement of the same operation, computed on the CPU from exactly
the values the kernel read (bf16 inputs widened exactly).  Backward kernels are checked against float64 autograd of the forward as the
reference model writes it, never against a hand-derived gradient.  Shapes sit one below, at and one above the kernels' vector widths,
tiles and rows per workgroup; samples and groups carry distinct values (B >= 3); accumulated outputs start from non-zero values and
written ones from NaN; guard rows, gaps and padding hold a sentinel that must survive.

Bounds, per element (or per row of a reduction):
  fp32 results   |got - ref| <= k * 2^-24 * (sum of the absolute terms that make the result), k stated per check
  bf16 results   one bf16 ulp of the float64 value + the fp32 bound of the value before rounding
  casts and pure data movement: bit-identical to torch's bf16 rounding of the fp32 value.
Each check prints the measured k ("ratio"); the bound is at most 2.5 times the worst value measured on an MI355X (docstrings).

The argument-check tests at the end run on the CPU: every check they exercise comes before the entry's first HIP call."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
U = 2.0 ** -24


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _f64(t):
    return t.detach().cpu().double()


def _ratio(got, ref, terms, atol=0.0):
    """max |got - ref| / (2^-24 * terms) over the elements (fp32 result); terms below the normal range count as 2^-126.  atol: an absolute
    allowance taken off first (2^-126 for results of the hardware exp, which keeps its relative precision only for normal results)."""
    err = ((_f64(got) - ref).abs() - atol).clamp_min(0)
    r = err / (U * terms.clamp_min(2.0 ** -126))
    r = torch.where(torch.isnan(err), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def _ratio16(got, ref, terms, atol=0.0):
    """bf16 result: the error beyond one bf16 ulp of the float64 value (and atol, as in _ratio), in units of 2^-24 * terms."""
    a = ref.abs().clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
    err = (_f64(got.float()) - ref).abs()
    r = (err - ulp - atol).clamp_min(0) / (U * terms.clamp_min(2.0 ** -126))
    r = torch.where(torch.isnan(err), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def _le(name, value, bound):
    print(f"ratio {name}: {value:.3g} (bound {bound})")
    assert value <= bound, (name, value, bound)


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


SENT = -12345.5                               # guard value (compared bit for bit in the buffer's own dtype)


def _guarded(n, extra, dtype=torch.float32, fill=float("nan")):
    """a device buffer of n + extra elements: the first n filled with `fill`, the guard tail with SENT"""
    buf = torch.full((n + extra,), SENT, dtype=dtype, device="cuda")
    buf[:n] = fill
    return buf


def _guard_ok(buf, n):
    tail = buf[n:]
    return bool(torch.equal(_bits(tail), _bits(torch.full_like(tail, SENT))))


# ---- train_kernels.hip -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M,N,K,bound", [(70, 130, 300, 4), (70, 130, 200, 10), (63, 65, 17, 9), (64, 64, 15, 9), (1030, 1030, 290, 14)])
def test_sgemm_acc_transposes_strides_split_k_against_float64(M, N, K, bound):
    """rald_op_sgemm_acc: C[m][n] += alpha * sum_k A(m,k) B(n,k) in all four trans_a / trans_b forms, leading dimensions above the natural
    width (the gaps hold NaN: a read of them poisons the result), alpha = -0.75, C a window of a sentinel-filled buffer (guard rows past M,
    gap columns past N).  70 x 130 x 300 has 6 tiles and K > 256: the split-K path (fp32 atomics); the other shapes run the single pass
    (K <= 256, or 289 tiles at 1030 x 1030).  Measured k: 1.73, 4.62, 3.94, 3.71, 5.88 in the order of the shapes; bounds 4, 10, 9, 9, 14."""
    from rald_amd import train_ops as TO
    g = _g(100 + K)
    alpha = -0.75
    worst = 0.0
    for ta in (False, True):
        for tb in (False, True):
            Ab = torch.full((K, M + 5) if ta else (M, K + 5), float("nan"))
            Bb = torch.full((K, N + 3) if tb else (N, K + 3), float("nan"))
            A = torch.randn(Ab[:, :M].shape if ta else Ab[:, :K].shape, generator=g)
            B = torch.randn(Bb[:, :N].shape if tb else Bb[:, :K].shape, generator=g)
            (Ab[:, :M] if ta else Ab[:, :K]).copy_(A)
            (Bb[:, :N] if tb else Bb[:, :K]).copy_(B)
            Ad, Bd = Ab.cuda(), Bb.cuda()
            Cb = torch.full((M + 3, N + 7), SENT, device="cuda")
            C0 = torch.randn(M, N, generator=g)
            Cb[:M, :N] = C0.cuda()
            TO.sgemm_acc(Ad[:, :M] if ta else Ad[:, :K], Bd[:, :N] if tb else Bd[:, :K], Cb[:M, :N], trans_a=ta, trans_b=tb, alpha=alpha)
            Am = A.double().t() if ta else A.double()                   # [M, K]
            Bm = B.double().t() if tb else B.double()                   # [N, K]
            ref = C0.double() + alpha * Am @ Bm.t()
            terms = C0.double().abs() + abs(alpha) * Am.abs() @ Bm.abs().t()
            worst = max(worst, _ratio(Cb[:M, :N], ref, terms))
            assert bool((Cb[:M, N:] == SENT).all()) and bool((Cb[M:] == SENT).all()), (ta, tb)
    _le(f"sgemm_acc {M}x{N}x{K}", worst, bound)


@gpu
def test_silu_forward_backward_against_float64_autograd_including_the_exp_overflow_edge():
    """rald_op_silu_fwd / _bwd (train_dit.silu, silu_bwd) on 1 000 + edge values: |x| from 88 to 100 (exp(-x) overflows fp32 below
    x = -88.72; 1 / (1 + exp(-x)) then flushed silu and its gradient to 0 where they are ~1e-37), the zero of the derivative, 0 and
    denormal-range inputs.  Reference: F.silu in float64 and its autograd; sigmoid counts as an fp32 intermediate (at least 2^-126 in the
    terms).  Measured k: forward 2.86, backward 11.8; bounds 7, 28."""
    from rald_amd import train_dit as TD
    g = _g(7)
    edge = torch.tensor([-100.0, -95.0, -89.0, -88.75, -88.7, -88.0, -87.0, 87.0, 88.0, 88.7, 89.0, 100.0, 0.0, -0.0, 1e-30, -1e-30, -1.2784645,
                         1.2784645, 20.0, -20.0, 40.0, -40.0])
    x = torch.cat([torch.randn(1000, generator=g) * 4, edge])
    dy = torch.randn(x.numel(), generator=g) + 0.1
    y = TD.silu(x.cuda())
    x64 = x.double().requires_grad_()
    y64 = F.silu(x64)
    y64.backward(dy.double())
    s = torch.sigmoid(x.double())
    sn = s.clamp_min(2.0 ** -126)                                   # sigmoid is an fp32 intermediate: below 2^-126 it is subnormal
    _le("silu fwd", _ratio(y, y64.detach(), x.double().abs() * sn), 7)
    dx = TD.silu_bwd(x.cuda(), dy.cuda())
    _le("silu bwd", _ratio(dx, x64.grad, dy.double().abs() * sn * (1 + x.double().abs() * (1 - s))), 28)


@gpu
def test_edm_loss_grad_per_sample_coefficients_and_optional_D():
    """rald_op_edm_loss_grad: B = 4 samples of 300 elements (not a multiple of 256) with distinct {c_skip, c_out, weight}; dF against float64
    autograd of EDMLoss's mean(weight * (c_skip*x + c_out*F - y)^2); D_out against the float64 mix; *loss written (prefilled 7).  dF is
    bit-identical with and without D_out; dF and D_out past `total` keep their sentinel.  Measured k: D 1.52, dF 2.49, loss 0.028;
    bounds 3.5, 6, 0.07."""
    from rald_amd._lib import check, lib
    g = _g(8)
    B, per = 4, 300
    total = B * per
    Fv, xn, y = (torch.randn(total, generator=g) for _ in range(3))
    coef = torch.stack([torch.tensor([0.2 + 0.1 * b, 0.9 - 0.15 * b, 1.5 + 0.7 * b]) for b in range(B)])
    F64 = Fv.double().requires_grad_()
    cs, co, w = (coef[:, j].double().repeat_interleave(per) for j in range(3))
    D64 = cs * xn.double() + co * F64
    loss64 = (w * (D64 - y.double()) ** 2).mean()
    loss64.backward()
    dev = [t.cuda() for t in (Fv, xn, y, coef)]
    outs = []
    for with_d in (True, False):
        dF, Dout = _guarded(total, 64), _guarded(total, 64)
        loss = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
        check(lib().rald_op_edm_loss_grad(*(_p(t) for t in dev), per, total, _p(dF), _p(Dout) if with_d else None, _p(loss), _st()))
        assert _guard_ok(dF, total) and _guard_ok(Dout, total)
        outs.append((dF[:total].clone(), loss.clone()))
        if with_d:
            _le("edm D", _ratio(Dout[:total], D64.detach(), (cs * xn.double()).abs() + (co * Fv.double()).abs()), 3.5)
        else:
            assert bool(torch.isnan(Dout[:total]).all())                      # D_out null: nothing written
    assert torch.equal(outs[0][0], outs[1][0])
    rterms = (cs * xn.double()).abs() + (co * Fv.double()).abs() + y.double().abs()
    _le("edm dF", _ratio(outs[0][0], F64.grad, 2 * w * co.abs() * rterms / total), 6)
    for _, loss in outs:                                                  # (a float64 atomic sum: its order varies launch to launch)
        _le("edm loss", _ratio(loss, loss64.detach().reshape(1), (w * rterms ** 2).mean().reshape(1)), 0.07)


@gpu
@pytest.mark.parametrize("cols,bound", [(1, 2.8), (63, 3.3), (64, 3.3), (65, 2.7), (300, 6)])
def test_row_lse_wide_range_and_one_dominant_entry(cols, bound):
    """rald_op_row_lse (train_ops.row_lse): 13 rows (not a multiple of the 4 rows of a workgroup) spanning +-80 after the scale, one row where
    a single entry dominates, one constant row; against torch.logsumexp in float64.  Terms: max |scale*S| + log(cols) + 1.
    Measured k: 1.14, 1.35, 1.33, 1.08, 2.49 in the order of cols; bounds 2.8, 3.3, 3.3, 2.7, 6."""
    from rald_amd import train_ops as TO
    g = _g(9 + cols)
    scale = 0.3
    S = (torch.rand(13, cols, generator=g) * 160 - 80) / scale
    S[1] = -80 / scale
    S[1, cols // 2] = 80 / scale
    S[2] = 1.5
    lse = TO.row_lse(S.cuda(), scale)
    a = S.double() * scale
    ref = torch.logsumexp(a, dim=-1)
    _le(f"row_lse cols={cols}", _ratio(lse, ref, a.abs().amax(-1) + math.log(cols) + 1), bound)


@gpu
@pytest.mark.parametrize("heads,bound", [(1, 0.95), (8, 1.4)])
def test_rowdot_heads_batch_head_query_layout(heads, bound):
    """rald_op_rowdot_heads: delta[b][h][q] = <dO, O> over head h of row b*nq + q, B = 3, nq = 37: every (b, h, q) against float64 sums of the
    exact bf16 products (terms: sum |dO*O|); the 16 floats after the table keep their sentinel.  Measured k: 0.39 (1 head), 0.58 (8);
    bounds 0.95, 1.4."""
    from rald_amd._lib import check, lib
    g = _g(10 + heads)
    B, nq = 3, 37
    M = B * nq
    dO = torch.randn(M, heads * 64, generator=g).bfloat16()
    O = (torch.randn(M, heads * 64, generator=g) + torch.arange(M)[:, None] * 0.01).bfloat16()
    delta = _guarded(B * heads * nq, 16)
    dOd, Od = dO.cuda(), O.cuda()
    check(lib().rald_op_rowdot_heads(_p(dOd), _p(Od), M, heads, nq, _p(delta), _st()))
    torch.cuda.synchronize()
    prod = (dO.double() * O.double()).view(B, nq, heads, 64)
    ref = prod.sum(-1).permute(0, 2, 1).reshape(-1)
    terms = prod.abs().sum(-1).permute(0, 2, 1).reshape(-1)
    assert _guard_ok(delta, B * heads * nq)
    _le(f"rowdot_heads h={heads}", _ratio(delta[:B * heads * nq], ref, terms), bound)


@gpu
@pytest.mark.parametrize("by_col", [0, 1])
def test_attn_bwd_elem_strided_row_and_column_normalisers(by_col):
    """rald_op_attn_bwd_elem (train_ops.attn_bwd_elem): S, dP [3][5][12], lse / delta read at b*vbatch_stride + i*vstride (vstride 2,
    vbatch_stride 27; every other slot holds NaN, so a shifted index poisons the result) with i = row (by_col 0) or column (by_col 1).
    P = exp(scale*S - lse[i]) and dS = P*(dP - delta[i])*scale against float64; with and without P (dS bit-identical); 32 bf16 after each
    output keep their sentinel.  Measured: every P and dS within one bf16 ulp of the float64 value (k = 0); bound 0."""
    from rald_amd import train_ops as TO
    g = _g(11 + by_col)
    Bt, R, Cc, vs, vbs, scale = 3, 5, 12, 2, 27, 0.125
    S = torch.randn(Bt, R, Cc, generator=g) * 6
    S[1, 2, 3] = 90.0                                             # one peaked score
    dP = torch.randn(Bt, R, Cc, generator=g)
    a = S.double() * scale
    nrm = torch.logsumexp(a, dim=2 if by_col == 0 else 1)           # [Bt, R] or [Bt, Cc]
    lse = torch.full((Bt * vbs,), float("nan"))
    delta = torch.full((Bt * vbs,), float("nan"))
    n_i = nrm.shape[1]
    for b in range(Bt):
        for i in range(n_i):
            lse[b * vbs + i * vs] = float(nrm[b, i]) + 0.05 * (b - i % 3)
            delta[b * vbs + i * vs] = 0.3 * b - 0.1 * i
    idx = (torch.arange(Bt)[:, None, None] * vbs + (torch.arange(R)[None, :, None] if by_col == 0 else torch.arange(Cc)[None, None, :]) * vs)
    idx = idx.expand(Bt, R, Cc)
    l64, d64 = lse.double()[idx], delta.double()[idx]
    P64 = torch.exp(a - l64)
    dS64 = P64 * (dP.double() - d64) * scale
    tP = P64 * ((a).abs() + l64.abs() + 1)
    tS = scale * P64 * (dP.double().abs() + d64.abs()) + scale * (dP.double() - d64).abs() * tP
    n = Bt * R * Cc
    outs = []
    for with_p in (True, False):
        Pb = _guarded(n, 32, torch.bfloat16)
        dSb = _guarded(n, 32, torch.bfloat16)
        TO.attn_bwd_elem(S.cuda(), dP.cuda(), lse.cuda(), delta.cuda(), Bt, R, Cc, vbs, vs, scale, by_col, Pb if with_p else None, dSb)
        assert _guard_ok(dSb, n) and _guard_ok(Pb, n)
        outs.append(dSb[:n].clone())
        if with_p:
            _le(f"attn_bwd_elem P by_col={by_col}", _ratio16(Pb[:n], P64.reshape(-1), tP.reshape(-1)), 0)
        else:
            assert bool(torch.isnan(Pb[:n].float()).all())
    assert torch.equal(outs[0], outs[1])
    _le(f"attn_bwd_elem dS by_col={by_col}", _ratio16(outs[0], dS64.reshape(-1), tS.reshape(-1)), 0)


# ---- small.hip -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("channels,bound", [(256, 1.8), (6, 1.2)])
def test_posemb_against_float64(channels, bound):
    """rald_op_posemb: out [n, channels] = cat[cos, sin](outer(t, (1/10000)^(k/half))), 7 distinct noise levels (c_noise = ln(sigma)/4 spans
    about [-1.6, 1.1]; wider here) against float64; the row after the table keeps its sentinel.  Terms: |argument| + 1 (the argument is
    formed in fp32 as PositionalEmbedding does).  Measured k: 0.75 (256 channels), 0.50 (6); bounds 1.8, 1.2."""
    from rald_amd._lib import check, lib
    t = torch.tensor([-2.0, -1.55, -0.3, 0.0, 0.01, 1.1, 3.0])
    n, half = t.numel(), channels // 2
    out = _guarded(n * channels, channels)
    td = t.cuda()
    check(lib().rald_op_posemb(_p(td), _p(out), n, channels, _st()))
    torch.cuda.synchronize()
    assert _guard_ok(out, n * channels)
    arg = t.double()[:, None] * (1.0 / 10000.0) ** (torch.arange(half, dtype=torch.float64) / half)
    ref = torch.cat([arg.cos(), arg.sin()], dim=1)
    terms = torch.cat([arg.abs() + 1, arg.abs() + 1], dim=1)
    _le(f"posemb C={channels}", _ratio(out[:n * channels].view(n, channels), ref, terms), bound)


@gpu
@pytest.mark.parametrize("n", [4, 1028, 4 * (2048 * 256 + 5)])
def test_cast_bf16_rounds_like_torch_bit_for_bit(n):
    """rald_op_cast_bf16 (train_ops.cast_bf16): round-to-nearest-even ties in both directions, values that round to +-inf, +-inf, the largest
    finite bf16 values, denormals and signed zeros are bit-identical to torch's bf16 rounding of the fp32 value; NaN stays NaN (torch's own
    NaN bits are not canonical).  n = 4 * (2048 * 256 + 5) runs the grid-stride loop (at most 2048 workgroups)."""
    from rald_amd import train_ops as TO
    g = _g(12)
    x = torch.randn(n, generator=g) * 3
    special = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8), -(1 + 3 * 2 ** -8), 3.3961e38, -3.3961e38, 3.3895e38, 3.3896e38,
                            float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 1e-40, -1e-40, 2 ** -133, 1.0, 65504.0 + 2 ** 5,
                            2 ** -126 * (1 + 2 ** -8), 3.4028235e38])
    k = min(n, special.numel())
    x[:k] = special[:k]
    ties = (torch.randint(-2 ** 15, 2 ** 15, (n // 3,), generator=g).to(torch.int32) << 16) | (1 << 15)     # exact halfway points
    x[k:k + ties.numel()] = ties.view(torch.float32)[: max(0, min(ties.numel(), n - k))]
    got = TO.cast_bf16(x.cuda()).cpu()
    want = x.bfloat16()
    nan = torch.isnan(x)
    assert bool(torch.isnan(got[nan].float()).all())
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))


# ---- radar_train.hip -------------------------------------------------------------------------------------------------------------------
@gpu
def test_conv_pack_weights_both_forms_with_padding():
    """rald_op_conv_pack_weights (train_encoder.pack_conv): W [20][6][27] -> forward [Cout][27][pad_to = 8] and dgrad [Cin][27][pad_to = 24]
    (taps flipped), bit-identical to torch's bf16 rounding of the permuted parameter, zeros in the padding."""
    from rald_amd import train_encoder as TE
    g = _g(13)
    Cout, Cin = 20, 6
    W = torch.randn(Cout, Cin, 3, 3, 3, generator=g)
    fwd = TE.pack_conv(W.cuda(), dgrad=False, pad_to=8).cpu()
    want = torch.zeros(Cout, 27, 8, dtype=torch.bfloat16)
    want[:, :, :Cin] = W.view(Cout, Cin, 27).permute(0, 2, 1).bfloat16()
    assert torch.equal(fwd.view(torch.int16), want.view(torch.int16))
    dg = TE.pack_conv(W.cuda(), dgrad=True, pad_to=24).cpu()
    want = torch.zeros(Cin, 27, 24, dtype=torch.bfloat16)
    want[:, :, :Cout] = W.view(Cout, Cin, 27).flip(2).permute(1, 2, 0).bfloat16()
    assert torch.equal(dg.view(torch.int16), want.view(torch.int16))


@gpu
@pytest.mark.parametrize("M,C,Cpad", [(37, 5, 8), (300, 16, 64), (1, 64, 64)])
def test_pad_channels_bit_exact(M, C, Cpad):
    """rald_op_pad_channels (train_ops.pad_channels): bf16 of the fp32 rows, bit for bit, zero channels C .. Cpad-1."""
    from rald_amd import train_ops as TO
    x = torch.randn(M, C, generator=_g(14)) * 5
    got = TO.pad_channels(x.cuda(), Cpad).cpu()
    want = torch.zeros(M, Cpad, dtype=torch.bfloat16)
    want[:, :C] = x.bfloat16()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@gpu
@pytest.mark.parametrize("OD,OH,OW,C", [(1, 2, 3, 5), (2, 1, 1, 64), (3, 2, 2, 3)])
def test_zero_insert2_bit_exact(OD, OH, OW, C):
    """rald_op_zero_insert2: dY [3][OD][OH][OW][C] fp32 -> bf16 on the even positions of the 2x grid, zeros elsewhere, bit for bit; the 64
    bf16 after the grid keep their sentinel."""
    from rald_amd._lib import check, lib
    B = 3
    dy = torch.randn(B, OD, OH, OW, C, generator=_g(15)) * 4
    n = B * 8 * OD * OH * OW * C
    out = _guarded(n, 64, torch.bfloat16)
    dyd = dy.cuda()
    check(lib().rald_op_zero_insert2(_p(dyd), _p(out), B, OD, OH, OW, C, _st()))
    torch.cuda.synchronize()
    assert _guard_ok(out, n)
    want = torch.zeros(B, 2 * OD, 2 * OH, 2 * OW, C, dtype=torch.bfloat16)
    want[:, ::2, ::2, ::2] = dy.bfloat16()
    assert torch.equal(out[:n].cpu().view(torch.int16), want.reshape(-1).view(torch.int16))


def _cube(B, D, H, W, ch, seed):
    """channels-last cube whose channel 0 is the data and every other channel NaN (a read of the wrong channel poisons the result)"""
    c = torch.full((B, D, H, W, ch), float("nan"))
    c[..., 0] = torch.randn(B, D, H, W, generator=_g(seed)) * 2
    return c


@gpu
@pytest.mark.parametrize("D,H,W,ch", [(1, 2, 3, 3), (2, 1, 2, 2), (3, 4, 5, 1)])
def test_patches27_zero_padding_at_every_face(D, H, W, ch):
    """rald_op_patches27: per voxel the 27-neighbourhood of channel 0 (taps kd*9 + kh*3 + kw, zero outside the volume) and 5 zeros, bf16,
    bit-identical to F.pad + unfold of the bf16-rounded channel; sides of 1 and 2 put every tap of some voxel outside; the other cube channels
    hold NaN; the 64 bf16 after the patches keep their sentinel."""
    from rald_amd._lib import check, lib
    B = 3
    cube = _cube(B, D, H, W, ch, 16)
    nv = B * D * H * W
    out = _guarded(nv * 32, 64, torch.bfloat16)
    cubed = cube.cuda()
    check(lib().rald_op_patches27(_p(cubed), ch, _p(out), B, D, H, W, _st()))
    torch.cuda.synchronize()
    assert _guard_ok(out, nv * 32)
    v = F.pad(cube[..., 0], (1, 1, 1, 1, 1, 1))
    taps = [v[:, kd:kd + D, kh:kh + H, kw:kw + W] for kd in range(3) for kh in range(3) for kw in range(3)]
    want = torch.zeros(nv, 32, dtype=torch.bfloat16)
    want[:, :27] = torch.stack(taps, dim=-1).reshape(nv, 27).bfloat16()
    assert torch.equal(out[:nv * 32].cpu().view(torch.int16), want.reshape(-1).view(torch.int16))


@gpu
@pytest.mark.parametrize("D,H,W,ch,Cout,bound", [(1, 2, 3, 3, 64, 5.5), (2, 1, 2, 2, 16, 4.9), (3, 4, 5, 1, 64, 9)])
def test_conv_in_reads_channel_zero_in_place(D, H, W, ch, Cout, bound):
    """rald_op_conv_in: the Cin = 1 first convolution (k3, pad 1) read in place from channel 0 of a [3][D][H][W][ch] cube whose other channels
    are NaN, against F.conv3d in float64; voxel counts that do not fill the last workgroup; the 64 floats after the output keep their
    sentinel.  Terms: |bias| + sum |w * x|.  Measured k: 2.22, 1.99, 3.68 in the order of the shapes; bounds 5.5, 4.9, 9."""
    from rald_amd._lib import check, lib
    B = 3
    g = _g(17)
    cube = _cube(B, D, H, W, ch, 18)
    Wt = torch.randn(Cout, 1, 3, 3, 3, generator=g) / 5
    bias = torch.randn(Cout, generator=g)
    nv = B * D * H * W
    out = _guarded(nv * Cout, 64)
    cubed, Wd, bd = cube.cuda(), Wt.cuda(), bias.cuda()
    check(lib().rald_op_conv_in(_p(cubed), ch, 1, _p(Wd), _p(bd), _p(out), B, D, H, W, Cout, _st()))
    torch.cuda.synchronize()
    assert _guard_ok(out, nv * Cout)
    x = cube[..., 0].double()[:, None]
    ref = F.conv3d(x, Wt.double(), bias.double(), padding=1).permute(0, 2, 3, 4, 1).reshape(nv, Cout)
    terms = (F.conv3d(x.abs(), Wt.double().abs(), None, padding=1).permute(0, 2, 3, 4, 1).reshape(nv, Cout) + bias.double().abs())
    _le(f"conv_in {D}x{H}x{W}", _ratio(out[:nv * Cout].view(nv, Cout), ref, terms), bound)


@gpu
@pytest.mark.parametrize("C,bound", [(1, 0), (63, 1.35), (65, 0.74), (130, 0.32)])
def test_rowdot_rows_of_any_width(C, bound):
    """rald_op_rowdot (train_ops.rowdot): 7 rows (not a multiple of the 4 of a workgroup), C not a multiple of 64, against float64 sums of the
    exact bf16 products (terms: sum |a*b|).  Measured k: 0 (C = 1: one exact product), 0.54, 0.30, 0.13; bounds 0, 1.35, 0.74,
    0.32."""
    from rald_amd import train_ops as TO
    g = _g(19 + C)
    a = torch.randn(7, C, generator=g).bfloat16()
    b = (torch.randn(7, C, generator=g) + torch.arange(7)[:, None] * 0.1).bfloat16()
    got = TO.rowdot(a.cuda(), b.cuda())
    prod = a.double() * b.double()
    _le(f"rowdot C={C}", _ratio(got, prod.sum(1), prod.abs().sum(1)), bound)


# ---- ae_kernels.hip --------------------------------------------------------------------------------------------------------------------
def _softmax_rows_input(rows, ld, n, seed):
    g = _g(seed)
    S = torch.full((rows, ld), float("nan"))                          # columns n .. ld-1: NaN (must not be read)
    S[:, :n] = torch.rand(rows, n, generator=g) * 160 - 80
    S[1, :n] = -80.0
    S[1, n // 2] = 80.0                                               # one entry dominates
    return S


def _softmax_terms(s, P):
    d = (s - s.amax(-1, keepdim=True)).abs()
    return P * (d + (P * d).sum(-1, keepdim=True) + 1)


@gpu
@pytest.mark.parametrize("n,ld", [(1, 64), (37, 64), (256, 256), (300, 320)])
def test_softmax_rows_against_float64(n, ld):
    """rald_op_softmax_rows (train_ops.softmax_rows): 5 rows spanning +-80, one dominated by a single entry; n = 1, n below ld, n above the
    256 threads of a workgroup; columns n .. ld-1 of S hold NaN and must come out 0.  bf16 P against float64 softmax; terms
    p * (|s - max| + sum p |s - max| + 1), and 2^-126 absolute where the exp result is subnormal.  Measured: every P within one bf16
    ulp (k = 0); bound 0."""
    from rald_amd import train_ops as TO
    S = _softmax_rows_input(5, ld, n, 20 + n)
    P = TO.softmax_rows(S.cuda(), n).cpu()
    ref = torch.softmax(S[:, :n].double(), dim=-1)
    assert not P[:, n:].float().any() and not torch.isnan(P.float()).any()
    _le(f"softmax_rows n={n}", _ratio16(P[:, :n], ref, _softmax_terms(S[:, :n].double(), ref), atol=2.0 ** -126), 0)


def _posterior_input(B, rows, L, seed):
    g = _g(seed)
    ml = torch.randn(B, rows, 2 * L, generator=g) * torch.tensor([0.5, 1.0, 2.0][:B] + [1.0] * (B - 3))[:, None, None]
    ml[:, :, :L] += torch.arange(B)[:, None, None] * 0.7                   # distinct per-sample kl
    edges = torch.tensor([-30.0, 20.0, -29.99, 19.99, -30.01, 20.01, -50.0, 40.0, -30.0, 20.0])
    lv = ml[:, :, L:].reshape(-1).clone()
    lv[:edges.numel()] = edges
    lv[-edges.numel():] = edges
    ml[:, :, L:] = lv.view(B, rows, L)
    eps = torch.randn(B, rows, L, generator=g)
    return ml, eps


def _posterior_ref(ml, eps, L):
    mean, logvar = ml[..., :L], torch.clamp(ml[..., L:], -30.0, 20.0)
    std, var = torch.exp(0.5 * logvar), torch.exp(logvar)
    z = mean + std * eps
    kl = 0.5 * torch.mean(mean ** 2 + var - 1.0 - logvar, dim=[1, 2])
    return z, kl


@gpu
@pytest.mark.parametrize("L,rows,bz,bkl", [(1, 1100, 3.5, 1.4), (2, 700, 3.6, 0.69), (32, 40, 3.3, 0.68)])
def test_posterior_both_branches_per_sample_kl_and_clamp_edges(L, rows, bz, bkl):
    """rald_op_posterior: z = mean + exp(0.5 clamp(logvar, -30, 20)) eps and kl[b] = 0.5 mean(mean^2 + var - 1 - logvar) over B = 3 samples with
    distinct statistics; L = 1, 2 (the scalar branch, L % 4 != 0) and 32 (float4), more elements per sample than the workgroup's 1 024
    threads; logvar exactly -30 and 20, just inside, just outside and far outside.  Against DiagonalGaussianDistribution in float64;
    z / kl past the outputs keep their sentinel; a second launch gives identical bits.  Measured k: z 1.42, 1.45, 1.35 and kl 0.57, 0.28,
    0.27 for L = 1, 2, 32; bounds 3.5, 3.6, 3.3 and 1.4, 0.69, 0.68."""
    from rald_amd._lib import check, lib
    B = 3
    ml, eps = _posterior_input(B, rows, L, 21 + L)
    n = B * rows * L
    mld, epsd = ml.cuda(), eps.cuda()
    res = []
    for _ in range(2):
        z, kl = _guarded(n, 64), _guarded(B, 16)
        check(lib().rald_op_posterior(_p(mld), _p(epsd), _p(z), _p(kl), B, rows, L, _st()))
        torch.cuda.synchronize()
        assert _guard_ok(z, n) and _guard_ok(kl, B)
        res.append((z[:n].clone(), kl[:B].clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    m64 = ml.double()
    zr, klr = _posterior_ref(m64, eps.double(), L)
    mean, lv = m64[..., :L], torch.clamp(m64[..., L:], -30.0, 20.0)
    std = torch.exp(0.5 * lv)
    tz = mean.abs() + std * eps.double().abs() * (1 + 0.5 * lv.abs())
    tkl = 0.5 * torch.mean(mean ** 2 + torch.exp(lv) * (1 + lv.abs()) + 1 + lv.abs(), dim=[1, 2])
    _le(f"posterior z L={L}", _ratio(res[0][0].view(B, rows, L), zr, tz), bz)
    _le(f"posterior kl L={L}", _ratio(res[0][1], klr, tkl), bkl)


# ---- ae_train.hip ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("L,rows", [(2, 300), (32, 40)])
def test_posterior_bwd_against_float64_autograd_with_nullable_gradients(L, rows):
    """rald_op_posterior_bwd: d[mean | logvar] against float64 autograd of (z, kl) as DiagonalGaussianDistribution writes them (torch.clamp
    passes the gradient at -30 and 20 inclusive, not outside), for dz and dkl both given, dz null and dkl null; B = 3 with distinct dkl[b];
    dml written everywhere (prefilled NaN), 64 floats past it keep their sentinel.  Measured k (dmean, dlogvar) for (dz, dkl) = both, dkl
    only, dz only: L = 2: (1.2, 2.27), (2.07, 1.79), (0, 1.92); L = 32: (0.98, 2.72), (1.91, 1.68), (0, 2.12) - dz only gives dmean = dz
    exactly; bounds below."""
    from rald_amd._lib import check, lib
    B = 3
    ml, eps = _posterior_input(B, rows, L, 31 + L)
    g = _g(32)
    dz = torch.randn(B, rows, L, generator=g)
    dkl = torch.tensor([0.7, -1.3, 2.1])
    n2 = B * rows * 2 * L
    dzd, dkld, mld, epsd = dz.cuda(), dkl.cuda(), ml.cuda(), eps.cuda()
    bounds = {2: {(True, True): (3, 5.6), (False, True): (5, 4.4), (True, False): (0, 4.8)},
              32: {(True, True): (2.4, 6.8), (False, True): (4.7, 4.2), (True, False): (0, 5.3)}}[L]
    for use_dz, use_dkl in ((True, True), (False, True), (True, False)):
        m64 = ml.double().requires_grad_()
        z, kl = _posterior_ref(m64, eps.double(), L)
        loss = (z * dz.double()).sum() * use_dz + (kl * dkl.double()).sum() * use_dkl
        loss.backward()
        dml = _guarded(n2, 64)
        check(lib().rald_op_posterior_bwd(_p(dzd) if use_dz else None, _p(dkld) if use_dkl else None, _p(mld), _p(epsd), _p(dml), B, rows, L,
                                          _st()))
        torch.cuda.synchronize()
        assert _guard_ok(dml, n2)
        got = dml[:n2].view(B, rows, 2 * L)
        mean, lvr = ml.double()[..., :L], ml.double()[..., L:]
        lv = lvr.clamp(-30.0, 20.0)
        inside = ((lvr >= -30) & (lvr <= 20)).double()
        kk = dkl.double()[:, None, None].abs() * use_dkl / (rows * L)
        gz = dz.double().abs() * use_dz
        tm = gz + kk * mean.abs()
        tl = inside * (gz * eps.double().abs() * 0.5 * torch.exp(0.5 * lv) * (1 + 0.5 * lv.abs()) + kk * 0.5 * (torch.exp(lv) * (1 + lv.abs()) + 1))
        _le(f"posterior_bwd dmean L={L} dz={use_dz} dkl={use_dkl}", _ratio(got[..., :L], m64.grad[..., :L], tm), bounds[use_dz, use_dkl][0])
        _le(f"posterior_bwd dlogvar L={L} dz={use_dz} dkl={use_dkl}", _ratio(got[..., L:], m64.grad[..., L:], tl), bounds[use_dz, use_dkl][1])


def _ln_ref_terms(x, dh, gamma, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mu) * rstd
    gh = (dh * gamma).abs()
    return rstd * (gh + gh.mean(-1, keepdim=True) + xh.abs() * (gh * xh.abs()).mean(-1, keepdim=True)), xh


@gpu
@pytest.mark.parametrize("rows,bounds", [(1, (2.9, 6, 2.4)), (63, (4.5, 3.4, 3)), (64, (4.7, 3.5, 2.3)), (65, (5.4, 2.9, 2.8)),
                                         (300, (4.9, 2.3, 1.1))])
def test_ln_affine_bwd_row_tails_accumulation_and_bf16_copy(rows, bounds):
    """rald_op_ln_affine_bwd (train_ae.ln_affine_bwd): nn.LayerNorm(512) backward at 1, 63, 64, 65 rows (64 per workgroup) and 300 (5
    workgroups) against float64 autograd of F.layer_norm: dx accumulated into a non-zero prefill, dgamma / dbeta accumulated, the bf16 copy
    written (prefilled NaN) and equal to the fp32 result rounded; without the copy the fp32 results are bit-identical; a second launch
    reproduces them; 64 elements after every output keep their sentinel.  Measured k (dx, dgamma, dbeta): rows 1 (1.19, 2.43, 0.99), 63
    (1.84, 1.36, 1.2), 64 (1.9, 1.4, 0.95), 65 (2.16, 1.18, 1.15), 300 (1.99, 0.92, 0.46); bounds as parametrized."""
    from rald_amd import train_ae as TA
    g = _g(40 + rows)
    D = 512
    x = torch.randn(rows, D, generator=g) * 1.7 + torch.arange(rows)[:, None] * 0.05
    dh = torch.randn(rows, D, generator=g)
    gamma = 1 + 0.3 * torch.randn(D, generator=g)
    dx0, dg0, db0 = torch.randn(rows, D, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
    x64 = x.double().requires_grad_()
    g64 = gamma.double().requires_grad_()
    b64 = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x64, (D,), g64, b64, eps=1e-5).backward(dh.double())
    xd, dhd, gd = x.cuda(), dh.cuda(), gamma.cuda()
    res = []
    for with_bf16 in (True, False, True):
        dx = _guarded(rows * D, 64, fill=0.0); dx[:rows * D] = dx0.reshape(-1).cuda()
        dg = _guarded(D, 64, fill=0.0); dg[:D] = dg0.cuda()
        db = _guarded(D, 64, fill=0.0); db[:D] = db0.cuda()
        dxb = _guarded(rows * D, 64, torch.bfloat16)
        TA.ln_affine_bwd(xd, dhd, gd, dx[:rows * D].view(rows, D), dg[:D], db[:D], dx_bf16=dxb[:rows * D].view(rows, D) if with_bf16 else None)
        assert _guard_ok(dx, rows * D) and _guard_ok(dg, D) and _guard_ok(db, D) and _guard_ok(dxb, rows * D)
        if with_bf16:
            assert torch.equal(dxb[:rows * D], dx[:rows * D].bfloat16())
        else:
            assert bool(torch.isnan(dxb[:rows * D].float()).all())
        res.append((dx[:rows * D].clone(), dg[:D].clone(), db[:D].clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    for a, b in zip(res[0], res[2]):
        assert torch.equal(a, b)
    t, xh = _ln_ref_terms(x.double(), dh.double(), gamma.double())
    _le(f"ln_affine_bwd dx rows={rows}", _ratio(res[0][0].view(rows, D), dx0.double() + x64.grad, dx0.double().abs() + t), bounds[0])
    _le(f"ln_affine_bwd dgamma rows={rows}", _ratio(res[0][1], dg0.double() + g64.grad, dg0.double().abs() + (dh.double() * xh).abs().sum(0)), bounds[1])
    _le(f"ln_affine_bwd dbeta rows={rows}", _ratio(res[0][2], db0.double() + b64.grad, db0.double().abs() + dh.double().abs().sum(0)), bounds[2])


def _pe_features(pts, basis):
    """the 51 PointEmbed features in float64 from the fp32 argument p . basis as the reference forms it (torch fp32)"""
    arg = (pts.float() @ basis.float()).double()
    return torch.cat([arg.sin(), arg.cos(), pts.double()], dim=-1)


@gpu
@pytest.mark.parametrize("rows,bounds", [(1, (6, 2.4)), (63, (9, 4.9)), (64, (7.9, 4.7)), (65, (8.8, 5.1)), (511, (9, 12)), (512, (11, 10)),
                                         (513, (8.9, 10.9)), (1100, (5.1, 16))])
def test_pe_wgrad_row_tails_and_reproducibility(rows, bounds):
    """rald_op_pe_wgrad (train_ae.pe_wgrad): dW [512][51] += dY^T . [sin | cos | xyz] and db += column sums of dY with the features recomputed
    from raw points in [-1, 1] and the real PointEmbed basis (arguments up to 128 pi); 512 rows per workgroup staged 64 at a time: 1, 63,
    64, 65, 511, 512, 513 and 1100 rows (3 workgroups).  Against float64 sums over features taken from the fp32 argument; dW / db
    accumulate into non-zero values; 64 floats after each keep their sentinel; a second launch gives identical bits.
    Measured k (dW, db): rows 1 (2.47, 0.99), 63 (3.71, 1.98), 64 (3.18, 1.88), 65 (3.54, 2.06), 511 (3.64, 4.8), 512 (4.51, 4.01), 513
    (3.57, 4.36), 1100 (2.05, 6.48); bounds as parametrized."""
    from rald_amd import train_ae as TA
    from rald_amd import weights
    g = _g(50 + rows)
    basis = weights.point_embed_basis()
    pts = torch.rand(rows, 3, generator=g) * 2 - 1
    dY = torch.randn(rows, 512, generator=g) + torch.arange(rows)[:, None] * 1e-3
    dW0, db0 = torch.randn(512, 51, generator=g), torch.randn(512, generator=g)
    res = []
    for _ in range(2):
        dW = _guarded(512 * 51, 64, fill=0.0); dW[:512 * 51] = dW0.reshape(-1).cuda()
        db = _guarded(512, 64, fill=0.0); db[:512] = db0.cuda()
        TA.pe_wgrad(dY.cuda(), pts.cuda(), basis.cuda(), dW[:512 * 51].view(512, 51), db[:512])
        assert _guard_ok(dW, 512 * 51) and _guard_ok(db, 512)
        res.append((dW[:512 * 51].clone(), db[:512].clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    f = _pe_features(pts, basis)
    ref = dW0.double() + dY.double().t() @ f
    terms = dW0.double().abs() + dY.double().abs().t() @ f.abs()
    _le(f"pe_wgrad dW rows={rows}", _ratio(res[0][0].view(512, 51), ref, terms), bounds[0])
    _le(f"pe_wgrad db rows={rows}", _ratio(res[0][1], db0.double() + dY.double().sum(0), db0.double().abs() + dY.double().abs().sum(0)), bounds[1])


@gpu
@pytest.mark.parametrize("n", [1, 7, 1000])
def test_point_features_against_float64(n):
    """rald_op_point_features: feat bf16 [n][64] = [sin(p.basis) | cos | xyz | 0 ...] with the real PointEmbed basis (arguments up to
    128 pi), against float64 sin / cos of the fp32 argument; the 13 pad columns are zero and the row after the table keeps its sentinel.
    Terms: 1 for sin / cos, |p| for xyz.  Measured: every feature within one bf16 ulp (k = 0); bound 0."""
    from rald_amd._lib import check, lib
    from rald_amd import weights
    g = _g(60 + n)
    basis = weights.point_embed_basis()
    pts = torch.rand(n, 3, generator=g) * 2 - 1
    out = _guarded(n * 64, 64, torch.bfloat16)
    ptsd, basisd = pts.cuda(), basis.cuda()
    check(lib().rald_op_point_features(_p(ptsd), _p(basisd), _p(out), n, _st()))
    torch.cuda.synchronize()
    assert _guard_ok(out, n * 64)
    got = out[:n * 64].view(n, 64).cpu()
    assert not got[:, 51:].float().any()
    f = _pe_features(pts, basis)
    terms = torch.cat([torch.ones(n, 48, dtype=torch.float64), pts.double().abs()], dim=1)
    _le(f"point_features n={n}", _ratio16(got[:, :51], f, terms), 0)


@gpu
def test_scale_rows_both_modes_per_sample_scales_with_dropped_samples():
    """rald_op_scale_rows (train_ae.scale_rows_add / scale_rows_bf16): rows_per_sample = 5, B = 4 with scales {1.25, 0, 2.5, 1/0.9} (a dropped
    sample in the middle), 12 columns.  Accumulate mode: x += s[r / 5] * y is the fp32 fma of the float64 product (k <= 1), rows of the
    dropped sample bit-unchanged, 64 floats past x keep their sentinel; bf16 mode: bit-identical to torch's bf16 rounding of the fp32
    product."""
    from rald_amd import train_ae as TA
    g = _g(70)
    rps, B, cols = 5, 4, 12
    rows = rps * B
    s = torch.tensor([1.25, 0.0, 2.5, 1 / 0.9])
    y = torch.randn(rows, cols, generator=g)
    x0 = torch.randn(rows, cols, generator=g)
    x = _guarded(rows * cols, 64, fill=0.0); x[:rows * cols] = x0.reshape(-1).cuda()
    TA.scale_rows_add(y.cuda(), s.cuda(), x[:rows * cols].view(rows, cols), rps)
    assert _guard_ok(x, rows * cols)
    got = x[:rows * cols].view(rows, cols).cpu()
    sr = s.repeat_interleave(rps)[:, None]
    _le("scale_rows add", _ratio(got, x0.double() + sr.double() * y.double(), (x0.double() + sr.double() * y.double()).abs()), 1)
    assert torch.equal(got[rps:2 * rps], x0[rps:2 * rps])
    out = TA.scale_rows_bf16(y.cuda(), s.cuda(), rps).cpu()
    assert torch.equal(out.view(torch.int16), (sr * y).bfloat16().view(torch.int16))


@gpu
@pytest.mark.parametrize("n,ld", [(1, 64), (37, 64), (300, 320)])
def test_softmax_bwd_rows_against_float64_autograd(n, ld):
    """rald_op_softmax_bwd_rows: P = softmax(S[r][:n]) and dS = P (dP - delta[r]) * scale for 5 rows spanning +-80 (one dominated by a single
    entry), delta[r] = <P, dP> of the row rounded to fp32; reference: float64 autograd of softmax (the fp32 delta enters the
    terms: dP - delta cancels).  n = 1, n below ld, n above 256; P nullable (dS bit-identical); columns n .. ld-1 of both written 0 (prefilled
    NaN; S / dP hold NaN there); the row after the outputs keeps its sentinel; a second launch gives identical bits.  2^-126 absolute is allowed where the exp result is
    subnormal.  Measured: every P and dS within one bf16 ulp (k = 0); bound 0."""
    from rald_amd._lib import check, lib
    rows, scale = 5, 0.0441941738
    S = _softmax_rows_input(rows, ld, n, 80 + n)
    g = _g(81)
    dP = torch.full((rows, ld), float("nan"))
    dP[:, :n] = torch.randn(rows, n, generator=g)
    s64 = S[:, :n].double().requires_grad_()
    P64 = torch.softmax(s64, dim=-1)
    delta = (P64.detach() * dP[:, :n].double()).sum(-1).float()
    (P64 * dP[:, :n].double()).sum().backward()
    ref = s64.grad * scale
    Sd, dPd, dd = S.cuda(), dP.cuda(), delta.cuda()
    res = []
    for with_p in (True, True, False):
        Pb, dSb = _guarded(rows * ld, ld, torch.bfloat16), _guarded(rows * ld, ld, torch.bfloat16)
        check(lib().rald_op_softmax_bwd_rows(_p(Sd), _p(dPd), _p(dd), rows, ld, n, scale, _p(Pb) if with_p else None, _p(dSb), _st()))
        torch.cuda.synchronize()
        assert _guard_ok(Pb, rows * ld) and _guard_ok(dSb, rows * ld)
        res.append((Pb[:rows * ld].view(rows, ld).cpu(), dSb[:rows * ld].view(rows, ld).cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][1], res[2][1])
    assert bool(torch.isnan(res[2][0].float()).all())
    P, dS = res[0]
    assert not P[:, n:].float().any() and not dS[:, n:].float().any()
    tP = _softmax_terms(S[:, :n].double(), P64.detach())
    d64 = dP[:, :n].double()
    tS = scale * (P64.detach() * (d64.abs() + delta.double().abs()[:, None]) + (d64 - delta.double()[:, None]).abs() * tP)
    _le(f"softmax_bwd_rows P n={n}", _ratio16(P[:, :n], P64.detach(), tP, atol=2.0 ** -126), 0)
    _le(f"softmax_bwd_rows dS n={n}", _ratio16(dS[:, :n], ref, tS, atol=2.0 ** -126 * scale * (d64.abs() + delta.double().abs()[:, None])), 0)


# ---- gemm.hip --------------------------------------------------------------------------------------------------------------------------
def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_g(seed)).float()


@gpu
@pytest.mark.parametrize("M,N,K", [(200, 136, 64), (128, 64, 128), (64, 96, 64)])
def test_gemm_nt2_two_batch_levels_on_column_slices_exact_integers(M, N, K):
    """rald_op_gemm_nt2 (train_ops.gemm2), the attention backward's head-batched products: C[b1][b2] = alpha * A[b1][b2] . B[b1][b2]^T + bias
    on small integers (every sum exact in fp32), batch = 3 outer x batch2 = 2 inner, the inner level a column slice of a wider row (strideA2 /
    strideB2 / strideC2 = a column offset, leading dimensions = the full row), alpha = 0.5; epilogue 1 (fp32) exact, epilogue 0 (bf16) equal
    to the exact value rounded; an asymmetric B catches a transposed write; the 8 columns past the slices and the rows past M keep the
    sentinel."""
    from rald_amd import train_ops as TO
    b1, b2, alpha = 3, 2, 0.5
    lda, ldb = b2 * K + 8, b2 * K + 16
    A = _ints((b1, M, lda), -3, 3, 90)
    Bm = _ints((b1, N, ldb), -2, 2, 91) + (torch.arange(N) % 3 == 0).float()[None, :, None]
    bias = _ints((N,), -4, 4, 92)
    Asl = A[:, :, :b2 * K].view(b1, M, b2, K).permute(0, 2, 1, 3)          # [b1, b2, M, K]
    Bsl = Bm[:, :, :b2 * K].view(b1, N, b2, K).permute(0, 2, 1, 3)
    ref = alpha * Asl @ Bsl.transpose(-1, -2) + bias                          # [b1, b2, M, N]
    ldc = b2 * N + 8
    for epi, dt in ((1, torch.float32), (0, torch.bfloat16)):
        Cb = torch.full((b1, M + 2, ldc), SENT, device="cuda", dtype=dt)
        Ad, Bd = A.cuda().bfloat16(), Bm.cuda().bfloat16()
        TO.gemm2(Ad, lda, M * lda, K, Bd, ldb, N * ldb, K, Cb, ldc, (M + 2) * ldc, N, M, N, K, b1, b2, epilogue=epi, alpha=alpha, bias=bias.cuda())
        got = Cb[:, :M, :b2 * N].view(b1, M, b2, N).permute(0, 2, 1, 3).float().cpu()
        want = ref if epi == 1 else ref.bfloat16().float()
        assert torch.equal(got, want), epi
        assert bool((Cb[:, :M, b2 * N:].float() == float(torch.tensor(SENT).to(dt))).all()) and bool((Cb[:, M:].float() == float(torch.tensor(SENT).to(dt))).all())


# ---- argument checks (CPU: each fires before the entry's first HIP call) --------------------------------------------------------------
@pytest.fixture()
def L_cpu():
    if torch.cuda.is_available():
        pytest.skip("argument checks run where no GPU is visible: a check that failed to fire would launch on dummy pointers")
    from rald_amd._lib import lib
    return lib()


def _refused(L, rc, *words):
    assert rc != 0
    msg = L.rald_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


DUMMY = 1 << 20                                                       # a 16-byte aligned non-null address that is never dereferenced


def test_argument_checks_name_the_constraint(L_cpu):
    L, d = L_cpu, DUMMY
    _refused(L, L.rald_op_geglu_fwd(d, d, 10, 12, None), "multiple of 8")
    _refused(L, L.rald_op_geglu_bwd(d, d, d, 10, 12, None), "multiple of 8")
    _refused(L, L.rald_op_attn_bwd_elem(d, d, d, d, 2, 5, 10, 10, 1, 0.1, 0, None, d, None), "multiple of 4")
    _refused(L, L.rald_op_scale_rows(d, d, d, None, 10, 6, 5, None), "cols", "multiple of 4")
    _refused(L, L.rald_op_scale_rows(d, d, None, d, 10, 6, 5, None), "cols", "multiple of 4")
    _refused(L, L.rald_op_ln_mod_bwd(d, d, d, 0, 16, 1.0, 1e-5, 32, 256, d, None, d, d, None), "512")
    _refused(L, L.rald_op_ln_mod_bwd(d, d, d, 0, 24, 1.0, 1e-5, 32, 512, d, None, d, d, None), "rows_per_group")
    _refused(L, L.rald_op_groupnorm_bwd(d, d, d, d, d, 0, d, None, d, d, d, 2, 100, 96, 0, 0, None), "64, 128 or 256")
    _refused(L, L.rald_op_groupnorm_bwd(d, d, d, d, d, 0, d, None, d, d, d, 2, 100, 512, 0, 0, None), "64, 128 or 256")
    _refused(L, L.rald_op_cast_bf16(d, d, 6, None), "multiple of 4")
    _refused(L, L.rald_op_softmax_rows(d, 30, d, 64, 4, 37, None), "ld", ">= n")
    _refused(L, L.rald_op_softmax_rows(d, 64, d, 30, 4, 37, None), "ld", ">= n")
    _refused(L, L.rald_op_softmax_bwd_rows(d, d, d, 4, 30, 37, 0.1, None, d, None), "ld", ">= n")
    need = L.rald_op_ln_affine_bwd_scratch_bytes(100)
    _refused(L, L.rald_op_ln_affine_bwd(d, d, d, 1e-5, 100, d, None, d, d, d, need - 4, None), "scratch too small")
    _refused(L, L.rald_op_ln_affine_bwd(d, d, d, 1e-5, 100, d, None, d, d, d + 4, need, None), "scratch", "16-byte aligned")
    _refused(L, L.rald_op_ln_affine_bwd(d + 4, d, d, 1e-5, 100, d, None, d, d, d, need, None), "16-byte alignment")
    _refused(L, L.rald_op_ln_affine_bwd(d, d, d, 1e-5, 100, d, d + 8, d, d, d, need, None), "16-byte alignment")
    need = L.rald_op_pe_wgrad_scratch_bytes(600)
    _refused(L, L.rald_op_pe_wgrad(d, d, d, 600, d, d, d, need - 4, None), "scratch too small")
    _refused(L, L.rald_op_pe_wgrad(d, d, d, 600, d, d, d + 4, need, None), "scratch", "16-byte aligned")
