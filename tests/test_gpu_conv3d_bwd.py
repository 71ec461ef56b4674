"""The convolution backward of the radar encoder per element against float64: the Conv3d weight gradient (rald_amd/csrc/gemm_tn.hip:
conv_wgrad_line_kernel<1> / <2>, the CONV form of gemm_tn_kernel narrow and wide, each in its atomic and in its slab + tn_reduce_kernel form,
each with shift and with division decode), the plain row-contracting GEMM of every Linear's dW, and the data gradients conv_dgrad /
down_dgrad of rald_amd/train_encoder.py.  Conventions and helpers of tests/test_gpu_train_ops.py and tests/test_gpu_radar_encoder_ops.py:
the reference is a plain float64 statement on the CPU from exactly the bf16 values the kernel read (for the weight gradient the header's
own formula: gather x[v * stride - pad + tap], zero outside, contract with dy); B >= 3 where the shape allows, distinct values per
sample; dy and x each sit between NaN planes of a larger buffer; dW and dbias are accumulated into, so they start from small non-zero
integers, lie in one allocation (dbias right behind dW) and carry a SENT guard tail; the workspace is pre-filled with NaN, so a slab read
before it is written poisons the result.

Every weight-gradient case first asks rald_op_conv3d_wgrad_route (the plan function of the launch itself) for its kernel, its ranges and
the steps / rows of one range, so a moved threshold fails the test instead of silently re-routing it.

Exact-integer data is the main instrument: x in [-3, 3], dy in [-2, 2], prefill in [-5, 5].  Every partial sum is an integer below
6 M + 5 < 2^24 (asserted per case), so the fp32 dW and dbias must equal the float64 reference BIT FOR BIT in every summation order: in the
atomic form (workspace = null), in the slab form, and the two against each other.  Random data (unit-variance bf16 dy and x) then bounds
the fp32 accumulation per element:
  |got - ref| <= k * 2^-24 * (|prefill| + sum |dy x|)          (dbias / colsum: sum |dy|)
with k at most 2.5 times the worst value measured on an MI355X (docstrings).

The route-table, reference and argument-check tests run on the CPU: they make no HIP call."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_radar_encoder_ops import _embed, _pack  # noqa: F401
from test_gpu_train_ops import DUMMY, SENT, L_cpu, _bits, _g, _guard_ok, _guarded, _le, _ratio, _refused  # noqa: F401

gpu = pytest.mark.gpu
NAN = float("nan")


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _same_bits(got, want64, what):
    """got (device, fp32 or bf16) equals the float64 reference rounded once to got's dtype, bit for bit"""
    want = want64.float().to(got.dtype).cuda().reshape(got.shape)
    bad = _bits(got.contiguous()) != _bits(want.contiguous())
    nbad = int(bad.sum())
    print(f"ratio {what}: {nbad} of {bad.numel()} elements differ (bound 0)")
    if nbad:
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError((what, nbad, "first at flat index", i, float(got.reshape(-1)[i]), float(want.reshape(-1)[i])))


def _rows_between_nan(t16, ld=None, extra=64):
    """bf16 [M, N] on the CPU -> (device buffer [extra + M + extra, ld] that is NaN wherever the matrix is not, the [M, N] view inside it)"""
    M, N = t16.shape
    buf = torch.full((M + 2 * extra, ld or N), NAN, dtype=torch.bfloat16)
    buf[extra:extra + M, :N] = t16
    d = buf.cuda()
    return d, d[extra:extra + M, :N]


def _patches(x, stride, pad):
    """the header's formula: 27 gathers xs[tap][v][ci] = x[b][od * s - p + kd][oh * s - p + kh][ow * s - p + kw][ci], zero outside the volume;
    x float64 [B, ID, IH, IW, Cin], output dims ID / s etc. -> list of 27 [M, Cin] matrices, tap = kd * 9 + kh * 3 + kw"""
    B, ID, IH, IW, Cin = x.shape
    O = [ID // stride, IH // stride, IW // stride]
    far = [max(0, (o - 1) * stride - pad + 2 - (i - 1)) for o, i in zip(O, (ID, IH, IW))]
    xp = F.pad(x, (0, 0, pad, far[2], pad, far[1], pad, far[0]))
    sl = lambda k, o: slice(k, k + (o - 1) * stride + 1, stride)
    return [xp[:, sl(kd, O[0]), sl(kh, O[1]), sl(kw, O[2])].reshape(-1, Cin) for kd in range(3) for kh in range(3) for kw in range(3)]


def _wgrad64(x, dy, stride, pad):
    """float64 dW [Cout, Cin, 27] = sum over output voxels of dy[v][co] x[v * stride - pad + tap][ci]"""
    return torch.stack([dy.t() @ p for p in _patches(x, stride, pad)], -1)


@functools.lru_cache(maxsize=2)
def _wgrad_data(shape, stride, pad, kind):
    """One data set per case, the float64 reference computed once.  kind 'int': x in [-3, 3], dy in [-2, 2], prefill in [-5, 5]; 'rnd':
    unit-variance bf16 x and dy, unit-variance fp32 prefill.  ref = prefill + gradient (float64); terms (rnd only) = |prefill| + sum |dy x|."""
    B, ID, IH, IW, Cin, Cout = shape
    g = _g(2000 + 7 * ID + 13 * IW + 3 * IH + Cin + 5 * Cout + stride + 11 * pad + len(kind))
    M = B * (ID // stride) * (IH // stride) * (IW // stride)
    if kind == "int":
        x = torch.randint(-3, 4, (B, ID, IH, IW, Cin), generator=g).bfloat16()
        dy = torch.randint(-2, 3, (M, Cout), generator=g).bfloat16()
        W0 = torch.randint(-5, 6, (Cout, Cin, 27), generator=g).float()
        b0 = torch.randint(-5, 6, (Cout,), generator=g).float()
        W0[W0 == 0] = 1.0                                                              # accumulated into: every start value non-zero
        b0[b0 == 0] = -1.0
        assert 6 * M + 5 < 2 ** 24
    else:
        x = torch.randn(B, ID, IH, IW, Cin, generator=g).bfloat16()
        dy = torch.randn(M, Cout, generator=g).bfloat16()
        W0 = torch.randn(Cout, Cin, 27, generator=g)
        b0 = torch.randn(Cout, generator=g)
    assert all(not torch.equal(x[0], x[s]) for s in range(1, B))                        # distinct values per sample
    x64, dy64 = x.double(), dy.double()
    d = dict(x16=x, dy16=dy, W0=W0, b0=b0, M=M, refW=W0.double() + _wgrad64(x64, dy64, stride, pad), refb=b0.double() + dy64.sum(0))
    if kind == "rnd":
        d["termsW"] = W0.double().abs() + _wgrad64(x64.abs(), dy64.abs(), stride, pad)
        d["termsb"] = b0.double().abs() + dy64.abs().sum(0)
    return d


def _wgrad_upload(d):
    keepx, x = _embed(d["x16"])
    keepy, dy = _rows_between_nan(d["dy16"])
    return dict(keep=(keepx, keepy), x=x, dy=dy, W0=d["W0"].cuda().reshape(-1), b0=d["b0"].cuda())


def _wgrad_run(dev, shape, stride, pad, slab, with_bias):
    """One launch of rald_op_conv3d_wgrad.  dW [Cout * Cin * 27] and dbias [Cout] lie back to back in one buffer that ends in 64 sentinels;
    slab: through a NaN-filled workspace of exactly _workspace_bytes, else workspace = null (atomics).  Returns (dW, the Cout floats behind it)."""
    from rald_amd._lib import check, lib
    from test_gpu_train_ops import _st
    L = lib()
    B, ID, IH, IW, Cin, Cout = shape
    n = Cout * Cin * 27
    buf = _guarded(n + Cout, 64)
    buf[:n] = dev["W0"]
    buf[n:n + Cout] = dev["b0"]
    ws, nbytes = None, 0
    if slab:
        nbytes = L.rald_op_conv3d_wgrad_workspace_bytes(B, ID, IH, IW, Cin, Cout, stride, pad)
        assert nbytes > 0 and nbytes % 4 == 0, (shape, "no slab form for this shape")
        ws = torch.full((nbytes // 4,), NAN, device="cuda")
    check(L.rald_op_conv3d_wgrad(dev["dy"].data_ptr(), dev["x"].data_ptr(), buf.data_ptr(), buf[n:].data_ptr() if with_bias else None, B, ID, IH, IW,
                                 Cin, Cout, stride, pad, None if ws is None else ws.data_ptr(), nbytes, _st()))
    torch.cuda.synchronize()
    assert _guard_ok(buf, n + Cout), (shape, slab, with_bias, "guard behind dW / dbias")
    return buf[:n].view(Cout, Cin, 27), buf[n:n + Cout]


def _wgrad_route(shape, stride, pad):
    from rald_amd import _handles as H
    return H.op_conv3d_wgrad_route(*shape, stride, pad)


def _has_slab(shape, stride, pad):
    from rald_amd._lib import lib
    return lib().rald_op_conv3d_wgrad_workspace_bytes(*shape, stride, pad) > 0


def _exact_wgrad(shape, stride, pad, route):
    """atomic and (where the shape has one) slab form, each with and without dbias, on exact-integer data: 0 elements differ from float64,
    and every run equals every other bit for bit; with dbias = null the floats behind dW keep their prefill."""
    assert _wgrad_route(shape, stride, pad) == route, (shape, stride, pad, _wgrad_route(shape, stride, pad))
    d = _wgrad_data(shape, stride, pad, "int")
    assert 6 * d["M"] + 5 < 2 ** 24 and float(d["refW"].abs().max()) < 2 ** 24
    dev = _wgrad_upload(d)
    first = None
    for slab in (False, True) if _has_slab(shape, stride, pad) else (False,):
        for with_bias in (True, False):
            what = f"wgrad {route[0]} {shape} s{stride} p{pad} {'slab' if slab else 'atomic'}{'' if with_bias else ' no dbias'}"
            dW, db = _wgrad_run(dev, shape, stride, pad, slab, with_bias)
            _same_bits(dW, d["refW"], what + " dW")
            _same_bits(db, d["refb"] if with_bias else d["b0"].double(), what + " dbias")
            if first is None:
                first = dW
            assert torch.equal(_bits(first), _bits(dW)), what


# ---- the plan function (CPU) ------------------------------------------------------------------------------------------------------------
# (shape (B, ID, IH, IW, Cin, Cout), stride, pad, (kernel, ranges that do work, 64-voxel steps | rows per range)), as the library answers.
# Line kernel, stride 1 / pad 1: W = 4 with 16 lines per step, shift decode, 4 ranges of 1 step and 4 idle ranges | division decode (D = 3),
# 9 steps as 4 ranges of 2 and one of 1 | 4 parameter blocks, 20 steps as 6 ranges of 3 and one of 2, one idle range: the three-stage pipeline
# at its first full turn | W = 64: one line per step, 66-row input line, 63 steps as 7 ranges of 8 and one of 7 | Cin != Cout, 2 blocks |
# 23 ranges: a second slot round per XCD (10 240 voxels, the largest float64 reference of the file).
LINE1 = [((2, 4, 8, 4, 64, 64), 1, 1, ("line", 4, 1)), ((3, 3, 8, 8, 64, 64), 1, 1, ("line", 5, 2)), ((2, 5, 4, 32, 128, 128), 1, 1, ("line", 7, 3)),
         ((3, 3, 7, 64, 64, 64), 1, 1, ("line", 8, 8)), ((3, 6, 12, 16, 128, 64), 1, 1, ("line", 8, 7)), ((4, 20, 16, 8, 64, 64), 1, 1, ("line", 23, 7))]
# Line kernel, stride 2 / pad 0, even dims: OW = 8, 6 ranges of 1 step | OW = 16, division decode (OD = 3), 4 blocks | OW = 64: the 129-row line,
# input row 2 W is the only row out of range | 5 steps per range on the two-stage pipeline.
LINE2 = [((3, 8, 8, 16, 64, 64), 2, 0, ("line", 6, 1)), ((2, 6, 12, 32, 128, 128), 2, 0, ("line", 5, 2)), ((4, 2, 8, 128, 64, 64), 2, 0, ("line", 8, 2)),
         ((4, 16, 20, 16, 64, 64), 2, 0, ("line", 8, 5))]
# Generic CONV kernel: narrow, N2 = 216 no multiple of 128, M = 180 with a tail of 52 rows, N1 = 8 (clamped column re-reads) | the encoder's conv_out
# gradient: narrow, shift decode, 54 n2 tiles | W = 6 keeps 64 -> 64 off the line kernel: narrow, 2 ranges, tail 176 = 2 full steps + 48 (the wave
# row that owns the second 32-row sub-step is partly masked) | stride 2 / pad 0 on odd dims: M = 54 < 64, iw = IW the only padded tap | wide:
# Cin = 24 (taps change inside a 128-column tile), N1 = 136 (a second n1 tile of 8 live columns), 4 ranges, tail 177 | M = 2 500: 10 ranges, a second
# slot round | the 64-voxel level, one step | stride 2, M = 24 | pad 0 and pad 2 (the entry accepts any pad >= 0).
GENERIC = [((3, 5, 3, 4, 8, 8), 1, 1, ("generic", 1, 192)), ((2, 8, 4, 2, 256, 16), 1, 1, ("generic", 1, 128)), ((3, 4, 6, 6, 64, 64), 1, 1, ("generic", 2, 256)),
           ((3, 5, 7, 6, 64, 64), 2, 0, ("generic", 1, 64)), ((3, 7, 5, 9, 24, 136), 1, 1, ("generic", 4, 256)), ((5, 10, 10, 5, 8, 136), 1, 1, ("generic", 10, 256)),
           ((2, 4, 4, 2, 128, 256), 1, 1, ("generic", 1, 64)), ((3, 4, 4, 4, 128, 128), 2, 0, ("generic", 1, 64)), ((3, 4, 4, 8, 16, 72), 1, 0, ("generic", 2, 192)),
           ((3, 4, 4, 8, 16, 72), 1, 2, ("generic", 2, 192))]
# The encoder's weight gradients at R, A, E = 128, 64, 32 and B = 4, in encoder order: (layer, D, H, W, Cin, Cout, stride, plan).  Every stride-1
# level with W in {4, ..., 32} and channel counts multiples of 64 is line, the W = 2 level is generic and the 16-output conv_out narrow (no workspace).
PRODUCT_WGRAD = [
    ("down.0 res", 128, 64, 32, 64, 64, 1, ("line", 56, 293)), ("down.0.downsample", 128, 64, 32, 64, 64, 2, ("line", 56, 37)),
    ("down.1 res", 64, 32, 16, 64, 64, 1, ("line", 56, 37)), ("down.1.downsample", 64, 32, 16, 64, 64, 2, ("line", 32, 8)),
    ("down.2.block.0.conv1", 32, 16, 8, 64, 128, 1, ("line", 24, 11)), ("down.2 res", 32, 16, 8, 128, 128, 1, ("line", 24, 11)),
    ("down.2.downsample", 32, 16, 8, 128, 128, 2, ("line", 8, 4)), ("down.3 res", 16, 8, 4, 128, 128, 1, ("line", 8, 4)),
    ("down.3.downsample", 16, 8, 4, 128, 128, 2, ("generic", 1, 256)), ("down.4.block.0.conv1", 8, 4, 2, 128, 256, 1, ("generic", 1, 256)),
    ("down.4 / mid res", 8, 4, 2, 256, 256, 1, ("generic", 1, 256)), ("conv_out", 8, 4, 2, 256, 16, 1, ("generic", 1, 256)),
]
# Plans only (no GPU case): shapes that sit on the thresholds the small test shapes stay clear of.  Slab form of the generic kernel: 32 tiles of
# 128 x 128 take one range per XCD (8), 28 tiles take round_up(256 / 28, 8) = 16.  Line ranges at the training batch B = 8: 4 parameter blocks fill
# 1 440 of 1 536 slots with 40 ranges (0.94 against 0.84 with 24: past the 0.05 margin; 56 would add under 0.05), 2 blocks take 56 (52 do work).
PLAN_ONLY = [((4, 16, 16, 6, 72, 256), 1, 1, ("generic", 8, 768)), ((4, 16, 16, 6, 64, 256), 1, 1, ("generic", 16, 384)),
             ((8, 32, 16, 8, 128, 128), 1, 1, ("line", 40, 13)), ((8, 32, 16, 8, 64, 128), 1, 1, ("line", 52, 10)), ((8, 128, 64, 32, 64, 64), 1, 1, ("line", 56, 586))]


def test_conv3d_wgrad_route_table_of_the_test_shapes_and_of_the_product():
    """rald_op_conv3d_wgrad_route makes no HIP call: its answers for every weight-gradient shape of this file and for the encoder's own
    convolutions, written out (kernel, ranges that do work, steps or rows per range); the workspace exists exactly for the line kernel and
    for Cout > 64; refused shapes return -1 and name the entry."""
    from rald_amd._lib import lib
    L = lib()
    for shape, stride, pad, route in LINE1 + LINE2 + GENERIC + PLAN_ONLY:
        assert _wgrad_route(shape, stride, pad) == route, (shape, stride, pad, _wgrad_route(shape, stride, pad))
        assert _has_slab(shape, stride, pad) == (route[0] == "line" or shape[5] > 64), shape
    for name, D, Hh, W, Cin, Cout, stride, route in PRODUCT_WGRAD:
        shape, pad = (4, D, Hh, W, Cin, Cout), 1 if stride == 1 else 0
        assert _wgrad_route(shape, stride, pad) == route, (name, _wgrad_route(shape, stride, pad))
        if stride == 1 and 4 <= W <= 32:
            assert route[0] == "line", name
        if W == 2:
            assert route[0] == "generic", name
        assert _has_slab(shape, stride, pad) == (Cout > 64 or route[0] == "line"), name
    # the conditions of the line kernel, one at a time: pad, odd dims under stride 2, channel counts, width, whole 64-voxel steps
    for shape, stride, pad in (((3, 3, 8, 8, 64, 64), 1, 0), ((3, 3, 8, 8, 64, 64), 1, 2), ((3, 8, 7, 16, 64, 64), 2, 0), ((3, 8, 8, 16, 64, 64), 2, 1),
                               ((3, 3, 8, 8, 32, 64), 1, 1), ((3, 3, 8, 8, 64, 96), 1, 1), ((3, 4, 8, 2, 64, 64), 1, 1), ((2, 2, 8, 128, 64, 64), 1, 1),
                               ((3, 3, 8, 6, 64, 64), 1, 1), ((3, 3, 5, 8, 64, 64), 1, 1)):
        assert _wgrad_route(shape, stride, pad)[0] == "generic", (shape, stride, pad)
    for bad in ((4, 8, 8, 8, 12, 64, 1, 1), (4, 8, 8, 8, 64, 12, 1, 1), (4, 8, 8, 8, 64, 64, 3, 1), (0, 8, 8, 8, 64, 64, 1, 1), (4, 8, 8, 8, 64, 64, 1, -1),
                (4, 1, 8, 8, 64, 64, 2, 0), (4, 8, 8, 8, 0, 64, 1, 1)):
        assert L.rald_op_conv3d_wgrad_route(*bad, None, None) == -1 and b"rald_op_conv3d_wgrad_route" in L.rald_last_error(), bad


def test_the_gather_formula_of_the_reference_equals_float64_autograd():
    """The reference of this file (the header's formula) against float64 autograd of the forward as the model writes it, where the two are
    the same statement: F.conv3d(padding = 1) for stride 1 / pad 1, and Downsample's F.pad(0, 1) + stride 2 on even and on odd dims.
    Integers: equal exactly."""
    g = _g(5)
    for (B, D, Hh, W, Cin, Cout), stride in (((2, 3, 4, 5, 3, 4), 1), ((2, 4, 6, 2, 3, 4), 2), ((2, 5, 7, 6, 3, 4), 2)):
        x = torch.randint(-3, 4, (B, D, Hh, W, Cin), generator=g).double()
        Wt = torch.zeros(Cout, Cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
        xn = x.permute(0, 4, 1, 2, 3)
        y = F.conv3d(xn, Wt, padding=1) if stride == 1 else F.conv3d(F.pad(xn, (0, 1, 0, 1, 0, 1)), Wt, stride=2)
        assert tuple(y.shape[2:]) == (D // stride, Hh // stride, W // stride)
        dy = torch.randint(-2, 3, y.shape, generator=g).double()
        y.backward(dy)
        got = _wgrad64(x, dy.permute(0, 2, 3, 4, 1).reshape(-1, Cout), stride, 1 if stride == 1 else 0)
        assert torch.equal(got, Wt.grad.reshape(Cout, Cin, 27)), stride


# ---- weight gradient, exact-integer data: every kernel form bit for bit ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,stride,pad,route", LINE1)
def test_conv3d_wgrad_line_kernel_stride_1_exact_on_integer_data(shape, stride, pad, route):
    """conv_wgrad_line_kernel<1> (shapes: LINE1 above) in its atomic and its slab + tn_reduce_kernel form, with and without dbias: every tap at
    every face, the zero voxel on either side of a line, the ranges' seams and the dbias workgroup are all in the comparison.  0 elements differ."""
    _exact_wgrad(shape, stride, pad, route)


@gpu
@pytest.mark.parametrize("shape,stride,pad,route", LINE2)
def test_conv3d_wgrad_line_kernel_stride_2_exact_on_integer_data(shape, stride, pad, route):
    """conv_wgrad_line_kernel<2> (shapes: LINE2 above; the reference is also float64 autograd of Downsample's F.pad(0, 1) + stride 2), atomic and
    slab form, with and without dbias.  0 elements differ."""
    _exact_wgrad(shape, stride, pad, route)


@gpu
@pytest.mark.parametrize("shape,stride,pad,route", GENERIC)
def test_conv3d_wgrad_generic_kernel_exact_on_integer_data(shape, stride, pad, route):
    """gemm_tn_kernel<CONV> narrow (Cout <= 64: atomic form only) and wide (Cout > 64: atomic and slab form), shapes GENERIC above, with and
    without dbias.  0 elements differ."""
    _exact_wgrad(shape, stride, pad, route)


# ---- plain gemm_tn, exact-integer data --------------------------------------------------------------------------------------------------
def _tn_run(A, Bm, C0, cs0, M, N1, N2, ldc, slab, with_cs):
    """One launch of rald_op_gemm_tn on views with leading dimensions above the widths.  C is a window of a sentinel-filled [N1 + 1, ldc] buffer,
    colsum ends in 64 sentinels; slab: a NaN-filled workspace of exactly _workspace_bytes.  Returns (C window, colsum)."""
    from rald_amd._lib import check, lib
    from test_gpu_train_ops import _st
    L = lib()
    Cb = torch.full((N1 + 1, ldc), SENT, device="cuda")
    Cb[:N1, :N2] = C0
    cs = _guarded(N1, 64)
    cs[:N1] = cs0
    ws, nbytes = None, 0
    if slab:
        nbytes = L.rald_op_gemm_tn_workspace_bytes(M, N1, N2)
        assert nbytes > 0 and nbytes % 4 == 0
        ws = torch.full((nbytes // 4,), NAN, device="cuda")
    check(L.rald_op_gemm_tn(A.data_ptr(), A.stride(0), Bm.data_ptr(), Bm.stride(0), Cb.data_ptr(), ldc, cs.data_ptr() if with_cs else None, M, N1, N2,
                            None if ws is None else ws.data_ptr(), nbytes, _st()))
    torch.cuda.synchronize()
    assert _guard_ok(cs, N1) and bool((Cb[:N1, N2:] == SENT).all()) and bool((Cb[N1:] == SENT).all()), (M, N1, N2, slab, "guards")
    return Cb[:N1, :N2], cs[:N1]


def _tn_data(M, N1, N2, kind):
    g = _g(3000 + M + 3 * N1 + 7 * N2 + len(kind))
    if kind == "int":
        A, Bm = torch.randint(-2, 3, (M, N1), generator=g).bfloat16(), torch.randint(-3, 4, (M, N2), generator=g).bfloat16()
        C0, cs0 = torch.randint(1, 6, (N1, N2), generator=g).float(), -torch.randint(1, 6, (N1,), generator=g).float()
        assert 6 * M + 5 < 2 ** 24
    else:
        A, Bm = torch.randn(M, N1, generator=g).bfloat16(), torch.randn(M, N2, generator=g).bfloat16()
        C0, cs0 = torch.randn(N1, N2, generator=g), torch.randn(N1, generator=g)
    return A, Bm, C0, cs0


@gpu
@pytest.mark.parametrize("M,N1,N2", [(1, 8, 8), (63, 64, 120), (65, 72, 136), (300, 136, 8), (2500, 136, 264), (70, 64, 1024)])
def test_gemm_tn_plain_form_exact_on_integer_data(M, N1, N2):
    """gemm_tn_kernel<false> (every Linear's dW and bias gradient): one row; one row short of a step, narrow, N2 no multiple of 128; one row past
    a step with second tiles of 8 live columns along both n1 and n2; N2 = 8 (clamped column re-reads of B) with a tail of 44 rows; 10 row ranges
    x 6 tiles; narrow with 8 n2 tiles.  lda = N1 + 8, ldb = N2 + 16 (the gaps hold NaN), ldc = N2 + 8 (the gap holds sentinels), A in [-2, 2],
    B in [-3, 3], prefill in [1, 5] / [-5, -1].  Atomic form, and the slab form wherever the shape has one (N1 > 64), each with and without
    colsum: 0 elements differ from float64, all runs bit-identical, and colsum = null leaves the buffer alone."""
    from rald_amd._lib import lib
    A, Bm, C0, cs0 = _tn_data(M, N1, N2, "int")
    keepa, Ad = _rows_between_nan(A, N1 + 8)
    keepb, Bd = _rows_between_nan(Bm, N2 + 16)
    refC, refcs = C0.double() + A.double().t() @ Bm.double(), cs0.double() + A.double().sum(0)
    has_slab = lib().rald_op_gemm_tn_workspace_bytes(M, N1, N2) > 0
    assert has_slab == (N1 > 64)
    first = None
    for slab in (False, True) if has_slab else (False,):
        for with_cs in (True, False):
            what = f"gemm_tn {M}x{N1}x{N2} {'slab' if slab else 'atomic'}{'' if with_cs else ' no colsum'}"
            Cg, cs = _tn_run(Ad, Bd, C0.cuda(), cs0.cuda(), M, N1, N2, N2 + 8, slab, with_cs)
            _same_bits(Cg, refC, what + " C")
            _same_bits(cs, refcs if with_cs else cs0.double(), what + " colsum")
            if first is None:
                first = Cg.clone()
            assert torch.equal(_bits(first), _bits(Cg.contiguous())), what


# ---- data gradients, exact-integer data -------------------------------------------------------------------------------------------------
def _dgrad_data(dims, Cin, Cout, seed):
    """dy in [-3, 3] [B, D, H, W, Cout] (bf16-exact), W in [-2, 2] [Cout, Cin, 3, 3, 3]; the reference is float64 autograd of F.conv3d(padding = 1)"""
    B, D, Hh, W = dims
    g = _g(seed)
    dy = torch.randint(-3, 4, (B, D, Hh, W, Cout), generator=g).float()
    Wt = torch.randint(-2, 3, (Cout, Cin, 3, 3, 3), generator=g).float()
    assert all(not torch.equal(dy[0], dy[s]) for s in range(1, B)) and 27 * Cout * 3 * 2 < 2 ** 24
    x = torch.zeros(B, Cin, D, Hh, W, dtype=torch.float64, requires_grad=True)
    F.conv3d(x, Wt.double(), padding=1).backward(dy.double().permute(0, 4, 1, 2, 3))
    return dy, Wt, x.grad.permute(0, 2, 3, 4, 1).contiguous()


@gpu
@pytest.mark.parametrize("dims,Cin,Cout,engine", [((2, 3, 8, 8), 64, 128, "line"), ((3, 5, 3, 4), 128, 64, "igemm")])
def test_conv_dgrad_bf16_dy_read_as_it_lies_exact_on_integer_data(dims, Cin, Cout, engine):
    """train_encoder.conv_dgrad = rald_op_conv_pack_weights(dgrad = 1) + the forward Conv3d with the channel roles swapped, Cout a multiple of
    64 and dy already bf16 (read in place, between two NaN planes): the line engine (384 voxels, W = 8) and the igemm engine (180 voxels,
    W = 4, a tail tile).  Every sum is an integer below 27 * Cout * 6 < 2^24: the fp32 dx equals float64 autograd of F.conv3d bit for bit, and
    the out_bf16 form equals its bf16 rounding."""
    from rald_amd import _handles as H
    from rald_amd import train_encoder as TE
    B, D, Hh, W = dims
    assert H.op_conv3d_route(B, D, Hh, W, Cout, Cin, 1, 1, 0) == (engine, 1)
    dy, Wt, ref = _dgrad_data(dims, Cin, Cout, 60 + Cin)
    keep, dyd = _embed(dy.bfloat16())
    dyd = dyd.view(B, D, Hh, W, Cout)
    assert dyd.is_contiguous()
    Wd = Wt.cuda()
    for out_bf16 in (False, True):
        dx = TE.conv_dgrad(dyd, Wd, out_bf16=out_bf16)
        torch.cuda.synchronize()
        assert dx.dtype == (torch.bfloat16 if out_bf16 else torch.float32) and dx.shape == (B, D, Hh, W, Cin)
        _same_bits(dx, ref, f"conv_dgrad {engine} {dims} {Cout}->{Cin} {'bf16' if out_bf16 else 'fp32'}")


@gpu
def test_conv_dgrad_of_16_output_channels_padded_to_64_ignores_the_pad_lanes():
    """conv_dgrad of the encoder's conv_out (Cout = 16, Cin = 256) at (2, 3, 8, 8): fp32 dy goes through pad_channels to 64 lanes and the weights
    are packed with pad_to = 64.  fp32 and out_bf16 equal float64 autograd bit for bit; and the same composition by hand with the value 3 in the
    48 pad lanes of the packed weights (the pad lanes of dy are zero) gives the same bits: nothing of a pad lane reaches the result."""
    from rald_amd import _handles as H
    from rald_amd import train_encoder as TE
    from rald_amd import train_ops as TO
    dims, Cin, Cout = (2, 3, 8, 8), 256, 16
    B, D, Hh, W = dims
    assert H.op_conv3d_route(B, D, Hh, W, 64, Cin, 1, 1, 0) == ("line", 1)
    dy, Wt, ref = _dgrad_data(dims, Cin, Cout, 77)
    dyd, Wd = dy.cuda(), Wt.cuda()
    for out_bf16 in (False, True):
        dx = TE.conv_dgrad(dyd, Wd, out_bf16=out_bf16)
        torch.cuda.synchronize()
        _same_bits(dx, ref, f"conv_dgrad padded 16->64 {'bf16' if out_bf16 else 'fp32'}")
        wp = TE.pack_conv(Wd, dgrad=True, pad_to=64)
        assert wp.shape == (Cin, 27, 64) and bool((wp[:, :, Cout:] == 0).all())
        wp[:, :, Cout:] = 3.0
        dy16 = TO.pad_channels(dyd, 64)
        assert bool((dy16[..., Cout:] == 0).all())
        by_hand = TE.conv3d(dy16, wp, torch.zeros(Cin, device="cuda"), None, 1, 1, out_bf16=out_bf16)
        torch.cuda.synchronize()
        assert torch.equal(_bits(by_hand), _bits(dx)), out_bf16


@gpu
@pytest.mark.parametrize("odims,Cc", [((3, 2, 3, 5), 64), ((2, 4, 4, 8), 128)])
def test_down_dgrad_stride_1_pad_2_on_the_igemm_engine_exact_on_integer_data(odims, Cc):
    """train_encoder.down_dgrad = zero_insert2 + the forward Conv3d at stride 1, PAD 2 (the igemm engine's only pad-2 caller), against float64
    autograd of Downsample.forward, F.conv3d(F.pad(x, (0, 1, 0, 1, 0, 1)), W, stride = 2).  Output dims (3, 2, 3, 5) with C = 64 (480 voxels of the
    zero-inserted grid, W = 10) and (2, 4, 4, 8) with C = 128, whose zero-inserted input has W = 16 and M = 1024: only pad != 1 keeps it off the
    line engine.  dy and W in [-2, 2]: every sum is an integer below 27 * Cout * 2 * 2 < 2^24, the fp32 dx equals the reference bit for bit."""
    from rald_amd import _handles as H
    from rald_amd import train_encoder as TE
    B, OD, OH, OW = odims
    assert H.op_conv3d_route(B, 2 * OD, 2 * OH, 2 * OW, Cc, Cc, 1, 2, 0) == ("igemm", 1)
    if Cc == 128:
        assert (B * 8 * OD * OH * OW) % 128 == 0 and H.op_conv3d_route(B, 2 * OD, 2 * OH, 2 * OW, Cc, Cc, 1, 1, 0) == ("line", 1)
    assert 27 * Cc * 2 * 2 < 2 ** 24
    g = _g(80 + Cc)
    dy = torch.randint(-2, 3, (B, OD, OH, OW, Cc), generator=g).float()
    Wt = torch.randint(-2, 3, (Cc, Cc, 3, 3, 3), generator=g).float()
    assert all(not torch.equal(dy[0], dy[s]) for s in range(1, B))
    x = torch.zeros(B, Cc, 2 * OD, 2 * OH, 2 * OW, dtype=torch.float64, requires_grad=True)
    F.conv3d(F.pad(x, (0, 1, 0, 1, 0, 1)), Wt.double(), stride=2).backward(dy.double().permute(0, 4, 1, 2, 3))
    ref = x.grad.permute(0, 2, 3, 4, 1).contiguous()
    buf = torch.full((B * OD + 2, OH, OW, Cc), NAN)                                       # fp32 dy between two NaN planes
    buf[1:-1] = dy.reshape(B * OD, OH, OW, Cc)
    keep = buf.cuda()
    dx = TE.down_dgrad(keep[1:-1].view(B, OD, OH, OW, Cc), Wt.cuda())
    torch.cuda.synchronize()
    assert dx.dtype == torch.float32 and dx.shape == (B, 2 * OD, 2 * OH, 2 * OW, Cc)
    _same_bits(dx, ref, f"down_dgrad {odims} C={Cc}")


# ---- random data: the fp32 accumulation per element -------------------------------------------------------------------------------------
# measured k on an MI355X (dW, dbias | C, colsum), worst of the forms run -> bounds at most 2.5 times that:
#   line1 0.862, 0.0995   line2 0.826, 0.163   wide 0.757, 0.124   narrow 1.06, 0.0783   plain 0.679, 0.175
# (the forward engines at K = 1 728 to 6 912 measured 1.4 to 2.2: here 384 to 945 voxels are contracted, and a column sum adds exact bf16 values)
BOUNDS_RND = {"line1": (2.1, 0.24), "line2": (2.0, 0.4), "wide": (1.85, 0.31), "narrow": (2.6, 0.19), "plain": (1.65, 0.43)}


@gpu
@pytest.mark.parametrize("name,shape,stride,pad,kernel", [
    ("line1", (3, 3, 8, 8, 64, 64), 1, 1, "line"), ("line2", (3, 8, 8, 16, 64, 64), 2, 0, "line"), ("wide", (3, 7, 5, 9, 24, 136), 1, 1, "generic"),
    ("narrow", (3, 4, 6, 6, 64, 64), 1, 1, "generic")])
def test_conv3d_wgrad_random_data_per_element(name, shape, stride, pad, kernel):
    """Unit-variance bf16 dy and x, unit-variance fp32 prefill, against float64 of the same values:
    |got - ref| <= k * 2^-24 * (|prefill| + sum |dy x|) per element of dW, and the same with sum |dy| for dbias.  The line kernel and the wide
    generic kernel run in their slab form (what the encoder runs) and in their atomic form, the narrow one in its atomic form; k is the worst.
    Measured k on an MI355X (dW / dbias): line stride 1 0.862 / 0.0995, line stride 2 0.826 / 0.163, wide 0.757 / 0.124, narrow 1.06 / 0.0783;
    bounds BOUNDS_RND = 2.1 / 0.24, 2.0 / 0.4, 1.85 / 0.31, 2.6 / 0.19."""
    assert _wgrad_route(shape, stride, pad)[0] == kernel
    d = _wgrad_data(shape, stride, pad, "rnd")
    dev = _wgrad_upload(d)
    kW = kb = 0.0
    for slab in (True, False) if _has_slab(shape, stride, pad) else (False,):
        dW, db = _wgrad_run(dev, shape, stride, pad, slab, True)
        rW, rb = _ratio(dW, d["refW"], d["termsW"]), _ratio(db, d["refb"], d["termsb"])
        print(f"ratio wgrad rnd {name} {'slab' if slab else 'atomic'}: dW {rW:.3g} dbias {rb:.3g}")
        kW, kb = max(kW, rW), max(kb, rb)
    _le(f"wgrad rnd {name} dW", kW, BOUNDS_RND[name][0])
    _le(f"wgrad rnd {name} dbias", kb, BOUNDS_RND[name][1])


@gpu
def test_gemm_tn_plain_form_random_data_per_element():
    """rald_op_gemm_tn at (M, N1, N2) = (300, 136, 8) on unit-variance bf16 operands with lda = 144, ldb = 24, slab and atomic form:
    |got - ref| <= k * 2^-24 * (|prefill| + sum |a b|), colsum with sum |a|.  Measured k on an MI355X (C / colsum): 0.679 / 0.175; bounds 1.65 / 0.43."""
    M, N1, N2 = 300, 136, 8
    A, Bm, C0, cs0 = _tn_data(M, N1, N2, "rnd")
    keepa, Ad = _rows_between_nan(A, N1 + 8)
    keepb, Bd = _rows_between_nan(Bm, N2 + 16)
    A64, B64 = A.double(), Bm.double()
    refC, refcs = C0.double() + A64.t() @ B64, cs0.double() + A64.sum(0)
    tC, tcs = C0.double().abs() + A64.abs().t() @ B64.abs(), cs0.double().abs() + A64.abs().sum(0)
    kC = kc = 0.0
    for slab in (True, False):
        Cg, cs = _tn_run(Ad, Bd, C0.cuda(), cs0.cuda(), M, N1, N2, N2 + 8, slab, True)
        rC, rc = _ratio(Cg, refC, tC), _ratio(cs, refcs, tcs)
        print(f"ratio gemm_tn rnd {'slab' if slab else 'atomic'}: C {rC:.3g} colsum {rc:.3g}")
        kC, kc = max(kC, rC), max(kc, rc)
    _le("gemm_tn rnd C", kC, BOUNDS_RND["plain"][0])
    _le("gemm_tn rnd colsum", kc, BOUNDS_RND["plain"][1])


# ---- argument checks (CPU: each fires before the entry's first HIP call) --------------------------------------------------------------
def test_wgrad_argument_checks_name_the_constraint(L_cpu):
    L, d = L_cpu, DUMMY
    shape = (2, 4, 8, 8, 64, 128)
    _refused(L, L.rald_op_conv3d_wgrad(d, d, d, None, 2, 4, 8, 8, 12, 64, 1, 1, None, 0, None), "channel counts", "multiples of 8")
    _refused(L, L.rald_op_conv3d_wgrad(d, d, d, None, 2, 4, 8, 8, 64, 20, 1, 1, None, 0, None), "channel counts", "multiples of 8")
    _refused(L, L.rald_op_conv3d_wgrad(d, d, d, None, *shape, 3, 1, None, 0, None), "stride 1 or 2")
    _refused(L, L.rald_op_conv3d_wgrad(d + 8, d, d, None, *shape, 1, 1, None, 0, None), "16-byte alignment")
    _refused(L, L.rald_op_conv3d_wgrad(d, d + 8, d, None, *shape, 1, 1, None, 0, None), "16-byte alignment")
    need = L.rald_op_conv3d_wgrad_workspace_bytes(*shape, 1, 1)
    assert need > 0
    _refused(L, L.rald_op_conv3d_wgrad(d, d, d, None, *shape, 1, 1, d, need - 4, None), "workspace smaller than", "_workspace_floats")
    _refused(L, L.rald_op_conv3d_wgrad(d, d, d, None, *shape, 1, 1, d + 4, need, None), "workspace")
    _refused(L, L.rald_op_gemm_tn(d, 64, d, 64, d, 64, None, 100, 72, 64, None, 0, None), "leading dimensions")
    _refused(L, L.rald_op_gemm_tn(d, 72, d, 56, d, 64, None, 100, 72, 64, None, 0, None), "leading dimensions")
    _refused(L, L.rald_op_gemm_tn(d, 72, d, 64, d, 56, None, 100, 72, 64, None, 0, None), "leading dimensions")
    need = L.rald_op_gemm_tn_workspace_bytes(100, 72, 64)
    assert need > 0
    _refused(L, L.rald_op_gemm_tn(d, 72, d, 64, d, 64, None, 100, 72, 64, d, need - 4, None), "workspace smaller than", "_workspace_floats")
