"""The radar encoder's kernels (rald_amd/csrc/conv3d.hip, rald_amd/csrc/radar.hip) per element against float64: the four implicit-GEMM Conv3d engines (igemm, line,
plane, persistent plane), the split-K route with its reduce pass, the GroupNorm partials of the convolution epilogue, gn_finish, the
GroupNorm forward, and the three small data-movement / tokeniser kernels.  Conventions of tests/test_gpu_train_ops.py (whose helpers
this file imports): the reference is a plain float64 statement on the CPU from exactly the values the kernel read; B >= 3 where the
engine's shape allows, distinct values per sample; outputs start as NaN with 64 sentinel elements behind them; the input sits between
two NaN planes of a larger buffer; every check prints its measured ratio.

Every convolution test first asks rald_op_conv3d_route (the library's one engine-choice function) that its shape runs on the engine
the test is named for, so a moved threshold fails the test instead of silently re-routing it.

Exact-integer data is the main instrument: inputs in [-3, 3], weights in [-2, 2], small integer bias and residual.  Every partial sum
is an integer below 27 * 256 * 6 + 10 < 2^24, so the fp32 result must equal the float64 reference BIT FOR BIT on every engine, in any
summation order, split-K included, and the bf16 output must equal torch's bf16 rounding of that exact value.  Random data
(unit-variance inputs, weights scaled by (27 Cin)^-1/2) then bounds the fp32 accumulation per element:
  |got - ref| <= k * 2^-24 * (|bias| + |resid| + sum |w x|)       (+ one bf16 ulp of the reference for out_bf16)
with k at most 2.5 times the worst value measured on an MI355X (docstrings).

The argument-check and route-table tests run on the CPU: they make no HIP call."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_train_ops import DUMMY, SENT, U, L_cpu, _bits, _f64, _g, _guard_ok, _guarded, _le, _ratio, _ratio16, _refused  # noqa: F401

gpu = pytest.mark.gpu


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _pack(W):
    """the parameter [Cout, Cin, 3, 3, 3] -> the kernels' packed bf16 [Cout][tap = kd*9 + kh*3 + kw][Cin]"""
    return W.permute(0, 2, 3, 4, 1).reshape(W.shape[0], 27, W.shape[1]).contiguous().bfloat16()


def _conv64(x, W, stride):
    """float64 Conv3d k3 of channels-last x [B, D, H, W, Cin]: stride 1 pad 1, or Downsample.forward's F.pad(0, 1) + k3 s2 p0"""
    xn = x.permute(0, 4, 1, 2, 3)
    y = F.conv3d(F.pad(xn, (0, 1, 0, 1, 0, 1)), W, stride=2) if stride == 2 else F.conv3d(xn, W, padding=1)
    return y.permute(0, 2, 3, 4, 1).contiguous()


def _embed(x16):
    """bf16 [B, D, H, W, C] on the CPU -> (device buffer with one NaN plane before and after, the view of the input inside it)"""
    B, D, H, W, Cc = x16.shape
    buf = torch.full((B * D + 2, H, W, Cc), float("nan"), dtype=torch.bfloat16)
    buf[1:-1] = x16.reshape(B * D, H, W, Cc)
    d = buf.cuda()
    return d, d[1:-1]


@functools.lru_cache(maxsize=2)
def _conv_data(shape, stride, kind):
    """One data set per (shape, stride, kind), the float64 reference computed once.  kind 'int': x in [-3, 3], w in [-2, 2]; 'tri': both in
    {-1, 0, 1} (the GroupNorm-partial tests); 'rnd': unit-variance x, w ~ (27 Cin)^-1/2, everything rounded to bf16 first.  Returns
    x16, wp (bf16), bias, resid [M, Cout] (f32), base = conv + bias [M, Cout] (f64), terms (f64, 'rnd' only), out dims."""
    B, D, H, W, Cin, Cout = shape
    g = _g(1000 + 7 * D + 13 * W + Cin + 3 * Cout + stride + len(kind))
    if kind == "rnd":
        x = torch.randn(B, D, H, W, Cin, generator=g).bfloat16()
        Wt = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (27 * Cin) ** -0.5).bfloat16()
        bias = torch.randn(Cout, generator=g)
    else:
        a, b = (3, 2) if kind == "int" else (1, 1)
        x = torch.randint(-a, a + 1, (B, D, H, W, Cin), generator=g).bfloat16()
        Wt = torch.randint(-b, b + 1, (Cout, Cin, 3, 3, 3), generator=g).bfloat16()
        bias = torch.randint(-5, 6, (Cout,), generator=g).float()
    assert all(not torch.equal(x[0], x[s]) for s in range(1, B))                     # distinct values per sample
    conv = _conv64(x.double(), Wt.double(), stride)
    OD, OH, OW = conv.shape[1:4]
    M = B * OD * OH * OW
    resid = torch.randn(M, Cout, generator=g) if kind == "rnd" else torch.randint(-5, 6, (M, Cout), generator=g).float()
    base = conv.reshape(M, Cout) + bias.double()
    terms = None
    if kind == "rnd":
        terms = _conv64(x.double().abs(), Wt.double().abs(), stride).reshape(M, Cout) + bias.double().abs()
    return dict(x16=x, wp=_pack(Wt), bias=bias, resid=resid, base=base, terms=terms, dims=(OD, OH, OW), M=M)


def _route(shape, stride, allow_split):
    from rald_amd import _handles as H
    B, D, Hh, W, Cin, Cout = shape
    return H.op_conv3d_route(B, D, Hh, W, Cin, Cout, stride, 1 if stride == 1 else 0, allow_split)


def _conv_run(d, shape, stride, dev, mode, allow_split=0, gn=False):
    """One launch of rald_op_conv3d_full on the uploaded data set; mode 'plain' (fp32 out, NaN-prefilled), 'inplace' (out holds the residual
    and is passed as resid too) or 'bf16'.  Returns (output [M, Cout] view, gn_part [M/128, 32, 2] or None); guards are asserted here."""
    from rald_amd import _handles as H
    B, D, Hh, W, Cin, Cout = shape
    M, n = d["M"], d["M"] * Cout
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    buf = _guarded(n, 64, dtype=dt)
    if mode == "inplace":
        buf[:n] = dev["resid"].reshape(-1)
    part = _guarded(M // 128 * 64, 64, dtype=torch.float64) if gn else None
    ws = None
    eng, splits = _route(shape, stride, allow_split)
    if eng == "igemm-split":
        ws = torch.full((splits * n,), float("nan"), device="cuda")      # a partial slab read before it is written poisons the result
    H.op_conv3d_full(dev["x"], dev["wp"], dev["bias"], B, D, Hh, W, Cin, Cout, out=None if mode == "bf16" else buf,
                     out_bf16=buf if mode == "bf16" else None, resid=buf if mode == "inplace" else None, gn_part=part, split_ws=ws,
                     allow_split=allow_split, stride=stride, pad=1 if stride == 1 else 0)
    torch.cuda.synchronize()
    assert _guard_ok(buf, n), (shape, mode, "output guard")
    if gn:
        assert _guard_ok(part, M // 128 * 64), (shape, mode, "gn_part guard")
    return buf[:n].view(M, Cout), (part[:M // 128 * 64].view(M // 128, 32, 2) if gn else None)


def _upload(d):
    keep, x = _embed(d["x16"])
    return dict(keep=keep, x=x, wp=d["wp"].cuda(), bias=d["bias"].cuda(), resid=d["resid"].cuda())


def _same_bits(got, want64, what):
    """got (device, fp32 or bf16) equals the float64 reference rounded once to got's dtype, bit for bit"""
    want = want64.float().to(got.dtype).cuda()
    bad = _bits(got.contiguous()) != _bits(want)
    nbad = int(bad.sum())
    print(f"ratio {what}: {nbad} of {bad.numel()} elements differ (bound 0)")
    if nbad:
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError((what, nbad, "first at flat index", i, float(got.reshape(-1)[i]), float(want.reshape(-1)[i])))


def _exact_conv(shape, stride, engine, allow_split=0):
    """plain, in place (resid == out) and out_bf16 on exact-integer data; returns the plain and in-place fp32 results (device)"""
    eng, splits = _route(shape, stride, allow_split)
    assert eng == engine, (shape, eng, splits)
    d = _conv_data(shape, stride, "int")
    assert float((d["base"].abs() + 5).max()) < 2 ** 24
    dev = _upload(d)
    outs = []
    for mode in ("plain", "inplace") + (() if engine == "igemm-split" else ("bf16",)):
        got, _ = _conv_run(d, shape, stride, dev, mode, allow_split)
        want = d["base"] + d["resid"].double() if mode == "inplace" else d["base"]
        _same_bits(got, want, f"conv {engine} {shape} s{stride} {mode}")
        outs.append(got)
    return d, dev, outs


# ---- the engine-choice function (CPU) ------------------------------------------------------------------------------------------------
IGEMM_SHAPES = [((3, 5, 3, 4, 64, 16), 1), ((3, 3, 3, 8, 64, 64), 1), ((3, 5, 3, 4, 128, 72), 1), ((3, 6, 4, 10, 64, 64), 2), ((3, 5, 6, 10, 64, 72), 2)]
LINE_SHAPES = [(2, 3, 8, 8, 64, 64), (2, 2, 6, 16, 64, 64), (3, 2, 2, 32, 128, 128), (2, 3, 8, 8, 256, 4), (2, 3, 8, 8, 128, 16), (3, 4, 16, 16, 64, 64)]
PLANE_SHAPES = [(4, 12, 96, 16, 64, 64), (4, 12, 48, 32, 64, 128)]
PPLANE_SHAPES = [(4, 64, 64, 32, 64, 64), (4, 128, 64, 16, 64, 64)]
SPLIT_SHAPES = [((3, 4, 4, 2, 64, 64), 1, 9), ((3, 8, 4, 2, 256, 256), 1, 16), ((3, 4, 4, 4, 256, 16), 1, 16), ((3, 8, 4, 2, 64, 256), 1, 9),
                ((3, 8, 8, 4, 128, 128), 2, 16)]
# GroupNorm partials from the epilogue: (shape, engine); Cout 64, 128 and 256 on the line engine, one igemm shape (its slot is blockIdx.y)
GN_SHAPES = [((3, 4, 16, 16, 64, 64), "line"), ((3, 2, 2, 32, 128, 128), "line"), ((3, 2, 8, 8, 256, 256), "line"), ((3, 8, 4, 4, 64, 64), "igemm"),
             ((4, 12, 48, 32, 64, 128), "plane"), ((4, 64, 64, 32, 64, 64), "pplane")]

# The encoder and decoder at R, A, E = 128, 64, 32, B = 4 (samples per pass), every convolution form in the order the two networks run them:
# (layer, D, H, W, Cin, Cout, stride, engine, splits).  Engines as conv3d.hip's comments and DESIGN.md section 4 state them: the full-resolution
# 64-channel level is persistent-plane, the half-resolution 64-channel level plane, the other stride-1 levels with W in {8, 16, 32} line (also
# Cin = 128 at W = 16 and the 4-output conv_out), the downsamples at and above 16 384 output voxels plain igemm, and every convolution of the
# 512- and 64-voxel levels split-K.
PRODUCT = [
    ("enc down.0 res", 128, 64, 32, 64, 64, 1, "pplane", 1), ("enc down.0.downsample", 128, 64, 32, 64, 64, 2, "igemm", 1),
    ("enc down.1 res", 64, 32, 16, 64, 64, 1, "plane", 1), ("enc down.1.downsample", 64, 32, 16, 64, 64, 2, "igemm", 1),
    ("enc down.2.block.0.conv1", 32, 16, 8, 64, 128, 1, "line", 1), ("enc down.2 res", 32, 16, 8, 128, 128, 1, "line", 1),
    ("enc down.2.downsample", 32, 16, 8, 128, 128, 2, "igemm-split", 8), ("enc down.3 res", 16, 8, 4, 128, 128, 1, "igemm-split", 8),
    ("enc down.3.downsample", 16, 8, 4, 128, 128, 2, "igemm-split", 16), ("enc down.4.block.0.conv1", 8, 4, 2, 128, 256, 1, "igemm-split", 16),
    ("enc down.4 / mid res", 8, 4, 2, 256, 256, 1, "igemm-split", 16), ("enc conv_out", 8, 4, 2, 256, 16, 1, "igemm-split", 16),
    ("dec conv_in", 8, 4, 2, 64, 256, 1, "igemm-split", 9), ("dec mid / up.4 res", 8, 4, 2, 256, 256, 1, "igemm-split", 16),
    ("dec up.4.upsample", 16, 8, 4, 256, 256, 1, "igemm-split", 4), ("dec up.3.block.0.conv1", 16, 8, 4, 256, 128, 1, "igemm-split", 8),
    ("dec up.3 res", 16, 8, 4, 128, 128, 1, "igemm-split", 8), ("dec up.3.upsample", 32, 16, 8, 128, 128, 1, "line", 1),
    ("dec up.2 res", 32, 16, 8, 128, 128, 1, "line", 1), ("dec up.2.upsample", 64, 32, 16, 128, 128, 1, "line", 1),
    ("dec up.1.block.0.conv1", 64, 32, 16, 128, 64, 1, "line", 1), ("dec up.1 res", 64, 32, 16, 64, 64, 1, "plane", 1),
    ("dec up.1.upsample / up.0 res", 128, 64, 32, 64, 64, 1, "pplane", 1), ("dec conv_out", 128, 64, 32, 64, 4, 1, "line", 1),
]


def test_conv3d_route_table_of_the_test_shapes_and_of_the_product():
    """rald_op_conv3d_route makes no HIP call: its answers for every shape of this file and for the encoder's and decoder's own convolutions,
    written out.  allow_split = 0 never splits; a line-engine shape never splits either way."""
    from rald_amd import _handles as H
    from rald_amd._lib import lib
    for shape, stride in IGEMM_SHAPES:
        assert _route(shape, stride, 0) == ("igemm", 1), shape
    for shapes, eng in ((LINE_SHAPES, "line"), (PLANE_SHAPES, "plane"), (PPLANE_SHAPES, "pplane")):
        for shape in shapes:
            assert _route(shape, 1, 0) == (eng, 1) and _route(shape, 1, 1) == (eng, 1), shape
    for shape, stride, splits in SPLIT_SHAPES:
        assert _route(shape, stride, 1) == ("igemm-split", splits) and _route(shape, stride, 0) == ("igemm", 1), shape
    for shape, eng in GN_SHAPES:
        assert _route(shape, 1, 0) == (eng, 1), shape
    for name, D, Hh, W, Cin, Cout, stride, eng, splits in PRODUCT:
        assert H.op_conv3d_route(4, D, Hh, W, Cin, Cout, stride, 1 if stride == 1 else 0, 1) == (eng, splits), name
    # one sample per pass (the B = 1 latency path): fewer workgroups than the persistent and plane forms need
    assert H.op_conv3d_route(1, 128, 64, 32, 64, 64, 1, 1, 1) == ("plane", 1) and H.op_conv3d_route(1, 64, 32, 16, 64, 64, 1, 1, 1) == ("line", 1)
    L = lib()
    for bad in ((4, 8, 8, 8, 96, 64, 1, 1, 0), (4, 8, 8, 8, 64, 6, 1, 1, 0), (4, 8, 8, 8, 64, 64, 3, 1, 0), (4, 8, 8, 8, 64, 64, 1, 1, 2),
                (0, 8, 8, 8, 64, 64, 1, 1, 0), (4, 1, 8, 8, 64, 64, 2, 0, 0)):
        assert L.rald_op_conv3d_route(*bad, None) == -1 and b"rald_op_conv3d_route" in L.rald_last_error(), bad


# ---- exact-integer data: every engine bit for bit -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,stride", IGEMM_SHAPES)
def test_conv3d_igemm_engine_exact_on_integer_data(shape, stride):
    """conv3d_igemm_kernel in one pass (allow_split = 0): a tail tile (M = 180, 72, 360 - no multiple of 128), Cout < 64 with clamped weight rows
    and masked columns, W = 8 with M % 128 != 0, two k-chunks per tap with a partial second n-tile, and stride 2 / pad 0 against
    F.pad(0, 1) + k3 s2 (odd depth 5 included).  plain, resid == out and out_bf16: 0 elements differ."""
    _exact_conv(shape, stride, "igemm")


@gpu
@pytest.mark.parametrize("shape", LINE_SHAPES)
def test_conv3d_line_engine_exact_on_integer_data(shape):
    """conv3d_line_kernel: a tile spanning two d-planes and one crossing the sample boundary (H = W = 8, D = 3), H no multiple of a tile's 8 lines
    (W = 16), H smaller than a tile's 4 lines with Cin = 128 (the tap-major weight index), the decoder's conv_out form Cout = 4 and
    Cout = 16 (clamped weight rows, masked columns), and a shape the plane engines take when it is large enough.  0 elements differ."""
    _exact_conv(shape, 1, "line")


@gpu
@pytest.mark.parametrize("shape", PLANE_SHAPES)
def test_conv3d_plane_engine_exact_on_integer_data(shape):
    """conv3d_plane_kernel at its floor of 256 workgroups x 256 voxels (D = 12 keeps the persistent form away): W = 16 with six h-blocks per plane,
    W = 32 with two n-tiles; the d faces, the h-block seams and the w aprons are all in the comparison.  0 elements differ."""
    _exact_conv(shape, 1, "plane")


@gpu
@pytest.mark.parametrize("shape", PPLANE_SHAPES)
def test_conv3d_pplane_engine_exact_on_integer_data(shape):
    """conv3d_pplane_kernel at its floor of 256 workgroups x 8 planes: the whole output (every segment's first and last plane, both d faces, the
    h-block seams) against the float64 convolution.  0 elements differ."""
    _exact_conv(shape, 1, "pplane")


@gpu
@pytest.mark.parametrize("shape,stride,splits", SPLIT_SHAPES)
def test_conv3d_split_k_route_exact_and_identical_to_one_pass(shape, stride, splits):
    """The encoder's split-K route (allow_split = 1): conv3d_igemm_kernel with gridDim.z = splits + conv_split_reduce_kernel, through a NaN-filled
    workspace: 9 ranges of 3 k-steps, 16 uneven ranges of 108, Cout = 16 (masked columns in the partial stores, bias by i % Cout in the reduce),
    stride 2.  plain and in place (resid == out, both __restrict__ in the reduce kernel): 0 elements differ from float64, and the result
    equals the allow_split = 0 result bit for bit."""
    assert _route(shape, stride, 1) == ("igemm-split", splits)
    d, dev, outs = _exact_conv(shape, stride, "igemm-split", allow_split=1)
    for mode, got in zip(("plain", "inplace"), outs):
        one, _ = _conv_run(d, shape, stride, dev, mode, allow_split=0)
        assert torch.equal(_bits(one.contiguous()), _bits(got.contiguous())), (shape, mode)


# ---- GroupNorm partials from the convolution epilogue ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,engine", GN_SHAPES)
def test_conv3d_epilogue_groupnorm_partials_exact_then_gn_finish(shape, engine):
    """ConvArgs::gn_part on every tile form (igemm: slot blockIdx.y; line; plane: two slots per workgroup; pplane: m0 / 128 + half), Cout 64,
    128 and 256.  Inputs and weights in {-1, 0, 1}: the test asserts |output| <= 500 on the reference (measured max 130 to 240), so the 64
    squares a DPP row sums stay below 2^24 and every fp32 lane sum is exact: each slot gn_part[m / 128][g] must equal the float64 {sum, sum of
    squares} of that tile's 128 voxels and that group's channels bit for bit, with and without the in-place residual.  rald_op_gn_finish on
    the slots must equal the float64 per-sample sums exactly, and the statistics rald_op_groupnorm computes from the same fp32 output
    (its per-lane fp32 sums cover C squares: exact while C * max^2 < 2^24, asserted)."""
    from rald_amd import _handles as H
    from rald_amd import train_encoder as TE
    B, D, Hh, W, Cin, Cout = shape
    assert _route(shape, 1, 0) == (engine, 1)
    d = _conv_data(shape, 1, "tri")
    dev = _upload(d)
    M, So, cpg = d["M"], d["M"] // B, Cout // 32
    for mode in ("plain", "inplace"):
        want = d["base"] + d["resid"].double() if mode == "inplace" else d["base"]
        amax = float(want.abs().max())
        print(f"max |output| {mode}: {amax}")
        assert amax <= 500 and Cout * amax * amax < 2 ** 24
        got, part = _conv_run(d, shape, 1, dev, mode, gn=True)
        _same_bits(got, want, f"conv+gn {engine} {shape} {mode}")
        t = want.reshape(M // 128, 128, 32, cpg)
        ref = torch.stack([t.sum((1, 3)), (t * t).sum((1, 3))], -1)                     # [tiles, 32, 2]
        nbad = int((part.cpu() != ref).sum())
        print(f"ratio gn_part {engine} {shape} {mode}: {nbad} of {ref.numel()} slots differ (bound 0)")
        assert nbad == 0
        stats = _guarded(B * 64, 64, dtype=torch.float64)
        H.op_gn_finish(part, stats, B, So // 128)
        torch.cuda.synchronize()
        assert _guard_ok(stats, B * 64)
        sref = ref.reshape(B, So // 128, 32, 2).sum(1)
        assert torch.equal(stats[:B * 64].view(B, 32, 2).cpu(), sref), (shape, mode, "gn_finish")
        ones, zeros = torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda")
        _, st2 = TE.groupnorm(got.reshape(B, So, Cout).contiguous(), ones, zeros, False)
        assert torch.equal(st2.cpu(), sref), (shape, mode, "rald_op_groupnorm statistics")


@gpu
@pytest.mark.parametrize("nblk", [1, 5, 16, 17, 100])
def test_gn_finish_alone_on_integer_valued_doubles(nblk):
    """rald_op_gn_finish (gn_finish_kernel on caller partials): sixteen contiguous ranges of nblk slots, empty ranges (nblk = 1, 5), exactly one slot
    each (16), uneven (17, 100); B = 3; integer-valued doubles up to 2^40, so any order is exact: every statistic equals the float64 sum."""
    from rald_amd import _handles as H
    B = 3
    g = _g(40 + nblk)
    part = torch.randint(-(1 << 40), 1 << 40, (B * nblk, 32, 2), generator=g).double()
    buf = torch.full((B * nblk + 2, 32, 2), float("nan"), dtype=torch.float64)
    buf[1:-1] = part
    dbuf = buf.cuda()
    stats = _guarded(B * 64, 64, dtype=torch.float64)
    H.op_gn_finish(dbuf[1:-1], stats, B, nblk)
    torch.cuda.synchronize()
    assert _guard_ok(stats, B * 64)
    assert torch.equal(stats[:B * 64].view(B, 32, 2).cpu(), part.view(B, nblk, 32, 2).sum(1))


# ---- random data: the fp32 accumulation per element -----------------------------------------------------------------------------------
def _slab_planes(D):
    """output d-planes the persistent-plane reference covers: both faces and a segment's end, the next segment's start and its second plane"""
    return sorted({0, 1, 7, 8, 9, D - 2, D - 1})


@gpu
@pytest.mark.parametrize("shape,stride,engine,allow_split", [
    ((3, 5, 3, 4, 128, 72), 1, "igemm", 0), ((3, 2, 2, 32, 128, 128), 1, "line", 0),
    ((4, 12, 48, 32, 64, 128), 1, "plane", 0), ((3, 8, 4, 2, 256, 256), 1, "igemm-split", 1)])
def test_conv3d_engines_random_data_per_element(shape, stride, engine, allow_split):
    """Unit-variance bf16 inputs, weights ~ (27 Cin)^-1/2, fp32 bias and residual (a separate buffer here), against float64 of the same bf16 values:
    |got - ref| <= k * 2^-24 * (|bias| + |resid| + sum |w x|) per element, and for out_bf16 (no residual, no split) one bf16 ulp of the reference
    more.  Measured k on an MI355X (fp32 / bf16): igemm 1.47 / 0.192, line 1.38 / 0.0581, plane 2.09 / 0.393, split-K 0.421; bounds BOUNDS_RND."""
    from rald_amd import _handles as H
    assert _route(shape, stride, allow_split)[0] == engine
    d = _conv_data(shape, stride, "rnd")
    dev = _upload(d)
    B, D, Hh, W, Cin, Cout = shape
    n = d["M"] * Cout
    out = _guarded(n, 64)
    ws = torch.full((_route(shape, stride, allow_split)[1] * n,), float("nan"), device="cuda") if engine == "igemm-split" else None
    H.op_conv3d_full(dev["x"], dev["wp"], dev["bias"], B, D, Hh, W, Cin, Cout, out=out, resid=dev["resid"], split_ws=ws, allow_split=allow_split,
                     stride=stride, pad=1 if stride == 1 else 0)
    torch.cuda.synchronize()
    assert _guard_ok(out, n)
    k32 = _ratio(out[:n].view(-1, Cout), d["base"] + d["resid"].double(), d["terms"] + d["resid"].double().abs())
    k16 = None
    if engine != "igemm-split":
        got16, _ = _conv_run(d, shape, stride, dev, "bf16", allow_split)
        k16 = _ratio16(got16, d["base"], d["terms"])
    b32, b16 = BOUNDS_RND[engine]
    _le(f"conv rnd {engine} fp32", k32, b32)
    if k16 is not None:
        _le(f"conv rnd {engine} bf16", k16, b16)


@gpu
def test_conv3d_pplane_engine_random_data_per_element_on_d_slabs():
    """The persistent-plane engine on random data at its floor shape (4, 64, 64, 32, 64, 64).  The float64 reference is computed on d-slabs with a
    one-plane halo for every sample's output planes 0, 1, 7, 8, 9, D-2, D-1 (the volume's faces, a segment's last plane, the next segment's
    first two - where the rolling window has just replaced a plane), all h and w (the h-block seams included); same bound form as above.
    Measured k on an MI355X: 2.17; bound 5.4."""
    from rald_amd import _handles as H
    shape = PPLANE_SHAPES[0]
    B, D, Hh, W, Cin, Cout = shape
    assert _route(shape, 1, 0) == ("pplane", 1)
    g = _g(77)
    x = torch.randn(B, D, Hh, W, Cin, generator=g).bfloat16()
    Wt = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (27 * Cin) ** -0.5).bfloat16()
    bias = torch.randn(Cout, generator=g)
    resid = torch.randn(B, D, Hh, W, Cout, generator=g)
    keep, xd = _embed(x)
    n = B * D * Hh * W * Cout
    out = _guarded(n, 64)
    H.op_conv3d_full(xd, _pack(Wt).cuda(), bias.cuda(), B, D, Hh, W, Cin, Cout, out=out, resid=resid.cuda())
    torch.cuda.synchronize()
    assert _guard_ok(out, n)
    got = out[:n].view(B, D, Hh, W, Cout)
    xp = F.pad(x.double().permute(0, 4, 1, 2, 3), (0, 0, 0, 0, 1, 1))                       # one zero plane at each d face
    W64 = Wt.double()
    worst = 0.0
    for dd in _slab_planes(D):
        slab = xp[:, :, dd:dd + 3]
        ref = F.conv3d(slab, W64, padding=(0, 1, 1))[:, :, 0].permute(0, 2, 3, 1) + bias.double()
        terms = F.conv3d(slab.abs(), W64.abs(), padding=(0, 1, 1))[:, :, 0].permute(0, 2, 3, 1) + bias.double().abs()
        r = resid[:, dd].double()
        worst = max(worst, _ratio(got[:, dd], ref + r, terms + r.abs()))
    _le("conv rnd pplane fp32", worst, BOUNDS_RND["pplane"][0])


# measured k on an MI355X (fp32, bf16) -> bounds at most 2.5 times that
BOUNDS_RND = {"igemm": (3.6, 0.48), "line": (3.4, 0.14), "plane": (5.2, 0.98), "pplane": (5.4, None), "igemm-split": (1.05, None)}


# ---- GroupNorm forward ----------------------------------------------------------------------------------------------------------------
GN_EPS = float(torch.tensor(1e-6, dtype=torch.float32))               # the kernel widens the fp32 constant
# measured k on an MI355X per channel count (worst over the eight S and both activations) -> bounds at most 2.5 times that:
#   C = 64:  sum 4.71, sumsq 3.1, y plain 0.397, constant group 1.34, mean = 50 dev 3.95e4
#   C = 128: sum 9.41, sumsq 3.1, y plain 0.367, constant group 2.15, mean = 50 dev 67.5
#   C = 256: sum 20,   sumsq 23.2, y plain 0.547, constant group 2.72, mean = 50 dev 87.8
#   S = 16 400, C = 64: sum 4.7, sumsq 3.1, y plain 0.38, constant group 0 (within the bf16 ulp), mean = 50 dev 5.96
# The statistics' k grows with C because one lane's fp32 partial sums cover C values.  "mean = 50 dev" is what var = E[x^2] - mean^2 costs: the
# error of var is k 2^-24 E[x^2], i.e. relative mean^2 / var times larger - 2 500 for a group at 50 deviations (k of 6 to 90 at S >= 15), and
# unbounded in principle where a group of 2 to 8 values (S = 1, 3 at C = 64) happens to lie closer together than that: the 3.95e4.
BOUNDS_GN = {64: {"sum": 11, "sumsq": 7.5, "y plain": 0.95, "y constant group": 3.3, "y mean 50 dev": 9.8e4},
             128: {"sum": 23, "sumsq": 7.5, "y plain": 0.9, "y constant group": 5.3, "y mean 50 dev": 165},
             256: {"sum": 50, "sumsq": 58, "y plain": 1.35, "y constant group": 6.8, "y mean 50 dev": 215},
             "S16400": {"sum": 11, "sumsq": 7.5, "y plain": 0.95, "y constant group": 0.0, "y mean 50 dev": 14}}


def _gn_case(C, S, swish, seed):
    """One GroupNorm forward + apply at (B = 3, S, C): returns the measured ratios by class."""
    from rald_amd._lib import check, lib
    B, cpg = 3, C // 32
    g = _g(seed)
    x = torch.randn(B, S, C, generator=g)
    x[0] = x[0] * 1.5 + 0.3
    x[0, :, 5 * cpg:6 * cpg] = 1.7                                  # a constant group: var clamps (or comes out as rounding noise)
    x[1] = x[1] + 50.0                                              # mean = 50 deviations: the E[x^2] - mean^2 form loses ~11 bits
    x[2] = x[2] * 0.5 - 0.2
    gamma = 1 + 0.5 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    xb = torch.full((B * S + 2, C), float("nan"))
    xb[1:-1] = x.reshape(B * S, C)
    xd = xb.cuda()
    nblk = (S + 511) // 512
    nst = B * 64 * (1 + nblk)
    res = []
    for _ in range(2):
        y = _guarded(B * S * C, 64, dtype=torch.bfloat16)
        res.append(y)
    stats = _guarded(nst, 64, dtype=torch.float64)
    gd, bd = gamma.cuda(), beta.cuda()
    check(lib().rald_op_groupnorm(xd[1:-1].data_ptr(), gd.data_ptr(), bd.data_ptr(), res[0].data_ptr(), stats.data_ptr(), B, S, C, swish,
                                  torch.cuda.current_stream().cuda_stream))
    check(lib().rald_op_groupnorm_apply(xd[1:-1].data_ptr(), stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), res[1].data_ptr(), B, S, C, swish,
                                        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _guard_ok(res[0], B * S * C) and _guard_ok(res[1], B * S * C) and _guard_ok(stats, nst)
    assert torch.equal(_bits(res[0]), _bits(res[1])), "rald_op_groupnorm_apply differs from the forward call"
    x64 = x.double().view(B, S, 32, cpg)
    s_ref, q_ref = x64.sum((1, 3)), (x64 * x64).sum((1, 3))
    st = stats[:B * 64].view(B, 32, 2).cpu()
    out = {"sum": _ratio(st[..., 0], s_ref, x64.abs().sum((1, 3))), "sumsq": _ratio(st[..., 1], q_ref, q_ref)}
    n = S * cpg
    mean = (s_ref / n).view(B, 1, 32, 1)
    var = ((x64 - mean) ** 2).mean((1, 3), keepdim=True)             # the float64 statement: exactly 0 for the constant group
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    g64, b64 = gamma.double().view(1, 1, 32, cpg), beta.double().view(1, 1, 32, cpg)
    yr = (x64 - mean) * rstd * g64 + b64
    terms = (x64.abs() + mean.abs()) * rstd * g64.abs() + b64.abs()
    if swish:
        sg = torch.sigmoid(yr)
        terms = terms * (sg * (1 + yr * (1 - sg))).abs() + (yr * sg).abs()
        yr = yr * sg
    got = res[0][:B * S * C].view(B, S, 32, cpg)
    const = torch.zeros(B, 1, 32, 1, dtype=torch.bool)
    const[0, 0, 5, 0] = True
    m50 = torch.zeros(B, 1, 32, 1, dtype=torch.bool)
    m50[1] = True
    for name, mask in (("y constant group", const), ("y mean 50 dev", m50), ("y plain", ~(const | m50))):
        mk = mask.expand(B, S, 32, cpg)
        out[name] = _ratio16(got.cpu()[mk], yr[mk], terms[mk])
    return out


@gpu
@pytest.mark.parametrize("C", [64, 128, 256])
def test_groupnorm_forward_statistics_and_output_against_float64(C):
    """rald_op_groupnorm (gn_stats_kernel, gn_finish_kernel, gn_apply_kernel) at B = 3, S in {1, 3, 15, 17, 511, 512, 513, 1100} (below one
    unrolled step of 4 * 256 / (C / 4) voxels, the unrolled loop's tail, a last statistics block of 1 and of 76 voxels), swish on and off; C = 64
    is the cpg = 2 half-quad path.  Statistics per (sample, group): |sum - ref| <= k 2^-24 sum |x|, |sumsq - ref| <= k 2^-24 sum x^2.
    Output per element: one bf16 ulp of the float64 value + k 2^-24 t, t = (|x| + |mean|) rstd |gamma| + |beta|, through the swish
    t |swish'(y)| + |swish(y)|.  Sample 0 has one constant group (float64: var = 0, the output is act(beta); the kernel's E[x^2] - mean^2 is
    rounding noise there, clamped at 0); sample 1 has mean = 50 deviations (its k is reported and bounded on its own: the bound is relative to
    |x| + |mean|, so it documents what E[x^2] - mean^2 costs instead of failing on it).  rald_op_groupnorm_apply on the same statistics is
    bit-identical.  Measured k on an MI355X and the bounds: the table at BOUNDS_GN."""
    worst = {}
    for S in (1, 3, 15, 17, 511, 512, 513, 1100):
        for swish in (0, 1):
            for k, v in _gn_case(C, S, swish, 500 + S + C + swish).items():
                worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        print(f"ratio groupnorm C={C} {k}: {v:.3g} (bound {BOUNDS_GN[C][k]})")
    for k, v in worst.items():
        assert v <= BOUNDS_GN[C][k], (C, k, v)


@gpu
def test_groupnorm_forward_grid_stride_loop_past_1024_blocks():
    """S = 16 400, C = 64: S * C / 4 = 262 400 quads, 256 more than the 1 024 blocks of gn_apply_kernel cover in one pass (the grid-stride
    loop's second trip), and 33 statistics blocks (the last of 16 voxels) over gn_finish's sixteen ranges.  Measured k and bounds: the
    "S16400" row of BOUNDS_GN."""
    out = _gn_case(64, 16400, 1, 9)
    for k, v in out.items():
        print(f"ratio groupnorm S=16400 {k}: {v:.3g} (bound {BOUNDS_GN['S16400'][k]})")
    for k, v in out.items():
        assert v <= BOUNDS_GN["S16400"][k], (k, v)


# ---- the small kernels ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [4, 64, 136])
def test_upsample2_cast_is_repeat_interleave_then_bf16(C):
    """rald_op_upsample2_cast at B = 3, (D, H, W) = (3, 1, 5) (odd, one of them 1), C = 4 (one quad), 64, 136 (no power of two): bit-identical to
    repeat_interleave x2 on the three axes followed by .bfloat16()."""
    from rald_amd import _handles as H
    B, D, Hh, W = 3, 3, 1, 5
    x = torch.randn(B, D, Hh, W, C, generator=_g(60 + C)) * 3
    xb = torch.full((B * D + 2, Hh, W, C), float("nan"))
    xb[1:-1] = x.reshape(B * D, Hh, W, C)
    xd = xb.cuda()
    n = B * 8 * D * Hh * W * C
    y = _guarded(n, 64, dtype=torch.bfloat16)
    H.op_upsample2_cast(xd[1:-1], y, B, D, Hh, W, C)
    torch.cuda.synchronize()
    assert _guard_ok(y, n)
    want = x.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3).bfloat16()
    assert torch.equal(_bits(y[:n].cpu()), _bits(want.reshape(-1)))


@gpu
@pytest.mark.parametrize("zc", [1, 4, 16, 63, 64])
def test_pad_cast64_zero_fills_beyond_zc(zc):
    """rald_op_pad_cast64 with 3 and 37 rows (192 and 2 368 elements: less than one workgroup, and 9.25 of them): columns < zc are torch's bf16
    rounding of z, the others exact zeros, bit for bit; nothing behind the last row is written."""
    from rald_amd import _handles as H
    for rows in (3, 37):
        z = torch.randn(rows, zc, generator=_g(70 + zc + rows)) * 3
        zb = torch.full((rows + 2, zc), float("nan"))
        zb[1:-1] = z
        zd = zb.cuda()
        y = _guarded(rows * 64, 64, dtype=torch.bfloat16)
        H.op_pad_cast64(zd[1:-1], y, rows, zc)
        torch.cuda.synchronize()
        assert _guard_ok(y, rows * 64)
        want = torch.zeros(rows, 64, dtype=torch.bfloat16)
        want[:, :zc] = z.bfloat16()
        assert torch.equal(_bits(y[:rows * 64].cpu()), _bits(want.reshape(-1))), rows


BOUND_TOKENS = {7: 7.4, 16: 9.1}                       # measured k on an MI355X: 2.99 (zc = 7), 3.65 (zc = 16)


@gpu
@pytest.mark.parametrize("zc", [7, 16])
def test_radar_tokens_projection_and_three_embeddings_against_float64(zc):
    """rald_op_radar_tokens (radar_token_kernel, the tokeniser without the encoder): B = 3, token grid (R, A, E) = (4, 3, 2) - three distinct
    sizes, so a swapped embedding index reads another row -, C = 520 (no multiple of the 256 threads: a third, partial trip of the channel
    loop), zc = 16 and 7.  Per element |got - ref| <= k 2^-24 (|b| + sum |z W| + |r| + |a| + |e|).  Measured k on an MI355X: 2.99 (zc = 7), 3.65 (zc = 16); bounds 7.4, 9.1."""
    from rald_amd import _handles as H
    B, R, A, E, C = 3, 4, 3, 2, 520
    g = _g(80 + zc)
    z = torch.randn(B, R, A, E, zc, generator=g)
    Wp, bp = torch.randn(C, zc, generator=g) * zc ** -0.5, torch.randn(C, generator=g)
    re, ae, ee = torch.randn(R, C, generator=g), torch.randn(A, C, generator=g) * 2, torch.randn(E, C, generator=g) * 0.5
    zb = torch.full((B * R + 2, A, E, zc), float("nan"))
    zb[1:-1] = z.reshape(B * R, A, E, zc)
    zd = zb.cuda()
    n = B * R * A * E * C
    tok = _guarded(n, 64)
    H.op_radar_tokens(zd[1:-1], Wp.cuda(), bp.cuda(), re.cuda(), ae.cuda(), ee.cuda(), tok, B, R, A, E, zc, C)
    torch.cuda.synchronize()
    assert _guard_ok(tok, n)
    emb = re.double()[:, None, None] + ae.double()[None, :, None] + ee.double()[None, None, :]            # [R, A, E, C]
    ref = z.double() @ Wp.double().t() + bp.double() + emb
    terms = z.double().abs() @ Wp.double().abs().t() + bp.double().abs() + re.double().abs()[:, None, None] + ae.double().abs()[None, :, None] + \
        ee.double().abs()[None, None, :]
    _le(f"radar_tokens zc={zc}", _ratio(tok[:n].view(B, R, A, E, C), ref, terms), BOUND_TOKENS[zc])


# ---- argument checks (CPU: each fires before the entry's first HIP call) --------------------------------------------------------------
def test_argument_checks_of_the_radar_op_entries_name_the_constraint(L_cpu):
    L, d = L_cpu, DUMMY

    def full(out=d, out16=None, resid=None, gn=None, ws=None, ws_bytes=0, allow=0, shape=(3, 4, 16, 16, 64, 64), stride=1, pad=1, x=d):
        return L.rald_op_conv3d_full(x, d, d, resid, out, out16, gn, ws, ws_bytes, allow, *shape, stride, pad, None)

    _refused(L, full(x=None), "null pointer")
    _refused(L, full(out=None), "null pointer")
    _refused(L, full(shape=(3, 4, 16, 16, 96, 64)), "Cin must be a multiple of 64")
    _refused(L, full(shape=(3, 4, 16, 16, 64, 6)), "Cout of 4")
    _refused(L, full(stride=3), "bad geometry")
    _refused(L, full(shape=(3, 1, 16, 16, 64, 64), stride=2, pad=0), "bad geometry")
    _refused(L, full(allow=2), "allow_split")
    # out_bf16 excludes out, resid and a split route
    _refused(L, full(out=d, out16=d), "bf16 result replaces the fp32 one")
    _refused(L, full(out=None, out16=d, resid=d), "takes no residual")
    split = (3, 8, 4, 2, 256, 256)                                   # 16 ranges, M = 192
    need = 16 * 192 * 256 * 4
    _refused(L, full(out=None, out16=d, ws=d, ws_bytes=need, allow=1, shape=split), "bf16 result", "splits K")
    # the split workspace
    _refused(L, full(allow=1, shape=split), "split-K", "16-byte aligned workspace")
    _refused(L, full(ws=d + 8, ws_bytes=need, allow=1, shape=split), "split-K", "16-byte aligned workspace")
    _refused(L, full(ws=d, ws_bytes=need - 4, allow=1, shape=split), "workspace too small")
    # gn_part: So % 128 == 0, Cout in {64, 128, 256}, no split
    _refused(L, full(gn=d, shape=(2, 3, 8, 8, 64, 64)), "gn_part", "% 128 == 0")
    _refused(L, full(gn=d, shape=(3, 4, 16, 16, 64, 192)), "gn_part", "64, 128 or 256")
    _refused(L, full(gn=d, shape=(3, 4, 16, 16, 64, 16)), "gn_part", "64, 128 or 256")
    _refused(L, full(gn=d, ws=d, ws_bytes=16 * 384 * 256 * 4, allow=1, shape=(3, 8, 4, 4, 256, 256)), "gn_part", "splits K")
    _refused(L, L.rald_op_gn_finish(None, d, 3, 4, None), "gn_finish", "null pointer")
    _refused(L, L.rald_op_gn_finish(d, d, 3, 0, None), "gn_finish", "nblk must be positive")
    _refused(L, L.rald_op_gn_finish(d, d, 0, 4, None), "gn_finish", "must be positive")
    _refused(L, L.rald_op_upsample2_cast(d, d, 3, 3, 1, 5, 6, None), "upsample2_cast", "multiple of 4")
    _refused(L, L.rald_op_upsample2_cast(d, None, 3, 3, 1, 5, 8, None), "upsample2_cast", "null pointer")
    _refused(L, L.rald_op_upsample2_cast(d, d, 3, 0, 1, 5, 8, None), "upsample2_cast", "bad shape")
    _refused(L, L.rald_op_upsample2_cast(d + 4, d, 3, 3, 1, 5, 8, None), "upsample2_cast", "aligned")
    _refused(L, L.rald_op_pad_cast64(d, d, 10, 65, None), "pad_cast64", "1 .. 64")
    _refused(L, L.rald_op_pad_cast64(d, d, 10, 0, None), "pad_cast64", "1 .. 64")
    _refused(L, L.rald_op_pad_cast64(d, d, 0, 16, None), "pad_cast64", "row count")
    _refused(L, L.rald_op_radar_tokens(d, d, d, d, d, d, d, 3, 4, 3, 2, 65, 520, None), "radar_tokens", "1 .. 64")
    _refused(L, L.rald_op_radar_tokens(d, d, d, d, None, d, d, 3, 4, 3, 2, 16, 520, None), "radar_tokens", "null pointer")
    _refused(L, L.rald_op_radar_tokens(d, d, d, d, d, d, d, 70000, 4, 3, 2, 16, 520, None), "radar_tokens", "B <= 65535")
