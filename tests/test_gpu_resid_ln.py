"""The residual projection of the latent stacks, x += A.W^T + bias followed by the next (Ada)LayerNorm, per element against float64:
the dispatcher resid_gemm_ln (route 0), the fused kernel gemm_resid_ln (route 1) in its eight compiled forms with every run-time switch,
and the GEGLU epilogue that feeds its MXFP8 form.  Everything goes through rald_op_resid_gemm_ln / rald_op_gemm_geglu_mx8out, which fill
the same argument blocks as the models.  Conventions are those of test_gpu_train_ops.py: float64 references computed on the CPU from
exactly the values the kernel read (bf16 and e4m3 x e8m0 inputs widened exactly; only the float64 matrix product itself runs on the
device), outputs pre-filled with NaN, guard tails that must survive bit for bit, x starting from non-trivial values, modulation and
weight groups with distinct values, measured ratios printed and bounds at most 2.5 times the worst value measured on an MI355X.

Bounds, per element:
  x (fp32)   |x - ref| <= k * 2^-24 * (sum_k |a||w| + |bias| + |x_old|)          (+ sum_s 2^-11 |partial_s| through fp16 slabs)
  h (bf16)   one bf16 ulp of the float64 value + k * 2^-24 * T,
             T = rstd |add_one + g| (|v - mean| (1 + E[v^2] / (var + eps)) + mean_j |v_j|) + |b|
             (the E[v^2] / (var + eps) factor is the fused kernel's single-pass variance t2/512 - mean^2 in fp32)
  integer data: x bit-equal to the float64 result (every partial sum is an integer below 2^24, exact in fp32 in any order).

What reaches what (fused kernel = route 1; forms are <rows per tile>/<operands>/<GU = group-uniform modulation or per-row>):
  64/bf16/GU, 64/bf16/per-row; nk < 8, = 8, >= 9 (x_old after the loop, last piece after the loop, pieces in k-steps 0..8); M = 1, 63, 64,
      65, 1000; gstride 0, rows_per_group 512 / 64 (GU) and 250 / 3 (per-row), partial last group; nt_io 0 = 1
                                                     test_fused_64row_bf16_exact_integers, test_fused_bf16_random_per_element_bounds
  128/bf16/GU, 128/bf16/per-row; pipelined loop with nk = 1, 2, 3, 8, 32; last tile of 1, 17, 127, 128 rows; rows_per_group 64 and 250
      straddle, 512 and gstride 0 are GU; nt_io 0 = 1
                                                     test_fused_128row_bf16_exact_integers, test_fused_bf16_random_per_element_bounds
  64/MX and 128/MX, GU and per-row, ragged M          test_fused_mx8_operands_exact_integers
  h8 / hs (quantising epilogue) in all four bf16 / MX x 64 / 128 forms, zero block, ragged last tile
                                                     test_fused_h8_hs_equals_quantised_h
  strideW / w_rows with the XCD tile remap active and inactive, both tile heights, ragged last group
                                                     test_fused_per_group_weights_exact_integers
  the LDS the epilogue reuses, all eight forms        test_fused_results_do_not_depend_on_stale_lds
  route 0: fp16 slabs on the 64x64 ring (M = 512) and on 128x128 (M = 1600, 4096), fp32 slabs (M = 1000), gemm_nt + LayerNorm (M = 4097;
      K = 512 at M = 16383), fused (K = 512 at M = 16384), no LayerNorm (g null), h8 / hs (gemm_nt + layernorm_mod_mx8), strideW (batched
      gemm_nt)                                        test_dispatcher_routes_per_element, test_dispatcher_per_group_weights_exact_integers
  GEGLU epilogue on 128x128 tiles; on 256x256 tiles with out8 / outs from bf16 and MXFP8 operands
                                                     test_geglu_128x128_per_element, test_geglu_256x256_mx8_output_equals_quantised_bf16_output
  argument checks (CPU)                               test_argument_checks_refuse_before_any_launch"""
import math
import time

import pytest
import torch

gpu = pytest.mark.gpu
U = 2.0 ** -24
EPS = 1e-5


# ---- helpers (test_gpu_train_ops.py's) -------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _f64(t):
    return t.detach().cpu().double()


def _ratio(got, ref, terms, extra=None):
    """max (|got - ref| - extra) / (2^-24 * terms) over the elements (fp32 result)"""
    err = (_f64(got) - ref).abs()
    e = err if extra is None else (err - extra).clamp_min(0)
    r = e / (U * terms.clamp_min(2.0 ** -126))
    r = torch.where(torch.isnan(err), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def _ratio16(got, ref, terms, extra=None):
    """bf16 result: the error beyond one bf16 ulp of the float64 value (and `extra`), in units of 2^-24 * terms"""
    a = ref.abs().clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
    err = (_f64(got.float()) - ref).abs()
    e = err - ulp if extra is None else err - ulp - extra
    r = e.clamp_min(0) / (U * terms.clamp_min(2.0 ** -126))
    r = torch.where(torch.isnan(err), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


class _Checks:
    """prints every measured ratio, then asserts them all (so one run shows every figure)"""

    def __init__(self):
        self.bad = []

    def le(self, name, value, bound):
        print(f"ratio {name}: {value:.3g} (bound {bound})")
        if not value <= bound:
            self.bad.append((name, value, bound))

    def true(self, name, ok):
        if not ok:
            self.bad.append((name, "failed"))

    def done(self):
        assert not self.bad, self.bad


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


SENT = -12345.5                               # guard value of the float buffers (compared bit for bit in the buffer's own dtype)
SENT8 = 0xA5                                  # ... and of the byte buffers


def _guarded(n, extra, dtype=torch.float32, fill=float("nan")):
    """a device buffer of n + extra elements: the first n filled with `fill`, the guard tail with the sentinel"""
    buf = torch.full((n + extra,), SENT8 if dtype == torch.uint8 else SENT, dtype=dtype, device="cuda")
    buf[:n] = fill
    return buf


def _guard_ok(buf, n):
    tail = buf[n:]
    return bool(torch.equal(_bits(tail), _bits(torch.full_like(tail, SENT8 if buf.dtype == torch.uint8 else SENT))))


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_g(seed)).float()


@pytest.fixture(scope="module")
def H():
    from rald_amd import _handles
    return _handles


@pytest.fixture(autouse=True)
def _timed(request):
    t = time.perf_counter()
    yield
    print(f"time {request.node.name}: {time.perf_counter() - t:.2f} s")


def _e4m3_bytes(v):
    return v.to(torch.float8_e4m3fn).view(torch.uint8)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def _modulation(M, mode, seed, zero_block=False):
    """mode 'ae': one plain gamma / beta row, gstride 0, add_one 0 (the autoencoder's PreNorm); mode '<n>': AdaLN rows [scale | shift] of 1024
    floats per group of n rows, add_one 1.  zero_block: columns 32..63 get g = -add_one, b = 0, so h is exactly zero there."""
    if mode == "ae":
        G, gstride, rpg, add_one = 1, 0, 1 << 30, 0.0
    else:
        rpg = int(mode)
        G, gstride, add_one = -(-M // rpg), 1024, 1.0
    mod = torch.randn(G, 1024, generator=_g(seed)) * 0.5
    if mode == "ae":
        mod[:, :512] += 1.0
    if zero_block:
        mod[:, 32:64] = -add_one
        mod[:, 544:576] = 0.0
    return dict(mod=mod, G=G, gstride=gstride, rpg=rpg, add_one=add_one)


def _case(M, K, mode, seed, kind="int", w_groups=0, w_rows=0, zero_block=False):
    """kind 'int': bf16 integers (A in [-3,3], W in [-2,2] + the asymmetric n % 3 == 0 bump, bias and x_old in [-8,8]: |sum| <= 5*3*2048 + 16);
    'mxint': e4m3 integers in [-4,4] x e8m0 block scales 2^0..2^3 on both sides (products <= 1024, |sum| <= 2^21 at K = 2048);
    'rand': bf16 operands of unit scale, W / sqrt(K), and every fourth row of x_old with |mean| / std = 16."""
    c = dict(M=M, K=K, mx=kind == "mxint", w_rows=w_rows, strideW=512 * K if w_groups else 0, m=_modulation(M, mode, seed + 5, zero_block))
    wshape = (w_groups, 512, K) if w_groups else (512, K)
    bump = (torch.arange(512) % 3 == 0).float()[:, None]
    if kind == "int":
        c["A"] = _ints((M, K), -3, 3, seed)
        c["W"] = _ints(wshape, -2, 2, seed + 1) + bump
        c["bias"], c["x0"] = _ints((512,), -8, 8, seed + 2), _ints((M, 512), -8, 8, seed + 3)
    elif kind == "mxint":
        from oracle import mx_oracle as MX
        c["A8"], c["W8"] = _e4m3_bytes(_ints((M, K), -4, 4, seed)), _e4m3_bytes(_ints((512, K), -4, 3, seed + 1) + bump)
        c["SA"] = (127 + torch.randint(0, 4, (M, K // 32), generator=_g(seed + 6))).to(torch.uint8)
        c["SW"] = (127 + torch.randint(0, 4, (512, K // 32), generator=_g(seed + 7))).to(torch.uint8)
        c["A"], c["W"] = MX.dequantize_mx8(c["A8"], c["SA"]), MX.dequantize_mx8(c["W8"], c["SW"])       # exact: integers x 2^0..3
        c["bias"], c["x0"] = _ints((512,), -8, 8, seed + 2), _ints((M, 512), -8, 8, seed + 3)
    else:
        g = _g(seed)
        c["A"] = torch.randn(M, K, generator=g).bfloat16().float()
        c["W"] = (torch.randn(wshape, generator=g) / K ** 0.5).bfloat16().float()
        c["bias"] = torch.randn(512, generator=g)
        x0 = torch.randn(M, 512, generator=g) * 2 + 0.5
        r = torch.arange(M)
        s = torch.tensor([0.5, 1.0, 2.0])[r % 3][:, None]
        c["x0"] = torch.where((r % 4 == 1)[:, None], 16 * s + s * (x0 - 0.5) / 2, x0)
    return c


def _upload(c):
    d = {}
    if c["mx"]:
        for k in ("A8", "SA", "W8", "SW"):
            d[k] = c[k].cuda()
    else:
        d["A"], d["W"] = c["A"].cuda().bfloat16(), c["W"].cuda().bfloat16()
    d["bias"], d["x0"] = c["bias"].cuda(), c["x0"].cuda()
    m = c["m"]["mod"]
    d["mod"] = torch.cat([m, torch.full((1, 1024), float("nan"))]).cuda().flatten()      # a NaN row behind the last group
    c["d"] = d
    return c


def _products64(c, kparts=1):
    """float64 A.W^T and |A|.|W|^T (device matmul of the exactly widened operands, results on the CPU); kparts > 1 also returns the
    partial products of the kparts equal K-ranges"""
    A = c["A"].cuda().double()
    W = c["W"].cuda().double()
    M, K = c["M"], c["K"]

    def mm(a, w):
        if w.dim() == 2:
            return a @ w.t()
        out = torch.empty(M, 512, dtype=torch.float64, device="cuda")
        for gi in range(w.shape[0]):
            lo, hi = gi * c["w_rows"], min((gi + 1) * c["w_rows"], M)
            if lo < hi:
                out[lo:hi] = a[lo:hi] @ w[gi].t()
        return out
    parts = [mm(A[:, s * (K // kparts):(s + 1) * (K // kparts)], W[..., s * (K // kparts):(s + 1) * (K // kparts)]) for s in range(kparts)]
    P = parts[0] if kparts == 1 else torch.stack(parts).sum(0)
    Pa = mm(A.abs(), W.abs())
    return P.cpu(), Pa.cpu(), [p.cpu() for p in parts]


def _reference(c, kparts=1):
    """v = x_new, the terms of its bound, h and T (module docstring), all float64 on the CPU"""
    P, Pa, parts = _products64(c, kparts)
    bias, x0, m = c["bias"].double(), c["x0"].double(), c["m"]
    v = P + bias + x0
    tx = Pa + bias.abs() + x0.abs()
    grp = torch.arange(c["M"]) // m["rpg"] if m["gstride"] else torch.zeros(c["M"], dtype=torch.long)
    gg, bb = m["mod"][grp, :512].double(), m["mod"][grp, 512:].double()
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    sc = m["add_one"] + gg
    h = (v - mean) * rstd * sc + bb
    T = rstd * sc.abs() * ((v - mean).abs() * (1 + (v * v).mean(1, keepdim=True) / (var + EPS)) + v.abs().mean(1, keepdim=True)) + bb.abs()
    return dict(v=v, tx=tx, h=h, T=T, parts=parts)


def _launch(H, c, route=1, out="h", nt_io=1, ln=True):
    """one call into fresh guarded buffers; returns the outputs on the CPU.  out: 'h' (bf16) or 'h8' (h8 / hs); ln False: g and b null."""
    d, M, K, m = c["d"], c["M"], c["K"], c["m"]
    n = M * 512
    xb = _guarded(n, 2048)
    xb[:n] = d["x0"].flatten()
    kw, bufs = {}, {"x": (xb, n)}
    if out == "h":
        kw["h"] = _guarded(n, 2048, torch.bfloat16)
        bufs["h"] = (kw["h"], n)
    else:
        kw["h8"], kw["hs"] = _guarded(n, 2048, torch.uint8, 0x7F), _guarded(M * 16, 256, torch.uint8, 0xFF)
        bufs["h8"], bufs["hs"] = (kw["h8"], n), (kw["hs"], M * 16)
    if ln:
        kw.update(g=d["mod"], b=d["mod"][512:], gstride=m["gstride"], rows_per_group=m["rpg"], add_one=m["add_one"])
    if c["mx"]:
        kw.update(A8=d["A8"], SA=d["SA"], W8=d["W8"], SW=d["SW"])
    else:
        kw.update(A=d["A"], W=d["W"])
    if route == 0 and K >= 2048 and M <= 4096:
        kw["scratch"] = _guarded(4 * n, 1024)
        bufs["scratch"] = (kw["scratch"], 4 * n)
    H.op_resid_gemm_ln(xb, d["bias"], M, K, eps=EPS, strideW=c["strideW"], w_rows=c["w_rows"], nt_io=nt_io, route=route, **kw)
    torch.cuda.synchronize()
    for name, (buf, cnt) in bufs.items():
        assert _guard_ok(buf, cnt), f"{name}: guard tail overwritten"
    res = {k: buf[:cnt].cpu() for k, (buf, cnt) in bufs.items() if k != "scratch"}
    res["x"] = res["x"].view(M, 512)
    if "h" in res:
        res["h"] = res["h"].view(M, 512)
    else:
        res["h8"], res["hs"] = res["h8"].view(M, 512), res["hs"].view(M, 16)
    return res


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _exact_case(H, chk, c, name, kh, nt0=True):
    """integer data: x bit-equal to float64, h within its bound, nt_io 0 bit-identical to nt_io 1"""
    ref = _reference(_upload(c))
    r = _launch(H, c)
    chk.true(f"{name}: x exact", torch.equal(r["x"].double(), ref["v"]))
    chk.le(f"{name} h", _ratio16(r["h"], ref["h"], ref["T"]), kh)
    if nt0:
        chk.true(f"{name}: nt_io 0 == 1", _same(r, _launch(H, c, nt_io=0)))
    return r


# bounds that several checks share (measured on an MI355X: the worst value over the cases of the named test; bound <= 2.5 x that)
K_H_INT = {"64": 0.3,                         # h on integer data: test_fused_64row_bf16_exact_integers, measured 0.123
           "128": 1.3,                        # test_fused_128row_bf16_exact_integers, measured 0.54
           "mx": 1.2,                         # test_fused_mx8_operands_exact_integers, measured 0.498
           "strideW": 0.84,                   # test_fused_per_group_weights_exact_integers, measured 0.339
           "route0": 0.6}                     # test_dispatcher_per_group_weights_exact_integers, measured 0.241
K_H_UNFUSED_2048 = 5.4                        # h of gemm_nt + two-pass LayerNorm at K = 2048 (route 0, M = 4097), measured 2.19
K_GEGLU_128 = 0.38                            # measured 0.154
K_GEGLU_256 = {False: 0.3, True: 720}         # bf16 operands measured 0.121; MXFP8 operands 288 (the scaled MFMA's 128-deep dot product is
                                              # no fp32 sum: about 2^-16 of sum |a||w|, as tests/test_fp8.py records for gemm_mx8)


# ---- fused kernel, exact ---------------------------------------------------------------------------------------------------------------
@gpu
def test_fused_64row_bf16_exact_integers(H):
    """gemm_resid_ln<64,1,8>, bf16 operands, M in {1, 63, 64, 65, 1000} x K in {64, 448, 512, 576, 2048} (nk < 8: all of x_old after the loop;
    nk = 8: the last piece after the loop; nk >= 9: pieces in k-steps 0..8) with the modulation cycling through gstride 0, rows_per_group
    512 and 64 (group-uniform form) and 250 (per-row form), rows_per_group 3 at M = 65, and M = 1600 for four groups of 512 with a partial
    last one.  x must equal the float64 result bit for bit; h within its bound (K_H_INT: measured k 0.123); nt_io 0 and
    1 bit-identical."""
    chk = _Checks()
    modes = ["ae", "512", "64", "250"]
    cases = [(M, K, modes[(i * 5 + j) % 4]) for i, M in enumerate((1, 63, 64, 65, 1000)) for j, K in enumerate((64, 448, 512, 576, 2048))]
    cases += [(65, 64, "3"), (65, 576, "3"), (1600, 512, "512"), (1600, 576, "512"), (1000, 512, "64"), (1000, 64, "64")]
    for M, K, mode in cases:
        _exact_case(H, chk, _case(M, K, mode, 1000 + M + K), f"64 bf16 {M}x{K} {mode}", K_H_INT["64"])
    chk.done()


@gpu
@pytest.mark.parametrize("M", [24449, 24448 + 17, 24448 + 127, 24576])
def test_fused_128row_bf16_exact_integers(H, M):
    """gemm_resid_ln<128,2,4> (cdiv(M,128) >= 192), the pipelined loop: K in {64, 128, 192, 512} = nk 1 (no second stage), 2 (only the
    non-DMA iteration), 3 (one DMA iteration), 8, and K = 2048 at M = 24576; the last tile holds 1, 17, 127 or 128 rows (the second
    wave row may be empty).  Modulation cycles through gstride 0 and rows_per_group 512 (group-uniform), 64 and 250 (two groups per
    tile: the per-row form).  x bit-equal to float64, h within its bound (K_H_INT: measured k 0.54), nt_io 0 = 1 on one K per M."""
    chk = _Checks()
    modes = ["ae", "512", "64", "250"]
    i = [24449, 24465, 24575, 24576].index(M)
    Ks = (64, 128, 192, 512) + ((2048,) if M == 24576 else ())
    for j, K in enumerate(Ks):
        mode = modes[(i + j) % 4]
        _exact_case(H, chk, _case(M, K, mode, 2000 + M + K), f"128 bf16 {M}x{K} {mode}", K_H_INT["128"], nt0=(j == i))
    chk.done()


@gpu
@pytest.mark.parametrize("M,K,mode", [(65, 128, "3"), (1000, 256, "64"), (1000, 2048, "250"), (63, 2048, "ae"), (24448 + 17, 128, "250"),
                                      (24576, 512, "512"), (24449, 512, "ae")])
def test_fused_mx8_operands_exact_integers(H, M, K, mode):
    """The MXFP8-operand kernel (A8 / SA, W8 / SW), 64-row and 128-row forms, group-uniform and per-row modulation, ragged M: e4m3 integers
    in [-4,4] times block scales 2^0..2^3 on both sides, so a wrong scale byte, K-block or row is an exact mismatch.  x bit-equal to float64
    of the dequantised operands (oracle/mx_oracle.dequantize_mx8), h within its bound (K_H_INT: measured k 0.498), nt_io 0 = 1."""
    chk = _Checks()
    _exact_case(H, chk, _case(M, K, mode, 3000 + M + K, kind="mxint"), f"mx {M}x{K} {mode}", K_H_INT["mx"])
    chk.done()


@gpu
@pytest.mark.parametrize("w_rows,M,K", [(128, 1024, 64), (128, 640, 64), (512, 2048, 64), (128, 1000, 64), (128, 24576, 64), (512, 24576, 64),
                                        (128, 1024, 576)])
def test_fused_per_group_weights_exact_integers(H, w_rows, M, K):
    """strideW = 512 K, one distinct integer W per group of w_rows rows, so a tile that multiplies another group's W is an exact mismatch.
    64-row form: w_rows 128 at M = 1024 (8 groups, 2 tiles each: the XCD remap is active), at M = 640 (5 groups: inactive), at M = 1000 (the
    remap active with a ragged last group), w_rows 512 at M = 2048 (8 tiles per group: inactive).  128-row form: w_rows 128 and 512 at
    M = 24576 (192 groups of 1 tile, 48 groups of 4: active).  Modulation per weight group (group-uniform) or per 250 rows.  x bit-equal to float64; h: measured k 0.339 (K_H_INT)."""
    chk = _Checks()
    G = -(-M // w_rows)
    mode = str(w_rows) if M != 640 else "250"
    c = _case(M, K, mode, 4000 + M + w_rows + K, w_groups=G, w_rows=w_rows)
    _exact_case(H, chk, c, f"strideW {w_rows} {M}x{K}", K_H_INT["strideW"], nt0=False)
    chk.done()


@gpu
@pytest.mark.parametrize("kind,M,K,mode", [("rand", 1000, 512, "ae"), ("rand", 1000, 576, "250"), ("mxint", 1000, 256, "64"), ("mxint", 65, 128, "3"),
                                           ("rand", 24448 + 17, 128, "512"), ("rand", 24449, 192, "250"), ("mxint", 24448 + 17, 128, "ae"),
                                           ("mxint", 24448 + 127, 512, "250")])
def test_fused_h8_hs_equals_quantised_h(H, kind, M, K, mode):
    """The quantising LayerNorm epilogue (h8 / hs instead of h) in the bf16 / MXFP8 x 64 / 128-row x group-uniform / per-row forms: the same
    inputs once with h and once with h8 / hs.  x bit-identical between the two; (h8, hs) bit-equal to oracle quantize_mx8 of the bf16 h (the
    kernel quantises the bf16-rounded row).  Columns 32..63 have g = -add_one, b = 0: an exactly zero block, scale byte 0 and zero elements.
    Every M has a ragged last tile (lanes past M take part in the shuffles, and must not store: guard tails).  nt_io 0 = 1 here too."""
    from oracle import mx_oracle as MX
    c = _upload(_case(M, K, mode, 5000 + M + K, kind=kind, zero_block=True))
    a, b = _launch(H, c), _launch(H, c, out="h8")
    assert torch.equal(_bits(a["x"]), _bits(b["x"]))
    assert not bool(torch.isnan(a["h"].float()).any())
    q, s = MX.quantize_mx8(a["h"].float())
    assert torch.equal(b["hs"], s.view(M, 16)), int((b["hs"] != s.view(M, 16)).sum())
    assert torch.equal(b["h8"], q.view(M, 512)), int((b["h8"] != q.view(M, 512)).sum())
    assert bool((b["hs"][:, 1] == 0).all()) and bool((b["h8"][:, 32:64] == 0).all()) and bool((a["h"][:, 32:64] == 0).all())
    assert bool((b["hs"][:, 0] != 0).any())
    assert _same(b, _launch(H, c, out="h8", nt_io=0))


FORMS = [("rand", 1000, 192, "64"), ("rand", 1000, 192, "250"), ("mxint", 1000, 256, "ae"), ("mxint", 1000, 256, "250"),
         ("rand", 24448 + 17, 192, "512"), ("rand", 24448 + 17, 192, "250"), ("mxint", 24448 + 17, 256, "ae"), ("mxint", 24448 + 17, 256, "64")]


@gpu
@pytest.mark.parametrize("kind,M,K,mode", FORMS)
def test_fused_results_do_not_depend_on_stale_lds(H, kind, M, K, mode):
    """The epilogue reuses the staging buffers (transpose patches, row sums, bias | g | b): one case per compiled form (64 / 128 rows x bf16
    / MXFP8 x group-uniform / per-row), h and h8 / hs, run, then rald_debug_poison_lds, then run again: bit-identical."""
    from rald_amd._lib import check, lib
    c = _upload(_case(M, K, mode, 6000 + M + K, kind=kind))
    for out in ("h", "h8"):
        a = _launch(H, c, out=out)
        check(lib().rald_debug_poison_lds(torch.cuda.current_stream().cuda_stream))
        assert _same(a, _launch(H, c, out=out)), out


# ---- fused kernel, random data ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M,K,mode,kx,kh", [(1000, 64, "64", 4.5, 3.7), (1000, 448, "250", 4.2, 4.6), (1000, 512, "ae", 24, 6.5),
                                            (1000, 576, "512", 26, 8.8), (1000, 2048, "64", 41, 16), (65, 512, "3", 22, 1.25),
                                            (24448 + 17, 64, "250", 4.4, 5.4), (24449, 128, "512", 4.3, 4.9), (24448 + 127, 192, "64", 4.7, 4.9),
                                            (24576, 512, "ae", 4.7, 5.8), (24448 + 17, 2048, "512", 5.6, 18)])
def test_fused_bf16_random_per_element_bounds(H, M, K, mode, kx, kh):
    """The fused kernel on bf16 operands of unit scale (W / sqrt(K)), x_old = 0.5 + 2 randn, and every fourth row x_old = 16 s + s randn
    (s in {0.5, 1, 2}: |mean| / std of the row up to 16, which exercises the single-pass variance term of T).  Both tile heights, every nk
    regime, all modulation forms.  Measured k (x, h) in the order of the parameters: (1.83, 1.5), (1.69, 1.87), (9.64, 2.61), (10.5, 3.52),
    (16.4, 6.42), (8.83, 0.503), (1.79, 2.18), (1.74, 1.96), (1.89, 1.98), (1.91, 2.34), (2.24, 7.33).  (From nk = 8 on the 64-row form adds
    x_old to the accumulators during the first k-steps, so the later k-steps round at the magnitude of x_old: k for x grows with nk there;
    the 128-row form adds it in the epilogue.)"""
    chk = _Checks()
    c = _upload(_case(M, K, mode, 7000 + M + K, kind="rand"))
    ref = _reference(c)
    r = _launch(H, c)
    chk.le(f"fused {M}x{K} {mode} x", _ratio(r["x"], ref["v"], ref["tx"]), kx)
    chk.le(f"fused {M}x{K} {mode} h", _ratio16(r["h"], ref["h"], ref["T"]), kh)
    chk.done()


# ---- the dispatcher --------------------------------------------------------------------------------------------------------------------
def _mx8_dequant_ratio(h8, hs, href, T, kh):
    """h8 / hs of a kernel that quantises its fp32 value (layernorm_mod_mx8): scale byte sb must be the smallest with amax / 2^(sb-127) <= 448
    for an amax within the fp32 bound e = kh 2^-24 T of the float64 one, and every element within e + half an e4m3 ulp (at the magnitude
    |ref| + e under that scale; 2^-9 scale below 2^-6 scale) of the float64 value.  Returns (scale violations, worst error / allowance)."""
    from oracle import mx_oracle as MX
    S = torch.exp2(hs.double() - 127.0)                                                   # [M, 16]
    e = (kh * U * T).view(-1, 16, 32)
    ref = href.view(-1, 16, 32)
    lo, hi = (ref.abs() - e).clamp_min(0).amax(-1), (ref.abs() + e).amax(-1)
    bad = (lo > 448 * S) | ((hs > 0) & (hi < 224 * S))
    y = (ref.abs() + e) / S[..., None]
    ulp = torch.exp2(torch.floor(torch.log2(y.clamp_min(2.0 ** -6))) - 3)
    allow = e + 0.5 * ulp * S[..., None]
    got = MX.dequantize_mx8(h8, hs).double().view(-1, 16, 32)
    return int(bad.sum()), float(((got - ref).abs() / allow).max())


@gpu
@pytest.mark.parametrize("name,M,K,mode,slab16,kx,kh", [
    ("fp16 slabs, 64x64 ring", 512, 2048, "ae", True, 0, 0),
    ("fp32 slabs", 1000, 2048, "250", False, 5.6, 1.15),
    ("fp16 slabs, 128x128", 1600, 2048, "512", True, 0, 0),
    ("fp16 slabs, 128x128, M = 4096", 4096, 2048, "512", True, 0, 0),
    ("gemm_nt + LayerNorm, M = 4097", 4097, 2048, "512", False, 4, K_H_UNFUSED_2048),
    ("unfused, M = 16383", 16383, 512, "512", False, 5.3, 3.5),
    ("fused, M = 16384", 16384, 512, "512", False, 30, 14),
    ("no LayerNorm, split-K", 512, 2048, None, True, 0, None),
    ("no LayerNorm, gemm_nt", 4097, 2048, None, False, 4, None),
    ("h8 / hs: gemm_nt + layernorm_mod_mx8", 1024, 2048, "512", False, 4.2, K_H_UNFUSED_2048)])
def test_dispatcher_routes_per_element(H, name, M, K, mode, slab16, kx, kh):
    """resid_gemm_ln(a, 512, scratch) as the models call it, random bf16 data as in the fused test, each route against float64 on its own
    (M = 16383 and 16384 are not compared with each other: DESIGN section 14).  Through fp16 slabs x may additionally differ by
    sum_s 2^-11 |partial_s| (the float64 partial product of each of the 4 K-ranges: the fp16 rounding of the 2^-6-scaled slabs), and the
    saturation counter must read 0.  Without g / b x is updated and h keeps its NaN fill.  With h8 / hs the LayerNorm is
    layernorm_mod_mx8, which quantises its fp32 value: checked by _mx8_dequant_ratio with the fp32 allowance of the bf16 LayerNorm behind the
    same GEMM (K_H_UNFUSED_2048: the same two-pass arithmetic on the same x), no constant of its own.  Measured k (x, h) in the order of
    the parameters: (0, 0), (2.24, 0.463), (0, 0), (0, 0), (1.62, 2.19), (2.14, 1.43), (12, 5.96), (0, -), (1.62, -), (1.7, -); through fp16
    slabs the slab allowance alone covers the whole error, so k = 0 there.  M = 16384 runs the 64-row fused form (see the fused test for its k)."""
    from rald_amd._lib import lib
    chk = _Checks()
    c = _upload(_case(M, K, mode or "512", 8000 + M + K, kind="rand"))
    ref = _reference(c, kparts=4 if slab16 else 1)
    assert lib().rald_debug_f16_saturation_count(1) >= 0
    h8 = name.startswith("h8")
    r = _launch(H, c, route=0, out="h8" if h8 else "h", ln=mode is not None)
    chk.true("fp16 slab saturation", lib().rald_debug_f16_saturation_count(1) == 0)
    extra = sum(p.abs() for p in ref["parts"]) * 2.0 ** -11 if slab16 else None
    chk.le(f"route 0 {name} x", _ratio(r["x"], ref["v"], ref["tx"], extra), kx)
    if mode is None:
        chk.true("h untouched", torch.equal(_bits(r["h"]), _bits(torch.full_like(r["h"], float("nan")))))
    elif h8:
        nbad, worst = _mx8_dequant_ratio(r["h8"], r["hs"], ref["h"], ref["T"], kh)
        chk.true(f"scale bytes ({nbad} outside their range)", nbad == 0)
        chk.le(f"route 0 {name} h8 error / allowance", worst, 1.0)
    else:
        # through fp16 slabs every v_j is off by up to d = max_j of the slab allowance: v_j - mean moves by <= 2 d, var by <= 2 std d, so
        # rstd by <= rstd^2 d relative to itself: |dh| <= rstd |add_one + g| d (2 + |v - mean| rstd)
        hx = None
        if slab16:
            m = c["m"]
            grp = torch.arange(M) // m["rpg"] if m["gstride"] else torch.zeros(M, dtype=torch.long)
            dv = ref["v"] - ref["v"].mean(1, keepdim=True)
            rstd = ((dv ** 2).mean(1, keepdim=True) + EPS).rsqrt()
            hx = rstd * (m["add_one"] + m["mod"][grp, :512].double()).abs() * extra.amax(1, keepdim=True) * (2 + dv.abs() * rstd)
        chk.le(f"route 0 {name} h", _ratio16(r["h"], ref["h"], ref["T"], hx), kh)
    chk.done()


@gpu
def test_dispatcher_per_group_weights_exact_integers(H):
    """route 0 with strideW at M = 1024, w_rows = 128, K = 2048: gemm_nt batched over the 8 weight groups + LayerNorm; integer data, x
    bit-equal to float64, h within its bound (K_H_INT: measured k 0.241)."""
    chk = _Checks()
    c = _upload(_case(1024, 2048, "128", 8800, w_groups=8, w_rows=128))
    ref = _reference(c)
    r = _launch(H, c, route=0)
    chk.true("x exact", torch.equal(r["x"].double(), ref["v"]))
    chk.le("route 0 strideW h", _ratio16(r["h"], ref["h"], ref["T"]), K_H_INT["route0"])
    chk.done()


# ---- GEGLU -----------------------------------------------------------------------------------------------------------------------------
def _geglu_pack(W, bias):
    """rows of [x half | gate half] -> the packed order of the GEGLU epilogue (16 x rows, then their 16 gate rows)"""
    inner = W.shape[0] // 2
    c = torch.arange(inner)
    rowmap = torch.cat([32 * (c // 16) + c % 16, 32 * (c // 16) + 16 + c % 16])
    Wp, bp = torch.empty_like(W), torch.empty_like(bias)
    Wp[rowmap], bp[rowmap] = W, bias
    return Wp, bp


def _geglu_ref(A, W, bias):
    """float64 (x + b_x) gelu_erf(g + b_g), the fp32 terms of its bound, and |x + b_x| (device matmul, the rest on the CPU)"""
    inner = W.shape[0] // 2
    Ad, Wd = A.cuda().double(), W.cuda().double()
    y = (Ad @ Wd.t()).cpu() + bias.double()
    ty = (Ad.abs() @ Wd.abs().t()).cpu() + bias.double().abs()
    xv, gv = y[:, :inner], y[:, inner:]
    Phi = 0.5 * (1 + torch.erf(gv / math.sqrt(2.0)))
    gelu = gv * Phi
    dgelu = Phi + gv * torch.exp(-0.5 * gv * gv) / math.sqrt(2 * math.pi)
    ref = xv * gelu
    terms = ty[:, :inner] * gelu.abs() + xv.abs() * (ty[:, inner:] * dgelu.abs() + gelu.abs())
    return ref, terms, xv.abs()


GELU_POLY_ABS = 4.5e-5                        # gelu_poly2's documented absolute error (common.h)


@gpu
def test_geglu_128x128_per_element(H):
    """EPI_GEGLU on the 128x128 engine: M = 3000 (24 x 8 = 192 tiles of 128x128, M % 256 != 0), 1024 packed rows -> 512 columns, K = 192.
    Per element: one bf16 ulp + |x + b_x| 4.5e-5 (gelu_poly2 against erf GELU) + k 2^-24 terms.  Measured k: 0.154."""
    chk = _Checks()
    M, N, K = 3000, 1024, 192
    g = _g(9000)
    A = torch.randn(M, K, generator=g).bfloat16().float()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().float()
    bias = torch.randn(N, generator=g) * 0.1
    Wp, bp = _geglu_pack(W, bias)
    out = _guarded(M * 512, 1024, torch.bfloat16)
    H.op_gemm_geglu_mx8out(bp.cuda(), M, N, K, A=A.cuda().bfloat16(), W=Wp.cuda().bfloat16(), out=out[:M * 512].view(M, 512))
    torch.cuda.synchronize()
    assert _guard_ok(out, M * 512)
    ref, terms, ax = _geglu_ref(A, W, bias)
    chk.le("geglu 128x128", _ratio16(out[:M * 512].view(M, 512).cpu(), ref, terms, ax * GELU_POLY_ABS), K_GEGLU_128)
    chk.done()


@gpu
@pytest.mark.parametrize("mx,K", [(False, 64), (True, 128)])
def test_geglu_256x256_mx8_output_equals_quantised_bf16_output(H, mx, K):
    """EPI_GEGLU on the 256x256 engine at M = 4096, N = 4096 (256 tiles) with out8 / outs set, from bf16 operands (gemm_nt, K = 64) and
    from MXFP8 operands (gemm_mx8, K = 128: its k-step).  The call with out8 / outs must equal oracle quantize_mx8 of the bf16 output
    of the same call without them, bit for bit, and the bf16 output is within the GEGLU bound.  Measured k: 0.121 (bf16), 288 (MXFP8: see
    K_GEGLU_256)."""
    from oracle import mx_oracle as MX
    chk = _Checks()
    M, N = 4096, 4096
    g = _g(9100 + K)
    A = torch.randn(M, K, generator=g).bfloat16().float()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().float()
    bias = torch.randn(N, generator=g) * 0.1
    if mx:
        (A8, SA), (W8, SW) = MX.quantize_mx8(A), MX.quantize_mx8(W)
        A, W = MX.dequantize_mx8(A8, SA), MX.dequantize_mx8(W8, SW)
    Wp, bp = _geglu_pack(W, bias)
    if mx:
        W8p, SWp = MX.quantize_mx8(Wp)                                                    # per row: the packed rows' bytes
        assert torch.equal(MX.dequantize_mx8(W8p, SWp), Wp)
        ops = dict(A8=A8.cuda(), SA=SA.cuda(), W8=W8p.cuda(), SW=SWp.cuda())
    else:
        ops = dict(A=A.cuda().bfloat16(), W=Wp.cuda().bfloat16())
    n = M * (N // 2)
    out, out8, outs = _guarded(n, 4096, torch.bfloat16), _guarded(n, 4096, torch.uint8, 0x7F), _guarded(n // 32, 256, torch.uint8, 0xFF)
    H.op_gemm_geglu_mx8out(bp.cuda(), M, N, K, out=out[:n].view(M, N // 2), **ops)
    H.op_gemm_geglu_mx8out(bp.cuda(), M, N, K, out8=out8[:n].view(M, N // 2), outs=outs[:n // 32].view(M, N // 64), **ops)
    torch.cuda.synchronize()
    assert _guard_ok(out, n) and _guard_ok(out8, n) and _guard_ok(outs, n // 32)
    o = out[:n].view(M, N // 2).cpu()
    q, s = MX.quantize_mx8(o.float())
    chk.true("outs == quantize_mx8(out)", torch.equal(outs[:n // 32].view(M, N // 64).cpu(), s))
    chk.true("out8 == quantize_mx8(out)", torch.equal(out8[:n].view(M, N // 2).cpu(), q))
    ref, terms, ax = _geglu_ref(A, W, bias)
    chk.le(f"geglu 256x256 {'mx8' if mx else 'bf16'}", _ratio16(o, ref, terms, ax * GELU_POLY_ABS), K_GEGLU_256[mx])
    chk.done()


# bounds of the checks that share one constant (measured on an MI355X; bound <= 2.5 x the worst measured value, rounded up)


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


def test_argument_checks_refuse_before_any_launch(L_cpu):
    """rald_op_resid_gemm_ln and rald_op_gemm_geglu_mx8out on fake aligned pointers (the checks are numeric): each refusal names its
    constraint, on the fused route (1) and, where the dispatcher has the same or its own rule, on route 0."""
    L, d = L_cpu, DUMMY

    def call(route=1, mx=False, M=1024, K=512, lda=None, ldw=None, x=d, h=d, h8=None, hs=None, g=d, b=d, strideW=0, w_rows=0, scratch=None,
             scratch_bytes=0, rpg=512):
        lda, ldw = K if lda is None else lda, K if ldw is None else ldw
        ops = (None, d, d, lda, None, d, d, ldw) if mx else (d, None, None, lda, d, None, None, ldw)
        return L.rald_op_resid_gemm_ln(*ops, strideW, w_rows, d, x, h, h8, hs, g, b, 1024, rpg, 1.0, 1e-5, M, K, 1, route, scratch, scratch_bytes, None)

    for route in (0, 1):
        big = dict(M=16384) if route == 0 else {}                     # (route 0 reaches the fused kernel from M = 16384)
        _refused(L, call(route, K=96, lda=96, ldw=96, **big), "bad shape" if route else "K and the leading dimensions")
        _refused(L, call(route, mx=True, K=192, lda=192, ldw=192, **big), "bad shape" if route else "K and the leading dimensions")
        _refused(L, call(route, lda=520, **big), "leading dimensions")
        _refused(L, call(route, x=d + 4), "16-byte alignment")
        _refused(L, call(route, h=None), "h or h8")
        _refused(L, call(route, h=None, h8=d), "h8 and hs")
        _refused(L, call(route, mx=True, strideW=512 * 512, w_rows=128, **big), "per-group weights", "bf16")
        _refused(L, call(route, strideW=512 * 512, w_rows=192, M=16512), "per-group weights", "128")
        _refused(L, call(route, mx=True, M=1 << 25, K=2048), "scale index overflow")
        _refused(L, call(route, strideW=512 * 512, w_rows=0), "w_rows")
    _refused(L, call(0, strideW=512 * 512, w_rows=128, M=1000), "multiple of w_rows")
    _refused(L, call(0, strideW=512 * 512, w_rows=128, M=16384 + 64), "multiple of w_rows")
    need = 4 * 1000 * 512 * 4
    _refused(L, call(0, M=1000, K=2048, scratch=d, scratch_bytes=need - 4), "scratch too small")
    _refused(L, call(0, M=1000, K=2048, scratch=None, scratch_bytes=need), "scratch")
    _refused(L, call(0, M=4096, K=2048, scratch=d, scratch_bytes=4 * 4096 * 512 * 4 - 4), "scratch too small")
    _refused(L, call(1, g=None, b=None), "without a LayerNorm")
    _refused(L, call(2), "route")
    _refused(L, call(1, rpg=0), "bad shape")
    # the GEGLU entry: one operand form, one output form, and the engines' own shape rules
    ge = L.rald_op_gemm_geglu_mx8out
    _refused(L, ge(d, d, d, 64, d, None, None, 64, d, d, None, None, 2048, 4096, 4096, 64, None), "not both")
    _refused(L, ge(d, None, None, 64, d, None, None, 64, d, d, d, d, 2048, 4096, 4096, 64, None), "not both")
    _refused(L, ge(d, None, None, 64, d, None, None, 64, d, None, d, None, 2048, 4096, 4096, 64, None), "out8 and outs")
    _refused(L, ge(d, None, None, 64, d, None, None, 64, None, d, None, None, 2048, 4096, 4096, 64, None), "null bias")
    _refused(L, ge(d, None, None, 64, d, None, None, 64, d, None, d, d, 2048, 3840, 4096, 64, None), "full 256x256 tiles")
    _refused(L, ge(None, d, d, 128, None, d, d, 128, d, None, d, d, 2048, 3840, 4096, 128, None), "full 256x256 tiles")
    _refused(L, ge(None, d, d, 192, None, d, d, 192, d, d, None, None, 2048, 4096, 4096, 192, None), "multiple of 128")
