"""The streaming query decoder (rald_amd/csrc/ae_decode.hip) through its op entry rald_op_ae_decode, per query, against float64.

Two references, both on the CPU, both from the fp32 values handed to the entry, widened exactly; neither rounds anything to fp16 nor
imitates the kernel's order of operations:

  model reference    oracle.rald_oracle.ae_decode_queries on a float64 state dict (PointEmbed -> LN -> to_q; LN_ctx -> to_kv; softmax;
                     to_out; to_outputs), used with the real tables rald_op_ae_decode_tables makes of that state dict
  formula reference  what the entry is defined to compute from ARBITRARY tables (the per-query lines of test_decode_fold.py):
                         Y = LN_ctx(x) . t2aug          H = Y[:, feature slots], h0 = Y[:, 51], hb = Y[:, 53], u = Y[:, 63]
                         var = |L.[f;1]|^2              L read back from the fp16 image exactly
                         S_l = rstd (f.H_l + h0_l) + hb_l               (log2 units)
                         logit = softmax2(S) . u + c0
                     used where a test crafts t2aug / l_img / x to force an edge.  test_decode_fold.py pins its equivalence to the model;
                     test_references_agree_on_real_tables below repeats that for the functions of this file.

Error unit.  Per query |got - ref| <= k * 2^-11 * T_q.  If every score moves by at most d (log2 units), each softmax weight moves by a
factor within 2^(+-2d) (numerator and denominator), so the weighted mean of u moves by at most (2^(2d) - 1) max_l |u_l - mean|
~ 2 ln2 d max_l |u_l - mean|.  Score l is a sum of products of fp16 operands (11-bit significands): rounding the features and the
coefficients perturbs it by about 2^-11 rstd_q (sum_k |f_k| |H_lk| + |h0_l|) (h0 and hb are carried in hi + lo pairs, their share is far
smaller but is charged at the same rate), the fp16 variance factor and the hardware rsqrt move rstd_q by a relative 2^-11-ish, v_sin and
v_exp add a few fp32 ulps.  The fp16 image also has an absolute floor: with the sample's largest coefficient mx scaled into
[2^13, 2^14), fp16's smallest step 2^-24 is g = 2^(floor(log2 mx) - 37) in the coefficients' own units; entries below 2^-27 mx keep
fewer than 11 bits and are charged g each: rstd_q g (sum_k |f_k| + 2) + 2 g per score (two slots each for h0 and hb).  So with

    A_q = max_l( rstd_q (sum_k |f_k| |H_lk| + |h0_l|) + |hb_l| )  +  2^11 g (rstd_q (sum_k |f_k| + 2) + 2)
    T_q = ln2 * A_q * max_l |u_l - (ref_q - c0)|  +  |ref_q|

k counts the roundings: the derivation says a small number.  Not charged: the fp32 projection Y (2^-24 sum_c |LN(x)_c| |t2aug_ck|, 2^-13
of the fp16 term on real tables) and fp32 accumulation.  Every element of every output is compared; NaN counts as infinite error.
Each test prints its measured k ("ratio"); every bound is at most 2.5 times the worst k measured on an MI355X (docstrings).

Output buffers start as NaN and are followed by 64 sentinel floats that must survive bit for bit; the queries sit in an allocation whose
tail is NaN.  B >= 3 with distinct samples wherever B is not the subject.  The unmarked tests at the end run without a GPU: they keep
the crafted inputs honest (references agree, T_q finite and positive, the exact-LayerNorm rows are exact) and check the refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2
from oracle import rald_oracle as O
from rald_amd import synth, weights
from test_gpu_train_ops import DUMMY, L_cpu, _guard_ok, _guarded, _le, _refused  # noqa: F401  (L_cpu is a fixture)

gpu = pytest.mark.gpu
U16 = 2.0 ** -11
SLOT_ONE, SLOT_STD, SLOT_U = 51, 53, 63


# ---- tables, features, references ---------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _img_off(row, k):
    return row * 128 + (((k >> 3) ^ (row & 7)) << 4) + (k & 7) * 2


def _slot(f):
    if f < 24:
        return 16 * (f >> 3) + (f & 7)
    if f < 48:
        e = f - 24
        return 16 * (e >> 3) + 8 + (e & 7)
    return 48 + (f - 48)


_IMG_INDEX = np.array([[_img_off(i, k) // 2 for k in range(64)] for i in range(64)])


def _L_of(limg):
    """the [64][64] factor of the fp16 image (int16 bits), widened exactly"""
    return torch.from_numpy(limg.numpy().view(np.float16)[_IMG_INDEX].astype(np.float64))


def _limg_of(Lm):
    """fp16 image (int16 bits) of a [64][64] factor whose entries are fp16 numbers"""
    img = np.zeros(64 * 64, np.float16)
    img[_IMG_INDEX] = Lm.astype(np.float16)
    return torch.from_numpy(img.view(np.int16).copy())


def _sd(dim, M, kind="plain", basis=None):
    """decoder weights of the synthetic autoencoder (no latent stack: depth 0); 'peaked' = weights.stress_ae_state_dict"""
    sd = weights.make_state_dict(weights.ae_spec(dim=dim, num_latents=M, depth=0), seed=0)
    if kind == "peaked":
        sd = weights.stress_ae_state_dict(sd)
    if basis is not None:
        sd["point_embed.basis"] = basis.clone()
    return sd


def _tables(sd, d):
    """(t2aug fp32 [d,64], l_img int16 [4096], c0) as Ae::finalize makes them: rald_op_ae_decode_tables, on the host"""
    from rald_amd import _lib
    f32 = lambda t: np.ascontiguousarray(t.detach().numpy().astype(np.float32))
    wq = f32(sd["decoder_cross_attn.fn.to_q.weight"])
    wkv = f32(sd["decoder_cross_attn.fn.to_kv.weight"])
    wo, bo = sd["decoder_cross_attn.fn.to_out.weight"].double(), sd["decoder_cross_attn.fn.to_out.bias"].double()
    w_out, b_out = sd["to_outputs.weight"].double()[0], sd["to_outputs.bias"].double()[0]
    wfold = (wkv[d:].astype(np.float64).T @ (wo.T @ w_out).numpy()).astype(np.float32)
    c0 = float(np.float32(float(bo @ w_out + b_out)))
    ng, nb = f32(sd["decoder_cross_attn.norm.weight"]), f32(sd["decoder_cross_attn.norm.bias"])
    wpe, bpe = f32(sd["point_embed.mlp.weight"]), f32(sd["point_embed.mlp.bias"])
    t2 = np.zeros((d, 64), np.float32)
    limg = np.zeros(64 * 64, np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().rald_op_ae_decode_tables(d, p(wq), p(np.ascontiguousarray(wkv[:d])), p(ng), p(nb), p(wpe), p(bpe), p(wfold), p(t2), p(limg))
    assert rc == 0
    return torch.from_numpy(t2), torch.from_numpy(limg.view(np.int16).copy()), c0


def _features(q, basis):
    """[Q,3] float64 -> [Q,64] in slot order, 1 in SLOT_ONE (reference feature order: sin, cos, xyz)"""
    proj = q @ basis
    feat = torch.cat([proj.sin(), proj.cos(), q], dim=1)
    Fm = torch.zeros(q.shape[0], 64, dtype=torch.float64)
    Fm[:, [_slot(f) for f in range(51)]] = feat
    Fm[:, SLOT_ONE] = 1.0
    return Fm


def _context(case):
    """Y = LN_ctx(x) . t2aug in float64 [B,M,64]"""
    x = case["x"].double()
    dv = x - x.mean(-1, keepdim=True)                            # written out: the mean of integers that sum to zero is exactly zero
    xn = dv / (dv ** 2).mean(-1, keepdim=True).add(1e-5).sqrt() * case["gamma"].double() + case["beta"].double()
    return xn @ case["t2"].double()


def _scores(case, Yb, q):
    """(S [Q,M] in log2 units, rstd [Q], features [Q,64]) of the queries q [Q,3] on one sample's Y"""
    Fm = _features(q.double(), case["basis"].double())
    rstd = ((Fm @ _L_of(case["limg"]).t()) ** 2).sum(1).add(1e-5).rsqrt()
    return rstd[:, None] * (Fm[:, :51] @ Yb[:, :51].t() + Yb[:, SLOT_ONE]) + Yb[:, SLOT_STD], rstd, Fm


def _formula(case, ref=None, block=8192):
    """(formula reference [B,Q], T [B,Q]) in float64; T is taken around `ref` when one is given (the model reference)"""
    Y, q, c0 = _context(case), case["q"], case["c0"]
    B, Q = q.shape[:2]
    out, T = torch.zeros(B, Q, dtype=torch.float64), torch.zeros(B, Q, dtype=torch.float64)
    coef = list(range(52)) + [SLOT_STD]                          # the columns whose largest |entry| sets the sample's scale
    for b in range(B):
        H, h0, hb, u = Y[b][:, :51], Y[b][:, SLOT_ONE], Y[b][:, SLOT_STD], Y[b][:, SLOT_U]
        mx = float(Y[b][:, coef].abs().max())
        g = 2.0 ** (math.floor(math.log2(mx)) - 37) if mx > 0 else 0.0
        for s in range(0, Q, block):
            S, rstd, Fm = _scores(case, Y[b], q[b, s:s + block])
            P = torch.exp2(S - S.max(1, keepdim=True).values)
            o = (P * u).sum(1) / P.sum(1) + c0
            fa = Fm[:, :51].abs()
            A = (rstd[:, None] * (fa @ H.abs().t() + h0.abs()) + hb.abs()).max(1).values
            A = A + 2.0 ** 11 * g * (rstd * (fa.sum(1) + 2) + 2)
            r = o if ref is None else ref[b, s:s + block]
            out[b, s:s + block] = o
            T[b, s:s + block] = math.log(2) * A * (u[None] - (r - c0)[:, None]).abs().max(1).values + r.abs()
    return out, T


def _model_ref(sd, case, block=8192):
    """KLAutoEncoder.decode's query half as the reference model writes it, in float64"""
    sd64 = {k: v.double() for k, v in sd.items()}
    x, q = case["x"].double(), case["q"].double()
    with torch.no_grad():
        return torch.cat([O.ae_decode_queries(sd64, x, q[:, s:s + block]).squeeze(-1) for s in range(0, q.shape[1], block)], dim=1)


def _k(got, ref, T):
    err = (got.detach().cpu().double() - ref).abs()
    r = err / (U16 * T)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


def _run(case, Q=None, rows=None):
    """the entry on the first Q queries (of the samples `rows`): queries before a NaN tail, output pre-filled with NaN before 64 sentinels"""
    from rald_amd import _handles as Hd
    sel = slice(None) if rows is None else rows
    x, q = case["x"][sel], case["q"][sel]
    q = q if Q is None else q[:, :Q]
    B, Q = q.shape[:2]
    qbuf = torch.full((B * Q * 3 + 192,), float("nan"), device="cuda")
    qbuf[:B * Q * 3] = q.reshape(-1).cuda()
    out = _guarded(B * Q, 64)
    dev = lambda t: t.contiguous().cuda()
    Hd.op_ae_decode(dev(x), dev(case["gamma"]), dev(case["beta"]), dev(case["t2"]), dev(case["limg"]), dev(case["basis"]), case["c0"],
                    qbuf[:B * Q * 3].view(B, Q, 3), out=out[:B * Q])
    torch.cuda.synchronize()
    assert _guard_ok(out, B * Q), "the decoder wrote past its output"
    return out[:B * Q].view(B, Q).cpu()


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _queries(B, Q, seed, lim=1.0):
    return (torch.rand(B, Q, 3, generator=_g(seed), dtype=torch.float64) * 2 - 1).mul(lim).float()


def _real_case(dim, M, B, Q, kind="plain", basis=None, seed=1, lim=1.0):
    """real tables of the synthetic decoder weights; x random with a different offset and spread per sample"""
    sd = _sd(dim, M, kind, basis)
    t2, limg, c0 = _tables(sd, dim)
    g = _g(1000 * seed + M + dim)
    x = torch.randn(B, M, dim, generator=g) * (0.5 + torch.rand(B, 1, 1, generator=g) * 2) + torch.randn(B, 1, dim, generator=g) * 0.3
    case = dict(x=x, gamma=sd["decoder_cross_attn.norm_context.weight"].clone(), beta=sd["decoder_cross_attn.norm_context.bias"].clone(),
                t2=t2, limg=limg, basis=sd["point_embed.basis"].clone(), c0=c0, q=_queries(B, Q, seed + 50, lim))
    return sd, case


def _rotated_basis(kind):
    """'dense': the shipped basis turned by a fixed, seeded rotation of the coordinates (every entry non-zero); 'off_block': the shipped
    basis with one small entry outside its blocks"""
    b = weights.point_embed_basis().clone()
    if kind == "dense":
        R, _ = torch.linalg.qr(torch.randn(3, 3, generator=_g(77), dtype=torch.float64))
        return (R @ b.double()).float()
    b[2, 3] = 0.37
    return b


def _block_case(scales, big_latent=None, M=64, Q=1024, target=6.0, seed=3, zero=False):
    """Per-sample (or per-latent) coefficient scales under real l_img / basis, dim 256.  LayerNorm undoes any scale of x, so the scale
    sits in t2aug: its rows are cut into blocks of 64 channels, the coefficient columns of block j are times scales[j], and a latent row
    of x lives in ONE block (small integers summing to zero there, exact zeros elsewhere: the mean is exactly zero, so LN(x) is exactly
    zero outside the block in fp32 as in float64).  Sample b uses block b; with big_latent, every sample uses block 0 except that latent,
    which uses block 1.  The u column is never scaled.  The unscaled table is normalised (by a power of two, from the float64 formula) so
    that the median over sample 0's queries of max_l |S_l| is about `target`."""
    dim, B = 256, (3 if big_latent is not None else len(scales))
    sd = _sd(dim, 128)
    _, limg, c0 = _tables(sd, dim)
    g = _g(seed)
    half = torch.randint(-3, 4, (B, M, 32), generator=g).float()
    x = torch.zeros(B, M, dim)
    for b in range(B):
        for l in range(M):
            blk = b if big_latent is None else (1 if l == big_latent[b] else 0)
            x[b, l, 64 * blk:64 * blk + 32] = half[b, l]
            x[b, l, 64 * blk + 32:64 * blk + 64] = -half[b, l].flip(0)
    base = torch.randn(dim, 64, generator=g)
    case = dict(x=x, gamma=torch.ones(dim), beta=torch.zeros(dim), t2=base.clone(), limg=limg, basis=weights.point_embed_basis(), c0=c0,
                q=_queries(B, Q, seed + 9))
    size = float(_scores(case, _context(case)[0], case["q"][0])[0].abs().max(1).values.median())
    norm = 2.0 ** round(math.log2(target / size))
    t2 = base.clone()
    for j in range(4):
        t2[64 * j:64 * j + 64, :SLOT_U] *= norm * scales[j] if j < len(scales) else 0.0
    if zero:
        t2[:, :SLOT_U] = 0
    case["t2"] = t2
    return case


# exact LayerNorm: a row of 256 multiples of 2^-7 with sum 0 and sum of squares LN_N * 2^-14 has mean 0 and, in fp32,
# mean square + 1e-5f == 4.0f exactly, so rstd = 0.5 and with gamma = 2, beta = 0 LN(x) = x bit for bit (every partial sum is exact)
LN_G, LN_N = 2.0 ** -7, 16777174


def _three_squares(n):
    a = math.isqrt(n)
    while a >= 0:
        r = n - a * a
        b = math.isqrt(r)
        while b >= 0 and b * b * 2 >= r:
            c = math.isqrt(r - b * b)
            if c * c == r - b * b:
                return [a, b, c]
            b -= 1
        a -= 1
    return None


def _exact_rows(design):
    """design [M,256] float64, multiples of 2^-7, channels 200.. unused -> fp32 rows with the property above (the balance lives in 200..)"""
    M = design.shape[0]
    x = design.clone()
    for l in range(M):
        m = (design[l] / LN_G).round().long()
        assert torch.equal(m.double() * LN_G, design[l]) and int(m[200:].abs().sum()) == 0
        s1 = int(m.sum())
        vals = [-(s1 // 8)] * 7 + [-(s1 - 7 * (s1 // 8))]           # the designed entries' sum, undone in eight parts
        rest = LN_N - int((m * m).sum()) - sum(v * v for v in vals)
        assert rest >= 0 and rest % 2 == 0, (l, rest)
        half = rest // 2
        big = 1024                                                   # pairs of +-8.0
        while half >= 2 * big * big:
            vals += [big, -big]
            half -= big * big
        v1 = math.isqrt(half)
        while True:
            three = _three_squares(half - v1 * v1)
            if three is not None:
                break
            v1 -= 1
        for v in [v1] + three:
            vals += [v, -v]
        assert len(vals) <= 56
        x[l, 200:200 + len(vals)] = torch.tensor(vals, dtype=torch.float64) * LN_G
    return x.float()


def _one_slot_limg():
    """variance factor with the single entry L[0][SLOT_ONE] = 1: var_q = 1 for every query"""
    Lm = np.zeros((64, 64))
    Lm[0, SLOT_ONE] = 1.0
    return _limg_of(Lm)


def _onehot_case(M, Q=1500, seed=5):
    """Softmax numerically one-hot on a latent that depends on the query, exact arithmetic up to the softmax.  Latent l owns a grid point
    p_l of nx x 4 x 4 points in (-1,1)^3 (a seeded permutation of the latents over the grid); H_l = 2c p_l on the x, y, z slots, hb_l =
    -c |p_l|^2, everything else zero, so S_l(q) = c |q|^2 - c |q - p_l|^2 (rstd_q = 1 to 5e-6): the nearest grid point wins by c * spacing^2 >= 512 log2
    units over every other latent, and the queries are grid points (exact in fp16).  u_l = +-2^j, all distinct: with the lazily moved maximum
    the surviving weight p is not exactly 1, and fl(fl(p u) / p) = u for every p only when u is a power of two.  LN(x) = x exactly
    (_exact_rows) and t2aug has one non-zero per used channel, so H, hb, u reach the kernel exactly as designed."""
    nx = M // 16
    c = 2.0 ** 13
    gx = (torch.arange(nx, dtype=torch.float64) * 2 + 1) / nx - 1                  # odd multiples of 1/nx
    gy = torch.tensor([-0.75, -0.25, 0.25, 0.75], dtype=torch.float64)
    grid = torch.stack(torch.meshgrid(gx, gy, gy, indexing="ij"), -1).reshape(M, 3)
    perm = torch.randperm(M, generator=_g(seed))
    p = grid[perm]                                                                # p[l] = grid point of latent l
    # +-2^j, j = 0 .. M/2 - 1, handed to the latents in a seeded order
    order = torch.randperm(M, generator=_g(seed + 2))
    u = torch.empty(M, dtype=torch.float64)
    u[order] = torch.exp2((torch.arange(M) // 2).double()) * torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0).double()
    design = torch.zeros(M, 256, dtype=torch.float64)
    t2 = torch.zeros(256, 64)
    # channels 0..2: 8 p_l (integers up to 7), channel 3: -8 |p_l|^2 (multiples of 1/8); t2aug turns them into 2c p_l and -c |p_l|^2
    design[:, 0:3] = p * 8
    design[:, 3] = -(p ** 2).sum(1) * 8
    for a in range(3):
        t2[a, 48 + a] = 2 * c / 8
    t2[3, SLOT_STD] = c / 8
    for l in range(M):                                                            # channel 4 + l carries u_l
        design[l, 4 + l] = 1.0
        t2[4 + l, SLOT_U] = float(u[l])
    Q0 = max(Q, 3 * M)
    pick = torch.cat([torch.arange(M).repeat(2), torch.randint(0, M, (Q0 - 2 * M,), generator=_g(seed + 3))])
    pick = pick[torch.randperm(Q0, generator=_g(seed + 4))]
    case = dict(x=_exact_rows(design)[None], gamma=torch.full((256,), 2.0), beta=torch.zeros(256), t2=t2, limg=_one_slot_limg(),
                basis=weights.point_embed_basis(), c0=0.0, q=grid[pick][None].float())
    return case, u, perm, pick


def _solve_rows(Ydes, T):
    """x [M,d] with LN(x) . T ~ Ydes (to ~1e-5 relative: LayerNorm's eps): the minimum-norm solution of [T | 1]^T w = [Ydes; 0] plus a
    vector of its null space that brings |w|^2 to d, so that w is its own LayerNorm output.  The references read x, not Ydes."""
    d = T.shape[0]
    A = torch.cat([T.double(), torch.ones(d, 1, dtype=torch.float64)], 1)                       # [d, 65]
    rhs = torch.cat([Ydes.double(), torch.zeros(Ydes.shape[0], 1, dtype=torch.float64)], 1)     # [M, 65]
    w0 = torch.linalg.solve(A.t() @ A, rhs.t()).t() @ A.t()                                     # [M, d]
    n = torch.randn(Ydes.shape[0], d, generator=_g(11), dtype=torch.float64)
    n = n - (torch.linalg.lstsq(A, n.t()).solution.t() @ A.t())
    n = n / n.norm(dim=1, keepdim=True)
    left = d - (w0 ** 2).sum(1)
    assert bool((left > 0).all()), "designed coefficients too large for the table's column scales"
    return (w0 + left.sqrt()[:, None] * n).float()


RAMP = (0.0, 3.0, 5.0, 40.0, 41.0, 100.0, 104.0, 300.0)


def _ramp_case(kind, Q=700, seed=7):
    """hb steps from one 32-latent tile to the next as in test_attention_reference_max_moves_lazily: +3 and +5 (below the threshold of 8:
    the maximum stays), +40, +41, +100, +104, +300 (log2 units) - 'rise'; the same falling - 'fall'; 'half1': a flat hb but for +60 on
    one latent of each sample whose accumulator row belongs to the h = 1 lanes only (rows 8g + 4 + i).  H and h0 are random with scores of
    a few units, u is N(0,1); real l_img and basis (dim 256).  M = 256, B = 3 (the samples differ in H, u and in the order inside a tile)."""
    dim, M, B = 256, 256, 3
    sd = _sd(dim, 128)
    _, limg, c0 = _tables(sd, dim)
    g = _g(seed)
    q = _queries(B, Q, seed + 1)
    basis = weights.point_embed_basis()
    Lm = _L_of(limg)
    rstd = float(((_features(q[0].double(), basis.double()) @ Lm.t()) ** 2).sum(1).add(1e-5).rsqrt().median())
    Ydes = torch.zeros(B, M, 64, dtype=torch.float64)
    Ydes[:, :, :52] = torch.randn(B, M, 52, generator=g, dtype=torch.float64) * (0.35 / rstd)
    Ydes[:, :, SLOT_U] = torch.randn(B, M, generator=g, dtype=torch.float64)
    steps = torch.tensor(RAMP if kind != "fall" else RAMP[::-1], dtype=torch.float64)
    if kind == "half1":
        for b, l in enumerate((4, 32 * 3 + 8 * 2 + 5, 32 * 7 + 8 * 3 + 7)):
            assert (l >> 2) & 1 == 1
            Ydes[b, l, SLOT_STD] = 60.0
    else:
        Ydes[:, :, SLOT_STD] = steps.repeat_interleave(32)[None] + torch.rand(B, M, generator=g, dtype=torch.float64)
    # column scales of the table: 4 x the largest designed entry of the column, so the solution stays well inside |w|^2 = d
    T = torch.randn(dim, 64, generator=g, dtype=torch.float64) * (4 * Ydes.abs().amax((0, 1)).clamp_min(1.0)) / math.sqrt(dim)
    x = torch.stack([_solve_rows(Ydes[b], T) for b in range(B)])
    return dict(x=x, gamma=torch.ones(dim), beta=torch.zeros(dim), t2=T.float(), limg=limg, basis=basis, c0=c0, q=q)


CRAFTED = {
    "scale_mixed": lambda: _block_case((2.0 ** -30, 1.0, 2.0 ** 12, 2.0 ** 30), target=2.0 ** -4),
    "scale_zero": lambda: _block_case((1.0, 1.0, 1.0), zero=True),
    "scale_tiny": lambda: _block_case((2.0 ** -118,) * 3, target=1.0),
    "range_2^20": lambda: _block_case((2.0 ** -20, 1.0), big_latent=(5, 44, 63), target=8.0),
    "ramp_rise": lambda: _ramp_case("rise"),
    "ramp_fall": lambda: _ramp_case("fall"),
    "ramp_half1": lambda: _ramp_case("half1"),
    "onehot_64": lambda: _onehot_case(64)[0],
    "onehot_128": lambda: _onehot_case(128)[0],
}


# ---- 1. real tables, model reference, shapes and tails ------------------------------------------------------------------------------------
SMALL_Q = (1, 31, 32, 33, 63, 64, 65, 767, 768, 769)
# B = 3: 256 / 3 = 85 workgroups of 12 waves per sample take 1020 chunks of 64 queries in one pass; chunk 1021 starts the second pass
CAP_Q = (1020 * 64 - 63, 1020 * 64 + 1, 1021 * 64 + 1)


@gpu
@pytest.mark.parametrize("dim,M,kind,bound", [(512, 512, "plain", 0.026), (512, 512, "peaked", 0.15), (256, 128, "plain", 0.073), (256, 128, "peaked", 0.26),
                                              (256, 512, "plain", 0.049), (512, 32, "plain", 0.14), (512, 1024, "plain", 0.018)])
def test_real_tables_every_query_count_against_the_model(dim, M, kind, bound):
    """B = 3, Q = 1 ... 769 around the 32-query half, the 64-query chunk and one workgroup's 12 chunks; at (256, 128) also the query counts
    around the grid cap's second pass.  Plain and peaked (stress_ae_state_dict) weights.  Measured k, in the order of the cases: 0.0107,
    0.0602, 0.0294, 0.107, 0.0196, 0.0593, 0.0073; bounds 0.026, 0.15, 0.073, 0.26, 0.049, 0.14, 0.018.  (k is far below 1 because T_q takes
    the worst latent's score size and the largest |u_l - ref|; the bound, not the unit, is what is tight.)"""
    Qs = SMALL_Q + (CAP_Q if (dim, M) == (256, 128) else ())
    sd, case = _real_case(dim, M, 3, max(Qs), kind)
    ref = _model_ref(sd, case)
    _, T = _formula(case, ref)
    worst = 0.0
    for Q in Qs:
        worst = max(worst, _k(_run(case, Q), ref[:, :Q], T[:, :Q]))
    _le(f"decode real {dim}/{M} {kind}", worst, bound)


# ---- 2. the timed launch, every element checked ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Q,bound", [(1200000, 0.023), (500003, 0.023)])
def test_the_benchmarks_launch_has_a_reference_for_every_element(Q, bound):
    """B = 1, 512/512: 8 192 reference queries drawn Q times (seeded, every one of them used), so each of the Q outputs has a float64 model
    reference: the grid cap 256 / B and the grid-stride loop of the launch that bench.py times.  Measured k: 0.00934 at both sizes; bound 0.023."""
    sd, case = _real_case(512, 512, 1, 8192, seed=2)
    ref = _model_ref(sd, case)
    _, T = _formula(case, ref)
    idx = torch.randint(0, 8192, (Q,), generator=_g(Q))
    assert idx.unique().numel() == 8192
    got = _run(dict(case, q=case["q"][:, idx]))
    _le(f"decode Q={Q}", _k(got, ref[:, idx], T[:, idx]), bound)


@gpu
def test_module_decode_of_1_2_million_queries_per_sample_against_the_golden():
    """The product path at the benchmark's size: m.decode(G5 latents) on G5's 4 096 golden queries drawn 1.2 M times per sample.  rel_l2
    against the golden logits under the 2e-3 of test_full_ae_encode_decode_vs_reference_golden, and every copy of a query within the
    largest error the 4 096-query launch itself shows against the golden."""
    from test_gpu_ae import _ae
    g = load_golden("g5_ae.npz")
    m = _ae(dim=512, M=512, latent_dim=32, N=10000)
    q = synth.queries(2, 4096)
    z = g["z"].cuda()
    gold = g["logits"].reshape(2, 4096).double()
    small = m.decode(z, q.cuda()).reshape(2, 4096).cpu().double()
    spread = float((small - gold).abs().max())
    idx = torch.randint(0, 4096, (1200000,), generator=_g(12))
    assert idx.unique().numel() == 4096
    big = m.decode(z, q[:, idx].cuda())
    assert big.shape == (2, 1200000, 1)
    big = big.reshape(2, -1).cpu().double()
    err = rel_l2(big, gold[:, idx])
    worst = float((big - gold[:, idx]).abs().max())
    print(f"module decode 1.2M: rel_l2 {err:.3g}, worst |error| {worst:.3g}, of the 4 096-query launch {spread:.3g}")
    assert err < 2e-3
    assert bool(torch.isfinite(big).all()) and worst <= spread


# ---- 3. many samples ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,bound", [(129, 0.073), (256, 0.083), (257, 0.076)])
def test_many_samples_each_against_its_own_reference(B, bound):
    """B = 129 (cap 256 / B = 1), 256 and 257 (one workgroup per sample), Q = 100, 256/128, every sample its own x.  Measured k: 0.0292,
    0.0333, 0.0304; bounds 0.073, 0.083, 0.076."""
    sd, case = _real_case(256, 128, B, 100, seed=3)
    ref = _model_ref(sd, case)
    _, T = _formula(case, ref)
    _le(f"decode B={B}", _k(_run(case), ref, T), bound)


# ---- 4. / 5. the per-sample scale of the fp16 image ----------------------------------------------------------------------------------------
@gpu
def test_per_sample_scale_of_samples_2_to_the_60_apart():
    """B = 4 whose coefficients are 2^-30, 1, 2^12, 2^30 times a table with scores of ~2^-4 log2 units: each sample within the same k in
    the batch and decoded alone, and bit-identical both ways (a scale read from another sample over- or underflows the fp16 image).
    The table's size keeps the largest sample's scores (2^26 .. 2^28) inside the kernel's domain (header of ae_decode.hip): with scores
    of ~6 the last sample's are 2^32, where fp32 cannot place a score within exp2's range of its own maximum, and its logits were NaN
    in the batch and alone.  Measured k per sample: 0.00056, 0.0126, 0.0326, 3e-12 (the same in the batch and alone);
    bound 0.08."""
    case = CRAFTED["scale_mixed"]()
    ref, T = _formula(case)
    got = _run(case)
    ks = [_k(got[b:b + 1], ref[b:b + 1], T[b:b + 1]) for b in range(4)]
    alone = [_run(case, rows=slice(b, b + 1)) for b in range(4)]
    ka = [_k(alone[b], ref[b:b + 1], T[b:b + 1]) for b in range(4)]
    print("k per sample in the batch", ks, "alone", ka)
    for b in range(4):
        assert torch.equal(alone[b], got[b:b + 1]), b
    _le("decode per-sample scale", max(ks + ka), 0.08)


@gpu
def test_all_zero_and_tiny_coefficients():
    """All coefficient columns zero: logit = mean(u) + c0 up to fp32 rounding (k, in fp16 units, ~0).  Largest coefficient ~2^-120: the
    scale's exponent would be 133; before ae_ctx_pack_kernel bounded it the image was inf * 0 = NaN (measured: k = inf).  Measured k: 0.00021 both;
    bound 0.0005."""
    case = CRAFTED["scale_zero"]()
    ref, T = _formula(case)
    Y = _context(case)
    assert float((ref - (Y[:, :, SLOT_U].mean(1, keepdim=True) + case["c0"])).abs().max()) < 1e-12
    _le("decode zero coefficients", _k(_run(case), ref, T), 0.0005)
    case = CRAFTED["scale_tiny"]()
    mx = float(_context(case)[:, :, :54].abs().max())
    print("largest coefficient 2^%.1f" % math.log2(mx))
    assert 2.0 ** -122 < mx < 2.0 ** -118
    ref, T = _formula(case)
    _le("decode tiny coefficients", _k(_run(case), ref, T), 0.0005)


@gpu
def test_one_latent_2_to_the_20_above_the_others():
    """One latent's coefficients 2^20 times the others' (scores ~8 against ~8 * 2^-20), a different latent per sample.  The image keeps 11
    bits of every entry above 2^-27 of the sample's largest and an absolute step of g = 2^-37 (of the largest entry's power of two) below:
    the small rows sit at 2^-20, so about 1 % of their entries (|N(0,1)| < 2^-7) fall under that floor; T_q charges g per entry.
    Measured k: 0.0271; bound 0.067."""
    case = CRAFTED["range_2^20"]()
    ref, T = _formula(case)
    _le("decode range 2^20", _k(_run(case), ref, T), 0.067)


# ---- 6. lazy maximum and the merge of the two lane halves -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,bound", [("rise", 0.0044), ("fall", 0.0055), ("half1", 0.00007)])
def test_maximum_moves_lazily_and_the_halves_merge(kind, bound):
    """_ramp_case: finite and within the unit.  Measured k: 0.00176, 0.00222, 2.84e-5; bounds 0.0044, 0.0055, 7e-5 (hb of 300
    enters A_q at the fp16 rate although it is carried in hi + lo: k is small)."""
    case = CRAFTED["ramp_" + kind]()
    ref, T = _formula(case)
    got = _run(case)
    assert bool(torch.isfinite(got).all())
    _le(f"decode ramp {kind}", _k(got, ref, T), bound)


# ---- 7. one-hot, exact ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M", [64, 128])
def test_one_hot_softmax_returns_the_selected_u_bit_for_bit(M):
    """_onehot_case: out == u[sel(q)] bit for bit; sel visits every latent (every residue mod 32, both lane halves, every tile).  Pins the
    latent <-> accumulator register <-> uv mapping."""
    case, u, perm, pick = _onehot_case(M)
    inv = torch.empty(M, dtype=torch.long)
    inv[perm] = torch.arange(M)
    sel = inv[pick]                                                               # latent that owns the query's grid point
    assert sel.unique().numel() == M
    ref, _ = _formula(case)
    assert float(((ref[0] - u[sel]) / u[sel]).abs().max()) < 1e-6               # the float64 reference is one-hot on sel too
    got = _run(case)
    assert torch.equal(got[0], u[sel].float()), (got[0] != u[sel].float()).nonzero()[:8]


# ---- 8. both basis kernels ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("basis_kind,dim,M,bound", [("dense", 512, 512, 0.0144), ("off_block", 512, 512, 0.0184), ("dense", 256, 128, 0.038),
                                                     ("off_block", 256, 128, 0.061)])
def test_a_basis_that_is_not_block_diagonal_takes_the_dense_kernel(basis_kind, dim, M, bound):
    """Tables built for a rotated basis (dense) and for the shipped basis with one off-block entry: ae_decode_stream_kernel<false>, three
    fmaf per projection, against the model with that basis.  Measured k: 0.0058, 0.0074, 0.0155, 0.0245; bounds 0.0144, 0.0184, 0.038,
    0.061."""
    basis = _rotated_basis(basis_kind)
    assert any(float(basis[a, e]) != 0 for a in range(3) for e in range(24) if e // 8 != a)
    sd, case = _real_case(dim, M, 3, 769, basis=basis, seed=4)
    ref = _model_ref(sd, case)
    _, T = _formula(case, ref)
    worst = max(_k(_run(case, Q), ref[:, :Q], T[:, :Q]) for Q in (65, 769))
    _le(f"decode {basis_kind} basis {dim}/{M}", worst, bound)


# ---- 9. query domain ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_queries_outside_the_unit_cube():
    """|coordinate| <= 4 (query_points and the post-processing feed [-1, 1]): 512 revolutions of the finest frequency still leave v_sin 15
    bits.  Measured k: 0.0163, inside the 0.026 that the same shape carries on [-1, 1], so that bound is asserted here too."""
    sd, case = _real_case(512, 512, 3, 2048, seed=5, lim=4.0)
    ref = _model_ref(sd, case)
    _, T = _formula(case, ref)
    got = _run(case)
    assert bool(torch.isfinite(got).all())
    _le("decode |coord| <= 4", _k(got, ref, T), 0.026)


# ---- 10. determinism ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_same_bits_twice_and_in_the_same_chunk():
    """The same call twice; a sample alone against the same sample inside a batch (its |max| word comes from an atomicMax: order-free; its
    chunks are the same 64 queries on another grid) and a slice of whole chunks: bit-identical.  A query among other wave-mates (a slice of the queries that starts
    in the middle of a chunk) is NOT: the lazy maximum moves when any lane of the wave asks, so a query's rescaling steps depend on its
    wave-mates (header of ae_decode.hip).  Measured: 9.5e-7 on logits of a few units; bounded by the 1e-5 of
    test_decode_many_queries_chunked_and_ragged."""
    sd, case = _real_case(512, 512, 3, 5000, "peaked", seed=6)
    a, b = _run(case), _run(case)
    assert torch.equal(a, b)
    for r in range(3):
        assert torch.equal(_run(case, rows=slice(r, r + 1)), a[r:r + 1])
    assert torch.equal(_run(dict(case, q=case["q"][:, 1280:1984].contiguous())), a[:, 1280:1984])       # 11 whole chunks
    part = _run(dict(case, q=case["q"][:, 1234:1301].contiguous()))
    print(f"a query among other wave-mates: differs by up to {float((part - a[:, 1234:1301]).abs().max()):.3g}")
    assert torch.allclose(part, a[:, 1234:1301], atol=1e-5, rtol=1e-5)


# ---- CPU side ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,M,kind", [(512, 512, "plain"), (256, 128, "peaked"), (512, 32, "plain")])
def test_references_agree_on_real_tables(dim, M, kind):
    """formula reference against model reference: 2e-4 rel_l2 as in test_decode_fold.py (the gap is the fp16 storage of L), for the shipped
    basis and for the two that take the dense kernel."""
    for basis in (None, _rotated_basis("dense"), _rotated_basis("off_block")):
        sd, case = _real_case(dim, M, 3, 600, kind, basis=basis)
        ref = _model_ref(sd, case)
        out, T = _formula(case, ref)
        err = rel_l2(out, ref)
        print("formula vs model", dim, M, kind, err)
        assert err < 2e-4
        assert bool(torch.isfinite(T).all()) and bool((T > 0).all())


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_cases_have_a_finite_positive_unit(name):
    case = CRAFTED[name]()
    ref, T = _formula(case)
    assert bool(torch.isfinite(ref).all())
    assert bool(torch.isfinite(T).all()) and bool((T > 0).all())


def test_exact_layernorm_rows_are_exact_in_fp32():
    """_exact_rows in IEEE fp32 (numpy), in two summation orders: mean 0, mean square + 1e-5f == 4.0f; the designed one-hot tables."""
    f = np.float32
    for M in (64, 128):
        case, u, perm, pick = _onehot_case(M)
        x = case["x"][0].numpy()
        assert np.all(x == np.round(x / LN_G) * LN_G)
        for order in (np.arange(256), np.random.RandomState(0).permutation(256)):
            s, sq = np.zeros(M, f), np.zeros(M, f)
            for c in order:
                s = f(s + x[:, c])
                sq = f(sq + f(x[:, c] * x[:, c]))
            assert np.all(s == 0) and np.all(f(f(sq * f(1 / 256)) + f(1e-5)) == f(4.0))
        Y = (case["x"][0].double() @ case["t2"].double())                          # LN(x) = x
        assert torch.equal(Y[:, SLOT_U], u) and u.unique().numel() == M
        assert bool((torch.log2(u.abs()) % 1 == 0).all())
        ref, _ = _formula(case)
        inv = torch.empty(M, dtype=torch.long)
        inv[perm] = torch.arange(M)
        assert float(((ref[0] - u[inv[pick]]) / u[inv[pick]]).abs().max()) < 1e-6


def test_decode_entry_refuses_bad_arguments(L_cpu):
    """every check of rald_op_ae_decode comes before its first HIP call and names the constraint"""
    L, d = L_cpu, DUMMY
    call = lambda B=2, Q=10, M=128, dim=256, x=d, q=d, out=d, scratch=d, nbytes=1 << 40: \
        L.rald_op_ae_decode(x, d, d, d, d, d, 0.0, q, out, B, Q, M, dim, scratch, nbytes, None)
    for M in (0, 48, 1056):
        _refused(L, call(M=M), "num_latents", "multiple of 32")
        assert L.rald_op_ae_decode_scratch_bytes(2, M) == -1
    _refused(L, call(dim=384), "dim", "256 or 512")
    _refused(L, call(Q=0), "n_queries")
    _refused(L, call(B=0), "batch")
    _refused(L, call(B=65536), "batch", "65535")
    assert L.rald_op_ae_decode_scratch_bytes(0, 128) == -1 and L.rald_op_ae_decode_scratch_bytes(65536, 128) == -1
    for kw in (dict(x=None), dict(q=None), dict(out=None), dict(scratch=None)):
        _refused(L, call(**kw), "null pointer")
    need = L.rald_op_ae_decode_scratch_bytes(2, 128)
    assert need >= 2 * (128 * 64 * 4 + 4 + 128 * 132 + 16)
    _refused(L, call(nbytes=need - 1), "scratch too small")
    _refused(L, call(scratch=d + 4), "16-byte aligned")
