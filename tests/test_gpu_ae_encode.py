"""The folded encoder of the set-latent autoencoder (rald_amd/csrc/ae_encode.hip, wired by Ae::encode) per element against float64:
ae_enc_features_kernel through rald_op_ae_enc_features, ae_enc_qproj_kernel through rald_op_ae_enc_qproj, the host tables of
rald_op_ae_encode_tables at their edges, and rald_ae_encode end to end at the smallest sizes that can go wrong.  Conventions are those of
test_gpu_resid_ln.py, test_gpu_attention.py and test_gpu_ae_decode.py (whose helpers are imported): float64 references computed on the
CPU from exactly the values the kernel read (fp32 inputs widened exactly; the fp32 x the kernel wrote is read back where the LayerNorm
consumes it), outputs pre-filled with NaN and followed by sentinels that must survive bit for bit, NaN behind every input the kernel
must not read past, every measured ratio printed before anything is asserted, bounds at most 2.5 times the worst value measured on an
MI355X.  U = 2^-24 throughout.

Error models.

  features   a_e = p . basis_e (float64, from the fp32 point and basis), tau_e = 1 + |x b_0e| + |y b_1e| + |z b_2e|:
      F  |F - f| <= 1/2 ulp_fp16(f) + k U tau_e              f = sin a_e, cos a_e.  The ulp term is the round-to-nearest conversion
                                                            (an absolute 2^-25 below fp16's normal range 2^-14): derived.  k U tau covers
                                                            the fp32 argument (three products, two sums, times 1/2pi), its reduction to
                                                            revolutions (rev - floor rev, + 1/4 for the cosine: 2^-24 revolutions) and
                                                            v_sin: measured.  Slots 48..50 are fp16(x | y | z) bit for bit, slot 51 and
                                                            52..63 zero bits, rows P..Pp-1 zero bits.
      G  |G - rstd f| <= 1/2 ulp_fp16(rstd f)               rstd = (|Wc f|^2 / d + 1e-5)^-1/2 DIRECTLY from PointEmbed's weights (Wc =
                       + k_r U (rstd tau_e                   [W | b] centred over the d channels), not from the factor R: the modified
                                + |rstd f| (c_f + c_r))      Gram-Schmidt of ae_embed_factor, its fp32 image and the kernel's triangular read
                                                            are pinned together.  rstd tau_e is the feature's own fp32 error.  rstd's
                                                            relative error is half that of var = sum_i s_i^2, s_i = sum_j R_ij f_j, whose
                                                            fp32 evaluation moves it by about 2 U sum_i |s_i| sum_j |R_ij| |f_j|, hence
                                                            c_r = (sum_i |s_i| sum_j |R_ij| |f_j| + 1e-5) / (var + 1e-5) >= 1, the ratio
                                                            of the absolute to the signed sums of the 52 row products as the kernel forms
                                                            them (R = the fp32 table, widened; c_r = 1 when var = 0: rsqrt and the fp32
                                                            1e-5 remain).  The features' fp32 errors enter var the same way with tau_j in
                                                            the place of |f_j|: c_f = sum_i |s_i| sum_j |R_ij| tau_j / (var + 1e-5) (a few
                                                            hundred on the unit cube: the finest frequency's argument is 400 radians).
      bias   the mean of (got - ref) / ulp_fp16(ref), plain and in the direction away from zero (times sign(ref)), over the elements
             of the points drawn at random (the crafted points repeat values, cos 0 = 1 above all, and with them one rounding error)
             whose fp16 ulp is at least 16 U x the fp32 term.  Round to nearest leaves both near 0 (floor 3 / sqrt(elements)); a
             conversion that truncates gives -0.5 in the second, one that rounds down -0.5 in the first
             (test_bias_measure_rejects_a_truncating_conversion, CPU).

  qproj      x = xin + X0[row % M] is ONE fp32 add: bit-equal to torch's.  With v = the x the kernel wrote, widened:
      Q  |Q_j - sum_c LN_c T1_cj| <= k U sum_c (|LN_c| + A_c) |T1_cj|,   A_c = rstd |gamma_c| (|v_c - mean| + mean_j |v_j|) + |beta_c|
                                                            A_c is the LayerNorm's own fp32 allowance in the form test_gpu_resid_ln.py uses
                                                            for h, without its single-pass factor E[v^2] / (var + eps): this kernel
                                                            subtracts the mean before it squares, so a row at offset 2^10 costs
                                                            rstd U mean|v| and no more.  A constant row has var = 0, rstd = 1e-5^-1/2.
      exact  rows of small integers with mean 0 and mean square 4 - 1e-5 in fp32 (test_gpu_ae_decode._exact_rows; for d = 512 such a row
             followed by itself rolled by 64 channels, which doubles every lane's partial sums), gamma = 2, beta = 0: LN(x) = x bit for bit;
             T1 = +-2^e, e = 0..3: every partial sum of Q is an integer multiple of 2^-7 below 2^24 of them, so Q is exact in any order.

  encode     the 2L moments of latent row (b, m) against oracle.rald_oracle.ae_encode_moments in float64 on the same fp32 weights and
             cloud; unit = 2^-8 times the rms of that row of the reference, every element within k units (bf16 operands of the five GEMMs
             behind the attentions are what k counts: 2^-8 is one bf16 step).  z and kl against the float64 posterior of the RETURNED mean
             and logvar within the bounds test_gpu_train_ops.py holds for rald_op_posterior (3.6 and 1.4).

Measured on an MI355X (worst over the listed cases; the bound asserted is at most 2.5 x that):
  features F   k   2.64  (K_F 6.6)   the same in every case with P >= 2: a coordinate of -2^-30, whose revolutions round to 1.0f
  features G   k_r 3.14  (K_R 7.8)   all-zero PointEmbed (rstd = rsqrt(1e-5f)); 2.9 on the seeded factors, 1.5 at PointEmbed x 2^6
  |bias|       F 0.0029, G 0.0018 at P = 1000 (BIAS_F 0.0071, BIAS_G 0.0043; smaller clouds sit under the floor 3 / sqrt(elements))
  qproj Q      k 0.59 at d = 256, 0.52 at d = 512  (K_Q 1.45); x and the exact case bit for bit
  encode       k 3.2 .. 4.8 on plain weights, 11.7 and 22.1 on peaked ones: beside each bound in ENCODE_CASES.  Whole-tensor rel-L2
               3.3e-3 .. 3.6e-3 plain, 5.1e-3 .. 5.6e-3 peaked (the old bound: 8e-3).  A sample in a batch of 3 equals the sample alone
               bit for bit, in a batch of 5 it differs by at most 1.2 units.  Posterior from the returned moments: z 1.74, kl 0.684
               (K_POST_Z 3.6, K_POST_KL 1.4 are test_gpu_train_ops.py's own; its L = 32 case sums 1 280 elements per sample, these 4 096)

What reaches what:
  ae_enc_features_kernel   P = 1 .. 1000 at B = 3 and B = 65 at P = 3 (ragged one-wave grid across samples), dim 512 and 256 factors,
                           zeros, +-1 faces, duplicates, |c| <= 4, -2^-30, multiples of pi/2          test_features_per_element
                           dependent / zero PointEmbed columns (r_jj = 0), all-zero PointEmbed (var = 0), PointEmbed x 2^-4, x 2^6
                                                                                                       test_features_weight_sets
  ae_embed_factor / ae_encode_tables (host)   the same weight sets: upper triangular, finite, |R f|^2 = |Wc f|^2 / d; zero pad columns
                                              of Q1 / T1 / T3 for dim 256 / 512, mix / learnable       test_tables_* (CPU)
  ae_enc_qproj_kernel<4>, <8>   rows 1 .. 1027 x M 1, 3, 128, xin null / given / in place, offset, tiny and constant rows
                                                                                                       test_qproj_per_element, test_qproj_exact
  Ae::encode 'mix'         P = 1 .. 129 (one or two key tiles, ragged), 1025 (key split: e_part + combine), B = 1, 3, 5 against B = 1,
                           512/512, peaked weights on a structured cloud                                test_encode_per_element
  Ae::encode 'learnable'   xin null, no mix attention, P = 1, 65, 1025                                  test_encode_per_element
  posterior wiring         eps layout, kl per sample, mean / logvar NULL                                test_encode_per_element
  stale LDS                features, qproj, one 'mix' and one 'learnable' encode                        test_same_bits_after_poisoned_lds
  argument checks (CPU)                                                                                test_entries_refuse_bad_arguments"""
import functools
import math
import time

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import rald_oracle as O
from rald_amd import synth, weights
from test_encode_fold import _tables as _enc_tables
from test_gpu_ae_decode import _exact_rows
from test_gpu_resid_ln import DUMMY, SENT, U, L_cpu, _bits, _Checks, _g, _guard_ok, _guarded, _ratio, _refused  # noqa: F401  (L_cpu is a fixture)
from test_gpu_train_ops import _posterior_ref

gpu = pytest.mark.gpu
NAN = float("nan")

# bounds (module docstring: measured values)
K_F = 6.6                                      # k of the features' fp32 term: measured 2.64
K_R = 7.8                                      # k_r of G's fp32 term: measured 3.14
BIAS_F, BIAS_G = 0.0071, 0.0043                # |mean signed error| in fp16 ulps: measured 0.0029, 0.0018 at P = 1000 (floor 3 / sqrt(elements))
K_Q = 1.45                                     # qproj: measured 0.59 (d = 256), 0.52 (d = 512)
K_POST_Z, K_POST_KL = 3.6, 1.4                 # the bounds test_posterior_both_branches_per_sample_kl_and_clamp_edges holds for rald_op_posterior


@pytest.fixture(scope="module")
def H():
    from rald_amd import _handles
    return _handles


@pytest.fixture(autouse=True)
def _timed(request):
    t = time.perf_counter()
    yield
    print(f"time {request.node.name}: {time.perf_counter() - t:.2f} s")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _half_ulp_f16(ref):
    """half an fp16 ulp of the float64 value: 2^(e-11) in the normal range, an absolute 2^-25 below 2^-14"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -40))).clamp_min(-14.0)
    return torch.exp2(e - 11)


def _bias(got, ref, noise=None):
    """(mean signed error, mean signed error away from zero, elements) in fp16 ulps of the reference, over the elements whose ulp is at
    least 16 x `noise` (the unit of the fp32 term: where it is larger the conversion is not what the error shows)"""
    ulp = 2 * _half_ulp_f16(ref)
    e = (got.double() - ref) / ulp
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    keep = torch.ones_like(e, dtype=torch.bool) if noise is None else ulp >= 16 * noise
    n = int(keep.sum())
    if n == 0:
        return 0.0, 0.0, 1
    return float(e[keep].mean()), float((e * torch.sign(ref))[keep].mean()), n


# ---- PointEmbed weight sets and the tables the product makes of them ----------------------------------------------------------------
WEIGHT_SETS = ("zero_col", "dup_col", "all_zero", "scale_lo", "scale_hi")


@functools.lru_cache(maxsize=None)
def _seed_sd(dim, mix=True):
    spec = weights.ae_spec(dim=dim, num_latents=128, depth=0, query_type="mix" if mix else "learnable")
    return weights.make_state_dict(spec, seed=0)


@functools.lru_cache(maxsize=None)
def _pe_case(dim, kind="plain"):
    """(state dict with this PointEmbed, its tables in float64 [Rf, Q1, T4, X0, T1, T3, c3]) - seed-0 weights, 128 latents"""
    sd = dict(_seed_sd(dim))
    W, b = sd["point_embed.mlp.weight"].clone(), sd["point_embed.mlp.bias"].clone()
    if kind == "zero_col":
        W[:, 7] = 0
    elif kind == "dup_col":
        W[:, 30] = W[:, 5]
        W[:, 49] = W[:, 48]
    elif kind == "all_zero":
        W.zero_(), b.zero_()
    elif kind == "scale_lo":
        W, b = W * 2.0 ** -4, b * 2.0 ** -4
    elif kind == "scale_hi":
        W, b = W * 2.0 ** 6, b * 2.0 ** 6
    else:
        assert kind == "plain"
    sd["point_embed.mlp.weight"], sd["point_embed.mlp.bias"] = W, b
    return sd, _enc_tables(sd, dim, 128, 8, True)


def _centred(sd):
    """Wc [d,52] float64: [W | b] of PointEmbed with every column centred over the d channels"""
    W = torch.cat([sd["point_embed.mlp.weight"].double(), sd["point_embed.mlp.bias"].double()[:, None]], 1)
    return W - W.mean(0, keepdim=True)


# ---- 1. features --------------------------------------------------------------------------------------------------------------------
def _points(B, P, seed):
    """[B,P,3] fp32; the kind of point b * P + p cycles through: random in the cube, exact zeros, a +-1 face, an exact duplicate of the
    point three before, |c| <= 4, coordinates of -2^-30 (rev - floor(rev) rounds to 1.0f), multiples of 1/256 (the finest frequency's
    argument 128 pi c is a multiple of pi/2), random."""
    g = _g(seed)
    n = B * P
    pts = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1).float()
    wide = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 8 - 4).float()
    face = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    axis = torch.randint(0, 3, (n,), generator=g)
    grid = torch.randint(-256, 257, (n, 3), generator=g).float() / 256
    for i in range(n):
        k = i % 8
        if k == 1:
            pts[i] = 0.0 if i % 16 == 1 else pts[i] * (torch.arange(3) != int(axis[i])).float()
        elif k == 2:
            pts[i, axis[i]] = face[i]
        elif k == 3:
            pts[i] = pts[i - 3]
        elif k == 4:
            pts[i] = wide[i]
        elif k == 5:
            pts[i, axis[i]] = -2.0 ** -30
            if i % 16 == 5:
                pts[i] = -2.0 ** -30
        elif k == 6:
            pts[i] = grid[i]
    return pts.view(B, P, 3)


def _features_ref(pc, basis, sd, Rf):
    """float64: f [B,P,52] (sin, cos, xyz, 1), tau [B,P,52], rstd [B,P] from the weights, c_r and c_f [B,P] from the fp32 factor"""
    p, bs = pc.double(), basis.double()
    parts = p[..., :, None] * bs                                         # [B,P,3,24], each product exact in float64 (24 x 24 bits)
    arg, tt = parts.sum(2), 1 + parts.abs().sum(2)
    one = torch.ones(p.shape[:2] + (1,), dtype=torch.float64)
    f = torch.cat([arg.sin(), arg.cos(), p, one], 2)
    tau = torch.cat([tt, tt, torch.zeros(p.shape[:2] + (4,), dtype=torch.float64)], 2)
    Wc = _centred(sd)
    var = ((f @ Wc.t()) ** 2).mean(-1)
    rstd = (var + 1e-5).rsqrt()
    R = torch.from_numpy(np.asarray(Rf, np.float64))
    s = (f @ R.t()).abs()
    den = (s ** 2).sum(-1) + 1e-5
    c_r = ((s * (f.abs() @ R.abs().t())).sum(-1) + 1e-5) / den
    c_f = (s * (tau @ R.abs().t())).sum(-1) / den
    return dict(f=f, tau=tau, rstd=rstd, c_r=c_r, c_f=c_f)


def _features_run(pc, basis, Rf):
    """rald_op_ae_enc_features on guarded buffers -> (F, G) as whole buffers (NaN-filled slices + sentinel tails) and the slice length"""
    from rald_amd._lib import check, lib
    B, P = pc.shape[:2]
    Pp = (P + 63) // 64 * 64
    n = B * Pp * 64
    pcbuf = torch.full((B * P * 3 + 192,), NAN, device="cuda")
    pcbuf[:B * P * 3] = pc.reshape(-1).cuda()
    tab = torch.full((72 + 52 * 52 + 64,), NAN, device="cuda")           # basis | factor | NaN
    tab[:72] = basis.reshape(-1).cuda()
    tab[72:72 + 2704] = torch.from_numpy(np.asarray(Rf, np.float32)).reshape(-1).cuda()
    F, G = _guarded(n, 256, torch.float16), _guarded(n, 256, torch.float16)
    check(lib().rald_op_ae_enc_features(pcbuf.data_ptr(), tab.data_ptr(), tab[72:].data_ptr(), F.data_ptr(), G.data_ptr(), B, P, Pp, _stream()))
    torch.cuda.synchronize()
    return F, G, n


def _features_check(chk, name, pc, dim, kind="plain"):
    """every assertion of section 1 on one cloud"""
    sd, tabs = _pe_case(dim, kind)
    basis = sd["point_embed.basis"]
    B, P = pc.shape[:2]
    Pp = (P + 63) // 64 * 64
    Fb, Gb, n = _features_run(pc, basis, tabs[0])
    chk.true(f"{name}: sentinel behind F", _guard_ok(Fb, n))
    chk.true(f"{name}: sentinel behind G", _guard_ok(Gb, n))
    F, G = Fb[:n].view(B, Pp, 64).cpu(), Gb[:n].view(B, Pp, 64).cpu()
    zero = lambda t: not bool(_bits(t.contiguous()).any())
    chk.true(f"{name}: pad rows of F are zero bits", zero(F[:, P:]))
    chk.true(f"{name}: pad rows of G are zero bits", zero(G[:, P:]))
    chk.true(f"{name}: slots 52..63 of F are zero bits", zero(F[:, :P, 52:]))
    chk.true(f"{name}: slots 52..63 of G are zero bits", zero(G[:, :P, 52:]))
    chk.true(f"{name}: slot 51 of F is zero", zero(F[:, :P, 51]))
    chk.true(f"{name}: slots 48..50 of F are fp16(x | y | z)", _same_bits(F[:, :P, 48:51].contiguous(), pc.half()))
    r = _features_ref(pc, basis, sd, tabs[0])
    f, tau, rstd = r["f"], r["tau"], r["rstd"][..., None]
    kf = _ratio(F[:, :P, :48], f[..., :48], tau[..., :48], extra=_half_ulp_f16(f[..., :48]))
    g = f * rstd
    tg = rstd * tau + g.abs() * (r["c_f"] + r["c_r"])[..., None]
    kr = _ratio(G[:, :P, :52], g, tg, extra=_half_ulp_f16(g))
    rnd = ((torch.arange(B * P) % 8 == 0) | (torch.arange(B * P) % 8 == 7)).view(B, P)       # _points: the points drawn at random in the cube
    bf = _bias(F[:, :P, :48][rnd], f[..., :48][rnd], U * tau[..., :48][rnd])
    bg = _bias(G[:, :P, :52][rnd], g[rnd], U * tg[rnd])
    chk.le(f"{name} F k", kf, K_F)
    chk.le(f"{name} G k_r", kr, K_R)
    chk.le(f"{name} F |bias| ({bf[0]:+.3g}, away from zero {bf[1]:+.3g}, {bf[2]} elements)", max(abs(bf[0]), abs(bf[1])), max(BIAS_F, 3.0 / math.sqrt(bf[2])))
    chk.le(f"{name} G |bias| ({bg[0]:+.3g}, away from zero {bg[1]:+.3g}, {bg[2]} elements)", max(abs(bg[0]), abs(bg[1])), max(BIAS_G, 3.0 / math.sqrt(bg[2])))
    print(f"{name}: rstd {float(rstd.min()):.3g} .. {float(rstd.max()):.3g}, c_r up to {float(r['c_r'].max()):.3g}, c_f up to {float(r['c_f'].max()):.3g}")


FEATURE_SHAPES = [(3, 1), (3, 2), (3, 63), (3, 64), (3, 65), (3, 127), (3, 129), (3, 1000), (65, 3)]


@gpu
@pytest.mark.parametrize("dim", [512, 256])
def test_features_per_element(dim):
    """Every element of F and G at every shape of FEATURE_SHAPES (B, P), on the factor rald_op_ae_encode_tables makes of the seed-0
    PointEmbed at this dim.  Measured k 2.64 at both dims, k_r 2.89 (512) and 2.83 (256) (P = 1: 1.13 and 0.67); bounds K_F, K_R."""
    chk = _Checks()
    for B, P in FEATURE_SHAPES:
        _features_check(chk, f"features d{dim} B{B} P{P}", _points(B, P, 100 + P + B), dim)
    chk.done()


@gpu
@pytest.mark.parametrize("kind", WEIGHT_SETS)
def test_features_weight_sets(kind):
    """P = 129, B = 3, dim 256: a zero and two duplicated PointEmbed columns (r_jj = 0 in ae_embed_factor), an all-zero PointEmbed
    (var = 0: G = 1e-5^-1/2 f), PointEmbed times 2^-4 and 2^6 (the ends of G's documented domain: every |f| >= 2^-8 stays in fp16's
    normal range).  Measured k 2.64 in all five; k_r 2.81, 2.81, 3.14, 3.12, 1.47 in the order of WEIGHT_SETS."""
    chk = _Checks()
    pc = _points(3, 129, 7)
    _features_check(chk, f"features {kind}", pc, 256, kind)
    if kind in ("scale_lo", "scale_hi", "all_zero"):
        sd, tabs = _pe_case(256, kind)
        r = _features_ref(pc, sd["point_embed.basis"], sd, tabs[0])
        g = (r["f"] * r["rstd"][..., None])[..., :48].abs()
        big = r["f"][..., :48].abs() >= 2.0 ** -8
        chk.true(f"{kind}: G in fp16's normal range for |f| >= 2^-8", bool((g[big] >= 2.0 ** -14).all()) and float(g.max()) < 65504)
    chk.done()


# ---- 2. host tables at their edges (CPU) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("zero_col", "dup_col", "all_zero"))
def test_tables_factor_of_dependent_columns(kind):
    """Rf is upper triangular (the kernel never reads left of the diagonal block), finite, and |Rf f|^2 = |Wc f|^2 / d in float64 on 1000
    random feature rows to 1e-5 relative (+ 1e-5, LayerNorm's eps, which is all there is for the all-zero PointEmbed)."""
    sd, tabs = _pe_case(256, kind)
    R = torch.from_numpy(tabs[0])
    assert bool(torch.isfinite(R).all())
    assert not bool(torch.tril(R, -1).any()), "entries left of the diagonal"
    f = torch.rand(1000, 52, generator=_g(3), dtype=torch.float64) * 2 - 1
    f[:, 51] = 1.0
    a, b = ((f @ R.t()) ** 2).sum(-1), ((f @ _centred(sd).t()) ** 2).mean(-1)
    err = float(((a - b).abs() / (b + 1e-5)).max())
    print(f"factor of {kind}: |R f|^2 against |Wc f|^2 / d, worst relative {err:.3g}; zero diagonal entries {int((R.diagonal() == 0).sum())}")
    assert err < 1e-5
    assert int((R.diagonal() == 0).sum()) == {"zero_col": 1, "dup_col": 2, "all_zero": 52}[kind]


@pytest.mark.parametrize("dim", [256, 512])
@pytest.mark.parametrize("mix", [True, False])
def test_tables_pad_columns_are_zero(dim, mix):
    """heads = 8: columns 51..63 of every head block of Q1 (the constant's score is dropped) and 52..63 of T1 and T3 are exactly zero -
    the attention multiplies them with the zero slots of F and G, and 0 * NaN would not be 0."""
    Rf, Q1, T4, X0, T1, T3, c3 = _enc_tables(_seed_sd(dim, mix), dim, 128, 8, mix)
    assert not T1[:, 52:].any() and not T3[:, 52:].any()
    assert T1[:, :52].all() and T3[:, :52].all()
    if mix:
        Q1 = Q1.reshape(128, 8, 64)
        assert not Q1[:, :, 51:].any() and Q1[:, :, :51].all()
    else:
        assert not Q1.any() and not T4.any()                             # not written
        assert np.array_equal(X0, _seed_sd(dim, False)["latents.weight"].double().numpy())


def test_bias_measure_rejects_a_truncating_conversion():
    """the bias figures on the float64 reference itself: round to nearest passes, round towards zero and round down do not"""
    pc = synth.point_cloud(3, 129, seed=7)
    sd, tabs = _pe_case(256)
    r = _features_ref(pc, sd["point_embed.basis"], sd, tabs[0])
    f, noise = r["f"][..., :48], U * r["tau"][..., :48]
    near = f.half()
    step = lambda less, more: (near.view(torch.int16) - less.to(torch.int16) + more.to(torch.int16)).view(torch.float16)   # sign-magnitude bits
    above = near.double() > f
    down = step(above & (f > 0), above & (f < 0))
    trunc = step(near.double().abs() > f.abs(), torch.zeros_like(above))
    assert bool((down.double() <= f).all()) and bool((trunc.double().abs() <= f.abs()).all())
    for name, got, fails in (("nearest", near, False), ("towards zero", trunc, True), ("down", down, True)):
        b = _bias(got, f, noise)
        print(f"bias of {name}: {b[0]:+.3g}, away from zero {b[1]:+.3g} over {b[2]} elements")
        assert (max(abs(b[0]), abs(b[1])) > max(BIAS_F, BIAS_G, 3.0 / math.sqrt(b[2]))) == fails
    assert _bias(trunc, f, noise)[1] < -0.4 and _bias(down, f, noise)[0] < -0.4


# ---- 3. qproj ---------------------------------------------------------------------------------------------------------------------------
def _row_kinds(n, d, g):
    """[n,d] rows: 0 plain N(0,1), 1 offset 2^10 spread 1, 2 spread 2^-10, 3 offset -3 spread 0.5, cycling"""
    x = torch.randn(n, d, generator=g)
    k = torch.arange(n) % 4
    x[k == 1] += 1024.0
    x[k == 2] *= 2.0 ** -10
    x[k == 3] = x[k == 3] * 0.5 - 3.0
    return x


def _qproj_data(d, rows, M, with_xin, seed):
    """X0 [M,d], xin [rows,d] or None, gamma, beta, T1 [d,64] (all 64 columns non-zero).  Row 0 of x is constant; the other rows of x cycle
    through _row_kinds (xin = the wanted row minus X0[row % M], so x is that row to a few ulps of X0), or, without xin, the rows of X0 do."""
    g = _g(seed)
    X0 = _row_kinds(M, d, g) if not with_xin else torch.randn(M, d, generator=g) * 0.7
    X0[0] = 0.75
    xin = None
    if with_xin:
        xin = _row_kinds(rows, d, g) - X0[torch.arange(rows) % M]
        xin[0] = 1.25
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    return dict(X0=X0, xin=xin, gamma=gamma, beta=beta, T1=torch.randn(d, 64, generator=g) / math.sqrt(d), rows=rows, M=M, d=d)


def _qproj_run(H, c, in_place=False):
    """-> (x buffer, Q buffer): rows * d and rows * 64 floats, NaN before the call, each before 64 sentinels; NaN behind xin and X0"""
    rows, M, d = c["rows"], c["M"], c["d"]
    x, Q = _guarded(rows * d, 64), _guarded(rows * 64, 64)
    X0b = torch.full((M * d + 1024,), NAN, device="cuda")
    X0b[:M * d] = c["X0"].reshape(-1).cuda()
    xin = None
    if c["xin"] is not None:
        if in_place:
            x[:rows * d] = c["xin"].reshape(-1).cuda()
            xin = x[:rows * d].view(rows, d)
        else:
            xb = torch.full((rows * d + 1024,), NAN, device="cuda")
            xb[:rows * d] = c["xin"].reshape(-1).cuda()
            xin = xb[:rows * d].view(rows, d)
    H.op_ae_enc_qproj(xin, X0b[:M * d].view(M, d), x[:rows * d].view(rows, d), c["gamma"].cuda(), c["beta"].cuda(), c["T1"].cuda(),
                      Q[:rows * 64].view(rows, 64), rows)
    torch.cuda.synchronize()
    return x, Q


def _qproj_ref(c, xk):
    """(float64 Q, terms) from the x the kernel wrote"""
    v = xk.double()
    mean = v.mean(-1, keepdim=True)
    dv = v - mean
    rstd = ((dv ** 2).mean(-1, keepdim=True) + 1e-5).rsqrt()
    ga, be, T1 = c["gamma"].double(), c["beta"].double(), c["T1"].double()
    ln = dv * rstd * ga + be
    A = rstd * ga.abs() * (dv.abs() + v.abs().mean(-1, keepdim=True)) + be.abs()
    return ln @ T1, (ln.abs() + A) @ T1.abs()


def _qproj_check(H, chk, name, c, in_place=False):
    rows, M, d = c["rows"], c["M"], c["d"]
    xb, Qb = _qproj_run(H, c, in_place)
    chk.true(f"{name}: sentinel behind x", _guard_ok(xb, rows * d))
    chk.true(f"{name}: sentinel behind Q", _guard_ok(Qb, rows * 64))
    xk, Q = xb[:rows * d].view(rows, d).cpu(), Qb[:rows * 64].view(rows, 64).cpu()
    want = c["X0"][torch.arange(rows) % M]
    if c["xin"] is not None:
        want = c["xin"] + want                                             # one fp32 add
    chk.true(f"{name}: x is the fp32 sum, bit for bit", _same_bits(xk, want))
    ref, terms = _qproj_ref(c, xk)
    chk.le(f"{name} Q k", _ratio(Q, ref, terms), K_Q)
    return xb, Qb


QPROJ_ROWS, QPROJ_M = (1, 3, 4, 5, 130, 1027), (1, 3, 128)


@gpu
@pytest.mark.parametrize("with_xin", [False, True])
@pytest.mark.parametrize("d", [256, 512])
def test_qproj_per_element(H, d, with_xin):
    """rows x M of QPROJ_ROWS x QPROJ_M (rows % 4 != 0 and rows % M != 0 both occur; the last workgroup clamps its row index and writes
    nothing past `rows`); with xin also in place (x = xin, the product's call).  Measured k: 0.41 (256, no xin), 0.59 (256, xin), 0.39
    (512, no xin), 0.52 (512, xin); bound K_Q."""
    chk = _Checks()
    for rows in QPROJ_ROWS:
        for M in QPROJ_M:
            c = _qproj_data(d, rows, M, with_xin, 10 * rows + M + d)
            _qproj_check(H, chk, f"qproj d{d} rows {rows} M {M} xin {with_xin}", c)
            if with_xin and M == 3:
                _qproj_check(H, chk, f"qproj d{d} rows {rows} M {M} in place", c, in_place=True)
    chk.done()


def _qproj_exact_data(d, seed=5):
    """9 rows (three workgroups, the last one clamped) with LN(x) = x bit for bit and T1 = +-2^e"""
    g = _g(seed + d)
    design = torch.zeros(9, 256, dtype=torch.float64)
    design[:, :200] = torch.randint(-128, 129, (9, 200), generator=g).double() * 2.0 ** -7
    a = _exact_rows(design)
    X0 = a if d == 256 else torch.cat([a, torch.roll(a, -64, 1)], 1)
    T1 = torch.exp2(torch.randint(0, 4, (d, 64), generator=g).float()) * torch.where(torch.rand(d, 64, generator=g) < 0.5, -1.0, 1.0)
    return dict(X0=X0, xin=None, gamma=torch.full((d,), 2.0), beta=torch.zeros(d), T1=T1, rows=9, M=9, d=d)


@pytest.mark.parametrize("d", [256, 512])
def test_qproj_exact_rows_are_exact_in_fp32(d):
    """the exact case in IEEE fp32 (numpy): each lane's channels (lane + 64 i) in order, then the 64 lane sums in two orders (at d = 256 any
    order of the channels is exact; at d = 512 the sum of squares passes 2^24 units of 2^-14, where fp32 holds only the even ones, and every
    lane sum is even): mean 0, mean square + 1e-5f == 4.0f; |x| . |T1| stays below 2^24 units of 2^-7, and the output columns differ"""
    c = _qproj_exact_data(d)
    x, f = c["X0"].numpy(), np.float32
    assert np.all(x == np.round(x * 128) / 128)
    s, sq = np.zeros((9, 64), f), np.zeros((9, 64), f)
    for i in range(d // 64):
        v = x[:, 64 * i:64 * i + 64]
        s = f(s + v)
        sq = f(sq + f(v * v))
    assert d == 256 or np.all((sq.astype(np.float64) * 2.0 ** 14) % 2 == 0)
    for order in (np.arange(64), np.random.RandomState(0).permutation(64)):
        ts, tq = np.zeros(9, f), np.zeros(9, f)
        for lane in order:
            ts = f(ts + s[:, lane])
            tq = f(tq + sq[:, lane])
        assert np.all(ts == 0) and np.all(f(f(tq * f(1 / d)) + f(1e-5)) == f(4.0))
    assert float((c["X0"].double().abs() @ c["T1"].double().abs()).max()) * 128 < 2.0 ** 24
    q = c["X0"].double() @ c["T1"].double()
    assert all(q[r].unique().numel() >= 60 for r in range(9)) and torch.equal(q.float().double(), q)


@gpu
@pytest.mark.parametrize("d", [256, 512])
def test_qproj_exact(H, d):
    """LN(x) = x exactly and power-of-two T1: Q is the float64 product bit for bit, for all 64 columns, every row of the three workgroups
    and both d: pins lane <-> channel <-> project4_rows' quarter <-> output column."""
    c = _qproj_exact_data(d)
    xb, Qb = _qproj_run(H, c)
    assert _guard_ok(xb, 9 * d) and _guard_ok(Qb, 9 * 64)
    assert _same_bits(xb[:9 * d].view(9, d).cpu(), c["X0"])
    want = (c["X0"].double() @ c["T1"].double()).float()
    got = Qb[:9 * 64].view(9, 64).cpu()
    assert _same_bits(got, want), (got != want).nonzero()[:8]


# ---- 4. rald_ae_encode end to end -----------------------------------------------------------------------------------------------------
L_DIM = 32
# name: (dim, M, query type, weights, cloud, P, B, bound on k)   # measured k (B = 3, 5: the worst of the batch and the samples alone)
ENCODE_CASES = {
    "mix P1": (256, 128, "mix", "plain", "uniform", 1, 2, 9.3),  # 3.76
    "mix P2": (256, 128, "mix", "plain", "uniform", 2, 2, 9.4),                                                       # 3.77
    "mix P63": (256, 128, "mix", "plain", "uniform", 63, 2, 9.3),  # 3.75
    "mix P64": (256, 128, "mix", "plain", "uniform", 64, 2, 9.8),                                                     # 3.94
    "mix P65": (256, 128, "mix", "plain", "uniform", 65, 2, 9.3),  # 3.75
    "mix P129": (256, 128, "mix", "plain", "uniform", 129, 2, 8.9),                                                   # 3.57
    "mix P1025": (256, 128, "mix", "plain", "uniform", 1025, 2, 10),  # 4.12
    "mix P65 B1": (256, 128, "mix", "plain", "uniform", 65, 1, 8),                                                    # 3.21
    "mix P65 B3": (256, 128, "mix", "plain", "uniform", 65, 3, 9.8),  # 3.95
    "mix P65 B5": (256, 128, "mix", "plain", "uniform", 65, 5, 11),                                                   # 4.77
    "learnable P1": (256, 128, "learnable", "plain", "uniform", 1, 2, 9.6),  # 3.85
    "learnable P65": (256, 128, "learnable", "plain", "uniform", 65, 2, 9.7),                                         # 3.89
    "learnable P1025": (256, 128, "learnable", "plain", "uniform", 1025, 2, 10),  # 4.03
    "512 P65": (512, 512, "mix", "plain", "uniform", 65, 1, 11),                                                      # 4.46
    "512 P1025": (512, 512, "mix", "plain", "uniform", 1025, 1, 9.3),  # 3.74
    "structured 256 plain": (256, 128, "mix", "plain", "structured", 1025, 2, 11),                                    # 4.62
    "structured 256 peaked": (256, 128, "mix", "peaked", "structured", 1025, 2, 29),  # 11.7
    "structured 512 plain": (512, 512, "mix", "plain", "structured", 1025, 1, 10),                                    # 4.09
    "structured 512 peaked": (512, 512, "mix", "peaked", "structured", 1025, 1, 55),  # 22.1
}


@functools.lru_cache(maxsize=None)
def _model(dim, M, qt, kind, P):
    """KLAutoEncoder with one latent layer (encode never touches the stack) on seeded weights -> (module on the device, its fp32 state dict)"""
    from rald_amd import models_ae as A
    m = A.KLAutoEncoder(depth=1, dim=dim, queries_dim=dim, num_inputs=P, num_latents=M, latent_dim=L_DIM, heads=8, dim_head=64, query_type=qt)
    sd = weights.make_state_dict(weights.spec_of_state_dict(m.state_dict()), 0)
    if kind == "peaked":
        sd = weights.stress_ae_state_dict(sd)
    m.load_state_dict(sd, strict=True)
    return m.cuda(), sd


def _cloud(kind, B, P, seed):
    return synth.structured_cloud(B, P, seed=seed) if kind == "structured" else synth.point_cloud(B, P, seed=seed)


def _encode(m, pc, eps, moments=True):
    """rald_ae_encode: the cloud before a NaN tail, every output pre-filled with NaN before its sentinels -> dict of CPU tensors"""
    from rald_amd._lib import check, lib
    B, P = pc.shape[:2]
    M, L = m.num_latents, m.latent_dim
    n = B * M * L
    pcbuf = torch.full((B * P * 3 + 192,), NAN, device="cuda")
    pcbuf[:B * P * 3] = pc.reshape(-1).cuda()
    epsd = eps.contiguous().cuda()
    z, kl = _guarded(n, 64), _guarded(B, 16)
    mean, logvar = (_guarded(n, 64), _guarded(n, 64)) if moments else (None, None)
    ptr = lambda t: None if t is None else t.data_ptr()
    check(lib().rald_ae_encode(m._handle()._h, pcbuf.data_ptr(), B, epsd.data_ptr(), ptr(mean), ptr(logvar), z.data_ptr(), kl.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert _guard_ok(z, n) and _guard_ok(kl, B), "encode wrote past z / kl"
    out = dict(z=z[:n].view(B, M, L).cpu(), kl=kl[:B].cpu())
    if moments:
        assert _guard_ok(mean, n) and _guard_ok(logvar, n), "encode wrote past mean / logvar"
        out.update(mean=mean[:n].view(B, M, L).cpu(), logvar=logvar[:n].view(B, M, L).cpu())
    return out


def _encode_ref(sd, pc):
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        mean, logvar = O.ae_encode_moments(sd64, pc.double())
    return torch.cat([mean, logvar], -1)                                   # [B,M,2L]


def _row_units(got, ref):
    """largest |got - ref| in units of 2^-8 x the rms of the reference's latent row, NaN counted as infinite"""
    unit = 2.0 ** -8 * (ref ** 2).mean(-1, keepdim=True).sqrt()
    r = (got.double() - ref).abs() / unit
    return float(torch.where(torch.isnan(r), torch.full_like(r, math.inf), r).max())


@gpu
@pytest.mark.parametrize("name", list(ENCODE_CASES))
def test_encode_per_element(name):
    """One case of ENCODE_CASES: every element of mean | logvar of every latent within `bound` units (2^-8 x the rms of the reference's
    row); z and kl against the float64 posterior of the returned moments; the same z and kl bit for bit when mean / logvar are NULL; the
    B = 3 and B = 5 cases also sample by sample against the sample encoded alone, within twice the bound."""
    dim, M, qt, kind, cloud, P, B, bound = ENCODE_CASES[name]
    chk = _Checks()
    m, sd = _model(dim, M, qt, kind, P)
    pc = _cloud(cloud, B, P, 40 + P + B)
    eps = torch.randn(B, M, L_DIM, generator=_g(P + B))
    ref = _encode_ref(sd, pc)
    out = _encode(m, pc, eps)
    got = torch.cat([out["mean"], out["logvar"]], -1)
    for key in ("mean", "logvar", "z", "kl"):
        chk.true(f"{name}: {key} finite", bool(torch.isfinite(out[key]).all()))
    print(f"encode {name}: rel-L2 mean {rel_l2(out['mean'], ref[..., :L_DIM]):.3g}, logvar {rel_l2(out['logvar'], ref[..., L_DIM:]):.3g} (whole tensors)")
    chk.le(f"encode {name} k", _row_units(got, ref), bound)
    # the posterior's wiring, from the moments the call returned
    ml = got.double()
    zr, klr = _posterior_ref(ml, eps.double(), L_DIM)
    mean, lv = ml[..., :L_DIM], torch.clamp(ml[..., L_DIM:], -30.0, 20.0)
    tz = mean.abs() + torch.exp(0.5 * lv) * eps.double().abs() * (1 + 0.5 * lv.abs())
    tkl = 0.5 * torch.mean(mean ** 2 + torch.exp(lv) * (1 + lv.abs()) + 1 + lv.abs(), dim=[1, 2])
    chk.le(f"encode {name} z", _ratio(out["z"], zr, tz), K_POST_Z)
    chk.le(f"encode {name} kl", _ratio(out["kl"], klr, tkl), K_POST_KL)
    bare = _encode(m, pc, eps, moments=False)
    chk.true(f"{name}: same z and kl without mean / logvar", _same_bits(bare["z"], out["z"]) and _same_bits(bare["kl"], out["kl"]))
    if B > 2:
        for b in range(B):
            one = _encode(m, pc[b:b + 1], eps[b:b + 1])
            alone = torch.cat([one["mean"], one["logvar"]], -1)
            chk.le(f"encode {name} sample {b} alone k", _row_units(alone, ref[b:b + 1]), bound)
            chk.le(f"encode {name} sample {b} in the batch against alone", _row_units(got[b:b + 1], alone.double()) , 2 * bound)
    chk.done()


# ---- 5. same bits twice, and after poisoned LDS ----------------------------------------------------------------------------------------
@gpu
def test_same_bits_after_poisoned_lds(H):
    """features (the factor sits in LDS), qproj (normalised rows and partial sums in LDS), one 'mix' and one 'learnable' encode: run,
    rald_debug_poison_lds, run again - the whole buffers, sentinels included, are bit-identical."""
    from rald_amd._lib import check, lib
    poison = lambda: check(lib().rald_debug_poison_lds(_stream()))
    sd, tabs = _pe_case(256)
    pc = _points(3, 129, 7)
    runs = {"features": lambda: _features_run(pc, sd["point_embed.basis"], tabs[0])[:2]}
    for d in (256, 512):
        for with_xin in (False, True):
            c = _qproj_data(d, 130, 3, with_xin, 77 + d)
            runs[f"qproj d{d} xin {with_xin}"] = lambda c=c: _qproj_run(H, c)
    for name in ("mix P1025", "learnable P65"):
        dim, M, qt, kind, cloud, P, B, _ = ENCODE_CASES[name]
        m, _sd = _model(dim, M, qt, kind, P)
        cl, eps = _cloud(cloud, B, P, 40 + P + B), torch.randn(B, M, L_DIM, generator=_g(P + B))
        runs[f"encode {name}"] = lambda m=m, cl=cl, eps=eps: tuple(_encode(m, cl, eps)[k] for k in ("mean", "logvar", "z", "kl"))
    for name, run in runs.items():
        a = run()
        poison()
        b = run()
        assert all(_same_bits(s, t) for s, t in zip(a, b)), name


# ---- 6. argument checks (CPU: each fires before the entry's first HIP call) -----------------------------------------------------------
def test_entries_refuse_bad_arguments(L_cpu):
    """rald_op_ae_enc_qproj and rald_op_ae_enc_features on fake aligned pointers: each refusal names its constraint"""
    L, d = L_cpu, DUMMY
    qp = lambda xin=d, X0=d, x=d, gamma=d, beta=d, T1=d, Q=d, rows=8, M=4, dim=256: \
        L.rald_op_ae_enc_qproj(xin, X0, x, gamma, beta, T1, Q, rows, M, dim, None)
    for dim in (0, 64, 128, 384, 1024):
        _refused(L, qp(dim=dim), "dim", "256 or 512")
    for rows in (0, -1):
        _refused(L, qp(rows=rows), "rows", "at least 1")
    for M in (0, -3):
        _refused(L, qp(M=M), "num_latents", "at least 1")
    for kw in (dict(X0=None), dict(x=None), dict(gamma=None), dict(beta=None), dict(T1=None), dict(Q=None)):
        _refused(L, qp(**kw), "null pointer")
    ft = lambda pc=d, basis=d, R=d, F=d, G=d, B=2, P=100, Pp=128: L.rald_op_ae_enc_features(pc, basis, R, F, G, B, P, Pp, None)
    for kw in (dict(pc=None), dict(basis=None), dict(R=None), dict(F=None), dict(G=None)):
        _refused(L, ft(**kw), "null pointer")
    _refused(L, ft(B=0), "batch", "at least 1")
    _refused(L, ft(P=0, Pp=0), "n_points", "at least 1")
    _refused(L, ft(P=129, Pp=128), "rows_per_sample", "at least n_points")
    for Pp in (100, 127, 160 - 1):
        _refused(L, ft(Pp=Pp), "rows_per_sample", "multiple of 64")
    _refused(L, ft(F=d + 8), "16-byte aligned")
    _refused(L, ft(G=d + 2), "16-byte aligned")


def test_qproj_wrapper_checks_shapes_before_the_library():
    """_handles.op_ae_enc_qproj refuses host tensors and wrong sizes itself (no device needed: nothing is launched)"""
    from rald_amd import _handles as Hd
    t = torch.zeros
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        Hd.op_ae_enc_qproj(None, t(4, 256), t(8, 256), t(256), t(256), t(256, 64), t(8, 64), 8)
