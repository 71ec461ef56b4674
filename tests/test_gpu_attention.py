"""The attention forward family per element against float64: attention_d64_kernel in its five instantiations and attention_combine_kernel
through rald_op_attention_args (it fills a whole AttnArgs), attn_self_proj_kernel / xattn_q2_proj_kernel with fp32 and fp16 slabs through
rald_op_attn_self_proj_slabs / rald_op_xattn_q2_proj_slabs, and the eight-slab fp16 reduce through rald_op_reduce_resid_ln_slabs.
Conventions are those of test_gpu_resid_ln.py (whose helpers are imported): float64 references computed on the CPU from exactly the
values the kernel read (bf16 / fp16 operands widened exactly; for the fp16 form the fp32 queries rounded to fp16 first), outputs
pre-filled with NaN, sentinels around every output slice that must survive bit for bit, inputs surrounded by NaN wherever the kernel has
no business reading, every measured ratio printed before anything is asserted.

Error model of attention_d64, per output element O[q, d].  s_j = float64 scores in exp2 units, P_j = 2^(s_j - max) / sum,
T = sum_j P_j |v_jd|, A = sum_j P_j |v_jd - O|, E = max_j c sum_d |q_d| |k_jd| (c = scale log2 e, or 1 for pre-scaled queries):

  |O_kernel - O| <= 1/2 ulp_bf16(O)                     the result is rounded to nearest
                  + kappa u_P T                         P is rounded to bf16 (u_P = 2^-8) or fp16 (u_P = 2^-11) before P.V while l sums
                                                        the unrounded p: every p_j moves by at most u_P / 2 of itself, so kappa <= 1/2 to
                                                        first order; kappa = 1 is asserted (derived, not measured)
                  + k 2^-24 (T + E A)                   fp32 score accumulation (a score error e moves O by ln 2 e A), v_exp_f32, the fp32
                                                        sums of the numerator and of l, the combine pass
                  + [fp16 form] 2^-25 sum_j |v_jd| / L  p below 2^-14 is subnormal in fp16 (absolute error 2^-25 each); L = sum_j
                                                        2^(s_j - max) >= 1, and the kernel's lazy reference max never exceeds the row max
  (an O_kernel on the far side of a power of two is rounded on a grid twice as wide; it is then more than one ulp(O) away from O, which the
  kappa term covers: kappa' u_P T > ulp(O) with the true kappa' <= 0.65 leaves (1 - kappa') u_P T > ulp(O) / 2.)
The kappa term would hide a truncating P conversion, so the mean SIGNED error of every random case, in units of u_P T, is bounded too
(truncation gives about -0.3).

The fused sub-blocks, per element of part[h][row][n] against float64 sum_d O_d Wo[n, 64h + d]:
  sum_d (ulp_bf16(O_d) + u_P T_d + K_FP32 2^-24 (T_d + E A_d)) |Wo|  +  k 2^-24 sum_d |O_d| |Wo|
  fp16 slabs: + one fp16 ulp of value 2^-6 (2^-18 absolute below the normal range, in units of the value)
  xattn_q2_proj: + ln 2 D 2^(2 D) A_d per O_d, D = max_j sum_d (2^-8 |q_d| + 2^-21 qscale sum_c |h_c| |Wq_dc|) |k_jd|: q = qscale h Wq^T is
  summed in fp32 (four partial sums of 128 products: the 2^-21 term, eight fp32 roundings at the size of the absolute sum) and rounded to
  bf16 (2^-8 |q_d| is twice the rounding); a score error e_j moves P_j by the factor 2^(e_j) and the normaliser by at most 2^D, hence the
  second-order factor 2^(2 D) on the first-order ln 2 D A.
reduce_resid_ln over eight fp16 slabs: x against float64 on the widened slabs within k 2^-24 (sum_s |part_s| + |bias| + |x_old|); h within
the bound of test_gpu_resid_ln.py (one bf16 ulp + k 2^-24 T).

Measured on an MI355X against these float64 references (the bounds below are at most 2.5 x the worst value), worst over the random and
the key-split cases of each instantiation <PRESCALED, VROW>:
                                     <0,0>     <1,0>     <0,1>     <1,1>     fp16
  kappa with k = 0                   0.826     0.823     0.817     0.811     0.763      (asserted: kappa = 1)
  k with kappa = 1                   0         0         0         0         0          (K_FP32 = 0: the kappa = 1 allowance already covers
                                                                                         the fp32 arithmetic; the term stays in the formula)
  |mean signed error| / (u_P T)      0.0064    0.0041    0.0054    0.0046    0.053      (BIAS; in the fp16 form the unit 2^-11 T is a quarter of
                                                                                         the result's own bf16 rounding, which is what is left)
  |split - unsplit| / (2 bound)      0.49      -         -         0.48      0.87
  slabs: error / allowance 0.12 - 0.124 (attn_self_proj), 0.092 - 0.128 (xattn_q2_proj; D up to 0.235 exp2 units), k = 0 (K_PART = 0)
  reduce over eight fp16 slabs: k 1.75 for x (0 on integers), 0.115 for h

What reaches what:
  attention_d64_kernel<0,0> (own scale, Vt)        random, one-hot, uniform, split     test_attention_random_per_element[plain], test_attention_exact[plain],
  attention_d64_kernel<1,0> (pre-scaled, Vt)       random, one-hot, uniform            ...[pre]            test_attention_key_split[plain]
  attention_d64_kernel<0,1> (own scale, row V)     random, one-hot, uniform            ...[vrow]
  attention_d64_kernel<1,1> (pre-scaled, row V)    random, one-hot, uniform, split     ...[pre_vrow], test_attention_key_split[pre_vrow]
  attention_d64_kernel<1,1,1> (fp16, fp32 q)       random, one-hot, uniform, split     ...[f16], test_attention_key_split[f16]
  attention_combine_kernel                          ksplit 2, 3, 5, 16, 17, 40, 64, -1  test_attention_key_split (per element + uniform), test_attention_exact (one-hot, ksplit 3)
  nq 32 / 96 / 128 / 160, nk 1 .. 192, ragged first tile, XCD remap on / off, q|k|v slices of one buffer, O slice, spare rows, strideQ 0,
  hsk 0 (bf16 Vt and bf16 row-major), v_padded with bf16                               test_attention_random_per_element (CASES)
  attn_self_proj fp32 / fp16 slabs                  random, one-hot                     test_self_proj_per_element, test_self_proj_exact
  xattn_q2_proj fp32 / fp16 slabs                   random, one-hot                     test_xattn_per_element, test_xattn_exact
  store_part_tile saturation + counter                                                  test_fp16_slab_saturation_counts_and_clamps
  reduce_resid_ln_kernel<8, fp16>                   random, integers                    test_reduce_eight_fp16_slabs
  argument checks (CPU)                                                                 test_attention_argument_checks_refuse_before_any_launch"""
import math
import time

import pytest
import torch

from test_gpu_resid_ln import SENT, U, _bits, _Checks, _g, _guard_ok, _guarded, _ratio, _ratio16

gpu = pytest.mark.gpu
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
DEV = "cuda"

# bounds (module docstring: measured values)
KAPPA = 1.0                                    # derived
K_FP32 = 0.0                                   # k of the fp32 term of attention_d64: measured 0 in every case
BIAS = {"bf16": 0.016, "f16": 0.133}           # |mean signed error| in units of u_P T (floor 3 / sqrt(elements)): measured 0.0064, 0.053
K_PART = 0.0                                   # k of the fp32 term of the slabs: measured 0
K_REDUCE_X, K_REDUCE_H = 4.3, 0.28             # measured 1.75, 0.115

FORMS = {"plain": dict(pre=False, vrow=False, f16=False), "pre": dict(pre=True, vrow=False, f16=False),
         "vrow": dict(pre=False, vrow=True, f16=False), "pre_vrow": dict(pre=True, vrow=True, f16=False),
         "f16": dict(pre=True, vrow=True, f16=True)}
RAMP = (0.0, 7.9, 16.0, 316.0, 300.0, 20.0, 27.9, 36.0)      # per key tile, exp2 units at slope 1: +7.9, +8.1, +300, then falling


@pytest.fixture(scope="module")
def H():
    from rald_amd import _handles
    return _handles


@pytest.fixture(autouse=True)
def _timed(request):
    t = time.perf_counter()
    yield
    print(f"time {request.node.name}: {time.perf_counter() - t:.2f} s")


def _ulp16(ref):
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)


def _round_to(t, dtype):
    return t.to(dtype).double()


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def _required_keys(nk, nq, ksplits=()):
    """the keys that must each dominate some query: all of them when nk <= nq, else the first and last key of every tile and of every
    split range, nk-1, nk-2 and one key per 4-key register group"""
    if nk <= nq:
        return list(range(nk))
    nt = -(-nk // 64)
    keys = []
    for t in range(nt):
        keys += [64 * t, min(64 * t + 63, nk - 1)]
    for ks in ksplits:
        per = -(-nt // ks)
        for s in range(ks):
            if s * per < nt:
                keys += [64 * s * per, min(64 * min((s + 1) * per, nt) - 1, nk - 1)]
    keys += [nk - 1, max(nk - 2, 0)]
    keys += [min(4 * g + g % 4, nk - 1) for g in range(-(-nk // 4))]
    return list(dict.fromkeys(keys))


def _attn_data(form, nq, nk, Hn, B, seed, hsk0=False, shared_q=False, ksplits=(), strict=True):
    """Q [B,H,nq,64], K / V [B,Hk,nk,64] (Hk = 1 with hsk0) in float64, already rounded to the operand type, and c.  Row kinds:
    flat (q ~ 2^-6), moderate (score std 3), peaked (one dominant key, 64 exp2 units over the rest), ramp (column 0 of K carries RAMP per tile,
    the query +-1 or 0.5 in it).  Column 1 is the pad trap: every query holds 2^-3 / c there, every real key 0."""
    f = FORMS[form]
    dt = torch.float16 if f["f16"] else torch.bfloat16
    c = 1.0 if f["pre"] else 0.125 * LOG2E
    g = _g(seed)
    Hk, Bq = (1 if hsk0 else Hn), (1 if shared_q else B)
    K = torch.randn(B, Hk, nk, 64, generator=g, dtype=torch.float64)
    ramp = torch.tensor(RAMP, dtype=torch.float64)[(torch.arange(nk) // 64) % 8]
    K[..., 0] = ramp + 0.5 * torch.rand(B, Hk, nk, generator=g, dtype=torch.float64)
    K[..., 1] = 0.0
    K = _round_to(K, dt)
    V = _round_to(torch.randn(B, Hk, nk, 64, generator=g, dtype=torch.float64) + 0.75, dt)
    need = _required_keys(nk, nq, ksplits)
    n_pk = min(max(nq // 4, -(-len(need) // (Bq * Hn))), nq - 3)
    perm = torch.randperm(nq, generator=g)
    Q = torch.zeros(Bq, Hn, nq, 64, dtype=torch.float64)
    covered, p = set(), 0
    for b in range(Bq):
        for h in range(Hn):
            rows = perm[torch.randperm(nq, generator=g)]
            kb = K[b if not shared_q else 0, 0 if hsk0 else h]
            for i, q in enumerate(rows.tolist()):
                if i < n_pk:                                                   # peaked
                    j = need[p % len(need)]
                    p += 1
                    covered.add(j)
                    kj = kb[j].clone()
                    kj[0] = 0.0
                    Q[b, h, q] = kj * (64.0 / (c * float(kj @ kj)))
                else:
                    kind = (i - n_pk) % 3
                    if kind == 0:                                              # flat
                        Q[b, h, q] = torch.randn(64, generator=g, dtype=torch.float64) * 2.0 ** -6
                    elif kind == 1:                                            # moderate
                        Q[b, h, q] = torch.randn(64, generator=g, dtype=torch.float64) * (3.0 / (8.0 * c))
                    else:                                                      # ramp
                        Q[b, h, q] = torch.randn(64, generator=g, dtype=torch.float64) * (1.0 / (8.0 * c))
                    Q[b, h, q, 0] = (1.0, -1.0, 0.5)[i % 3] / c if kind == 2 else 0.0
    Q[..., 1] = 2.0 ** -3 / c
    assert not strict or covered == set(need), (len(covered), len(need))
    if f["f16"]:
        Q32 = Q.float()                                                        # what the kernel is given
        Qr = Q32.half().double()                                               # ... and what it computes with
    else:
        Q32 = None
        Qr = _round_to(Q, torch.bfloat16)
    return dict(form=form, nq=nq, nk=nk, H=Hn, B=B, c=c, Q=Qr, Q32=Q32, K=K, V=V, hsk0=hsk0, shared_q=shared_q, dt=dt,
                scale=0.125, **f)


def _attn_ref(d):
    """float64 O, T, A, E and the fp16 subnormal term, each [B, nq, H*64] (E broadcast over d)"""
    B, Hn, nq, nk = d["B"], d["H"], d["nq"], d["nk"]
    O = torch.empty(B, nq, Hn * 64, dtype=torch.float64)
    T, A, E, sub = torch.empty_like(O), torch.empty_like(O), torch.empty_like(O), torch.zeros_like(O)
    for b in range(B):
        for h in range(Hn):
            q = d["Q"][0 if d["shared_q"] else b, h]
            k, v = d["K"][b, 0 if d["hsk0"] else h], d["V"][b, 0 if d["hsk0"] else h]
            s = d["c"] * (q @ k.t())
            w = torch.exp2(s - s.amax(1, keepdim=True))
            L = w.sum(1, keepdim=True)
            P = w / L
            o = P @ v
            sl = slice(64 * h, 64 * h + 64)
            O[b, :, sl], T[b, :, sl] = o, P @ v.abs()
            for q0 in range(0, nq, 32):
                A[b, q0:q0 + 32, sl] = (P[q0:q0 + 32, :, None] * (v[None] - o[q0:q0 + 32, None]).abs()).sum(1)
            E[b, :, sl] = (d["c"] * (q.abs() @ k.abs().t())).amax(1, keepdim=True)
            if d["f16"]:
                sub[b, :, sl] = 2.0 ** -25 * v.abs().sum(0, keepdim=True) / L
    return dict(O=O, T=T, A=A, E=E, sub=sub)


def _embed(val, rows, col0, width, dtype, fill):
    """val [B, r, c] into a device buffer [B, rows, width] of `fill` at column col0; returns (buffer, view of the r x c block)"""
    B, r, cc = val.shape
    buf = torch.full((B, rows, width), fill, dtype=dtype)
    buf[:, :r, col0:col0 + cc] = val.to(dtype)
    buf = buf.to(DEV)
    return buf, buf[:, :r, col0:col0 + cc]


def _flat_heads(x):
    """[B, H, n, 64] -> [B, n, H*64]"""
    B, Hn, n, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, n, Hn * 64)


def _run_attention(Hh, d, layout="plain", ksplit=0, kpad="trap"):
    """one launch of rald_op_attention_args on the case's data in the given memory layout; returns O [B, nq, H*64] on the CPU after
    checking the sentinels.  Layouts: 'plain' (contiguous operands), 'fused' (q | k | v, or q | k, as column slices of one buffer), 'spare'
    (every operand a column slice of its own wider buffer with spare rows between the samples).  Around the operands everything is NaN."""
    B, Hn, nq, nk, dt = d["B"], d["H"], d["nq"], d["nk"], d["dt"]
    HD, KD = Hn * 64, (64 if d["hsk0"] else Hn * 64)
    k_rows = -(-nk // 64) * 64
    padded = d["vrow"] and nk % 64 != 0
    nan = float("nan")
    # K with its pad rows: the trap (column 1 = 2^20, or 2^15 in fp16: an admitted pad key wins every softmax by thousands of exp2
    # units); the shared fp16 key / value rows have a zero pad by contract
    Kf = torch.zeros(B, k_rows, KD, dtype=torch.float64)
    Kf[:, :nk] = _flat_heads(d["K"])
    if kpad == "trap":
        Kf[:, nk:, 1::64] = 2.0 ** 15 if d["f16"] else 2.0 ** 20
    Qsrc = d["Q32"] if d["f16"] else d["Q"]
    Qf = _flat_heads(Qsrc)
    qdt = torch.float32 if d["f16"] else torch.bfloat16
    if d["vrow"]:
        Vf = torch.zeros(B, k_rows if padded else nk, KD, dtype=torch.float64)          # row-major pad: zero (the contract)
        Vf[:, :nk] = _flat_heads(d["V"])
    else:
        Vf = torch.full((B, KD, k_rows), 1e30, dtype=torch.float64)                     # Vt pad columns: large and finite
        Vf[:, :, :nk] = _flat_heads(d["V"]).transpose(1, 2)
    keep = []
    if layout == "fused" and not d["f16"]:
        rows = max(nq, k_rows) + 5
        parts = [Qf, Kf] + ([Vf] if d["vrow"] else [])
        width = sum(p.shape[2] for p in parts) + 16
        buf = torch.full((B, rows, width), nan, dtype=dt)
        views, c0 = [], 8
        for p in parts:
            buf[:, :p.shape[1], c0:c0 + p.shape[2]] = p.to(dt)
            views.append((p.shape[1], c0, p.shape[2]))
            c0 += p.shape[2]
        buf = buf.to(DEV)
        keep.append(buf)
        vs = [buf[:, :r, a:a + w] for r, a, w in views]
        Qv, Kv = vs[0], vs[1]
        Vv = vs[2] if d["vrow"] else _embed(Vf, KD + 3, 8, k_rows + 24, dt, nan)[1]
    elif layout == "spare":
        Qv = _embed(Qf, nq + 7, 8, HD + 24, qdt, nan)[1]
        Kv = _embed(Kf, k_rows + 3, 16, KD + 24, dt, nan)[1]
        Vv = _embed(Vf, Vf.shape[1] + 2, 8, Vf.shape[2] + 16, dt, nan)[1]
    else:
        Qv = _embed(Qf, nq, 0, HD, qdt, nan)[1]
        Kv = _embed(Kf, k_rows, 0, KD, dt, nan)[1]
        Vv = _embed(Vf, Vf.shape[1], 0, Vf.shape[2], dt, nan)[1]
    # O: a column slice of a wider buffer with spare rows; the slice NaN, everything else the sentinel
    obuf = torch.full((B, nq + 3, HD + 128), SENT, dtype=torch.bfloat16, device=DEV)
    Ov = obuf[:, :nq, 64:64 + HD]
    Ov.fill_(nan)
    scratch = None
    from rald_amd._lib import lib
    eff = ksplit if ksplit >= 0 else lib().rald_op_attention_pick_ksplit(nq, nk, Hn, B)
    if eff > 1:
        n = eff * B * Hn * nq * 66
        scratch = _guarded(n, 1024)
    Hh.op_attention_args(Ov, Kv, nq, nk, Hn, k_rows, Q=None if d["f16"] else Qv, Qf=Qv if d["f16"] else None, Vt=None if d["vrow"] else Vv,
                         V=Vv if d["vrow"] else None, scale=d["scale"], q_prescaled=d["pre"], f16=d["f16"], hsk=0 if d["hsk0"] else 64,
                         v_padded=padded, ksplit=ksplit, scratch=scratch, strideQ=0 if d["shared_q"] else None)
    torch.cuda.synchronize()
    out = obuf.cpu()
    inner = out[:, :nq, 64:64 + HD].clone()
    out[:, :nq, 64:64 + HD] = SENT
    assert torch.equal(_bits(out), _bits(torch.full_like(out, SENT))), "attention wrote outside its output slice"
    if scratch is not None:
        assert _guard_ok(scratch, n), "split scratch: guard tail overwritten"
    return inner


def _bound(ref, uP, k=K_FP32, kappa=KAPPA):
    return 0.5 * _ulp16(ref["O"]) + ref["sub"] + kappa * uP * ref["T"] + k * U * (ref["T"] + ref["E"] * ref["A"])


def _measure(chk, name, got, ref, uP, bias_key=None):
    """prints measured kappa (k = 0), k (kappa = 1) and the signed bias; asserts kappa = 1 with K_FP32, and the bias"""
    err = got.double() - ref["O"]
    bad = torch.isnan(err)
    ae = torch.where(bad, torch.full_like(err, math.inf), err.abs())
    base = 0.5 * _ulp16(ref["O"]) + ref["sub"]
    T = ref["T"].clamp_min(2.0 ** -126)
    kappa = float(((ae - base).clamp_min(0) / (uP * T)).max())
    kk = float(((ae - base - KAPPA * uP * T).clamp_min(0) / (U * (T + ref["E"] * ref["A"]).clamp_min(2.0 ** -126))).max())
    print(f"measured {name}: kappa {kappa:.3g} (with k = 0)")
    chk.le(f"{name} k (kappa = 1)", kk, K_FP32)
    if bias_key is not None:
        bias = float((torch.where(bad, torch.zeros_like(err), err) / (uP * T)).mean())
        chk.le(f"{name} |bias| ({bias:+.3g})", abs(bias), max(BIAS[bias_key], 3.0 / math.sqrt(err.numel())))
    return kappa


# (nq, nk, heads, batch, layout, hsk0) per form.  Every nq, every nk, every (heads, batch) and every layout at least once per form.
def _cases(form):
    f = FORMS[form]
    hb = [(8, 3), (1, 1), (3, 1), (2, 3), (8, 1), (4, 2)]      # (nk = 1 gives one output row per (sample, head): it gets the most of them)
    nks = [1, 31, 32, 33, 63, 64, 65, 128, 130, 192]
    nqs = [32, 96, 128, 160]
    lay = ["plain", "fused", "spare"]
    out = []
    for i, nk in enumerate(nks):
        Hn, B = hb[i % 6]
        nq = 160 if Hn * B % 8 == 0 else nqs[i % 3]                   # XCD remap active: nq = 160 so nx = 2
        out.append((nq, nk, Hn, B, lay[i % 3], False))
    out += [(128, 64, 8, 1, "fused", False), (96, 192, 2, 3, "spare", False)]
    if f["vrow"]:                                                      # the unpadded row-major V (v_padded = 0) is in the list: nk 64, 128, 192
        out.append((32, 128, 3, 1, "plain", False))
    if not f["f16"]:
        out.append((96, 130 if not f["vrow"] else 65, 3, 1, "spare", True))        # hsk = 0 on the bf16 forms
        out.append((32, 64, 8, 1, "plain", True))
    return out


# ---- attention_d64 ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_attention_random_per_element(H, form):
    """Every case of _cases(form) per element against float64 with kappa = 1 and K_FP32, and the signed bias of each case.  The fp16 form
    also runs with the queries shared between the samples (strideQ = 0) and key = value rows with a zero pad (hsk = 0: the product's form)."""
    chk = _Checks()
    uP = 2.0 ** -11 if FORMS[form]["f16"] else 2.0 ** -8
    worst = 0.0
    for i, (nq, nk, Hn, B, layout, hsk0) in enumerate(_cases(form)):
        d = _attn_data(form, nq, nk, Hn, B, 100 * len(form) + i, hsk0=hsk0)
        got = _run_attention(H, d, layout)
        worst = max(worst, _measure(chk, f"{form} nq {nq} nk {nk} {Hn}x{B} {layout}{' hsk0' if hsk0 else ''}", got, _attn_ref(d), uP,
                                    "f16" if FORMS[form]["f16"] else "bf16"))
    if form == "f16":
        for nq, nk, Hn, B in ((96, 130, 2, 3), (160, 63, 8, 1)):
            d = _attn_data(form, nq, nk, Hn, B, 900 + nk, hsk0=True, shared_q=True)
            d["V"] = d["K"]                                            # one fp16 row per key: key and value of every head
            got = _run_attention(H, d, "plain", kpad="zero")
            worst = max(worst, _measure(chk, f"f16 shared rows nq {nq} nk {nk} {Hn}x{B} strideQ 0", got, _attn_ref(d), uP, "f16"))
    chk.le(f"{form} kappa (k = 0), informative", worst, math.inf)
    chk.done()


def _pair(j):
    return j % 64, (j % 64 + 1 + j // 64) % 64


def _one_hot(form, nq, nk, Hn, B, seed):
    """key j holds 16 on the two dimensions of its own pair and 0 elsewhere, query i holds 16 / c' on the pair of key sel(i): its score is
    512 exp2 units, 256 over every other key, so P is exactly one-hot and O = V[sel] (integers) bit for bit"""
    d = _attn_data(form, nq, nk, Hn, B, seed, strict=False)
    g = _g(seed + 1)
    K = torch.zeros_like(d["K"])
    for j in range(nk):
        a, b2 = _pair(j)
        K[:, :, j, a] = 16.0
        K[:, :, j, b2] = 16.0
    sel = torch.randint(0, nk, (B, Hn, nq), generator=g)
    sel[..., 0], sel[..., nq - 1] = nk - 1, 0
    Q = torch.zeros_like(d["Q"])
    qv = 16.0 if d["pre"] else 128.0                                   # own scale: c = 0.125 log2 e, scores 512 log2 e
    for b in range(B):
        for h in range(Hn):
            for i in range(nq):
                a, b2 = _pair(int(sel[b, h, i]))
                Q[b, h, i, a] = qv
                Q[b, h, i, b2] = qv
    V = torch.randint(-8, 9, d["V"].shape, generator=g).double()
    d.update(Q=Q, Q32=Q.float(), K=K, V=V)
    want = torch.stack([torch.stack([V[b, h][sel[b, h]] for h in range(Hn)], 1) for b in range(B)]).reshape(B, nq, Hn * 64)
    return d, want


def _uniform(form, nq, nk, Hn, B, seed):
    """q = 0 and integer V whose column means are integers c, 1 <= |c| <= 4, every key at least 64 away from c (nk >= 2): O = c exactly"""
    d = _attn_data(form, nq, nk, Hn, B, seed, strict=False)
    g = _g(seed + 2)
    shp = d["V"].shape[:2]
    c = torch.randint(1, 5, (*shp, 1, 64), generator=g).double() * (torch.randint(0, 2, (*shp, 1, 64), generator=g).double() * 2 - 1)
    dev = torch.zeros(*shp, nk, 64, dtype=torch.float64)
    npair = (nk - (3 if nk % 2 else 0)) // 2 if nk >= 2 else 0
    if npair:
        r = torch.randint(64, 121, (*shp, npair, 64), generator=g).double() * (torch.randint(0, 2, (*shp, npair, 64), generator=g).double() * 2 - 1)
        dev[:, :, 0:2 * npair:2], dev[:, :, 1:2 * npair:2] = r, -r
    if nk % 2 and nk >= 3:
        a = torch.randint(64, 121, (*shp, 2, 64), generator=g).double()
        sg = torch.randint(0, 2, (*shp, 1, 64), generator=g).double() * 2 - 1
        dev[:, :, nk - 3:nk - 1] = a * sg
        dev[:, :, nk - 1] = -(a.sum(2)) * sg[:, :, 0]
    V = c + dev
    assert float(V.abs().max()) <= 256 and torch.equal(V.mean(2, keepdim=True), c.expand_as(V.mean(2, keepdim=True)))
    d.update(Q=torch.zeros_like(d["Q"]), Q32=torch.zeros_like(d["Q"]).float(), V=V)
    return d, _flat_heads(c.expand(d["B"], Hn, nq, 64))


@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_attention_exact(H, form):
    """bit-equal results on every instantiation: the one-hot softmax (pins key <-> accumulator row of both MFMAs and of the transposed
    read) unsplit and through the combine pass, and the uniform softmax (every key counts once: a dropped or an admitted key is a wrong
    integer) at ragged nk, with the XCD remap, unsplit and split."""
    chk = _Checks()
    for nq, nk, Hn, B, layout, ks in ((32, 33, 1, 1, "plain", 0), (160, 192, 8, 1, "fused", 0), (96, 130, 2, 3, "spare", 0),
                                      (160, 1000, 4, 2, "plain", 3), (128, 961, 1, 1, "spare", 16)):
        d, want = _one_hot(form, nq, nk, Hn, B, 7000 + nk)
        got = _run_attention(H, d, layout, ksplit=ks)
        chk.true(f"one-hot {form} nq {nq} nk {nk} {Hn}x{B} ksplit {ks}: {int((got.double() != want).sum())} wrong", torch.equal(got.double(), want))
    for nq, nk, Hn, B, layout, ks in ((32, 1, 1, 1, "plain", 0), (96, 31, 3, 1, "spare", 0), (160, 65, 8, 1, "fused", 0), (128, 130, 2, 3, "plain", 0),
                                      (160, 192, 4, 2, "spare", 0), (160, 1000, 8, 1, "plain", 5), (96, 961, 3, 1, "spare", 17),
                                      (128, 1024, 1, 1, "plain", -1)):
        d, want = _uniform(form, nq, nk, Hn, B, 7500 + nk)
        got = _run_attention(H, d, layout, ksplit=ks)
        chk.true(f"uniform {form} nq {nq} nk {nk} {Hn}x{B} ksplit {ks}: {int((got.double() != want).sum())} wrong", torch.equal(got.double(), want))
    chk.done()


@gpu
@pytest.mark.parametrize("form", ["plain", "pre_vrow", "f16"])
@pytest.mark.parametrize("nk,nq,Hn,B", [(1024, 160, 4, 2), (1000, 160, 8, 1), (961, 96, 3, 1)])
def test_attention_key_split(H, form, nk, nq, Hn, B):
    """The keys split over ksplit workgroups + attention_combine_kernel: ksplit 2, 3, 5, 16, 17, 40, 64 (5, 17, 40, 64 leave empty ranges; 961
    keys leave one key in the last tile), each per element within the same bound as the single pass, and within the sum of both bounds of
    the single pass.  ksplit = -1 on nq = 128, one head, batch 1, 16 tiles, where attention_pick_ksplit returns 4."""
    from rald_amd._lib import lib
    chk = _Checks()
    uP = 2.0 ** -11 if FORMS[form]["f16"] else 2.0 ** -8
    kss = (2, 3, 5, 16, 17, 40, 64)
    d = _attn_data(form, nq, nk, Hn, B, 3000 + nk + len(form), ksplits=kss)
    ref = _attn_ref(d)
    bound = _bound(ref, uP)
    base = _run_attention(H, d, "plain")
    _measure(chk, f"{form} nk {nk} unsplit", base, ref, uP, "f16" if FORMS[form]["f16"] else "bf16")
    for i, ks in enumerate(kss):
        got = _run_attention(H, d, ("plain", "spare")[i % 2], ksplit=ks)
        _measure(chk, f"{form} nk {nk} ksplit {ks}", got, ref, uP, "f16" if FORMS[form]["f16"] else "bf16")
        diff = (got.double() - base.double()).abs()
        chk.le(f"{form} nk {nk} ksplit {ks} |split - unsplit| / (2 bound)", float((torch.where(torch.isnan(diff), torch.full_like(diff, math.inf), diff) / (2 * bound)).max()), 1.0)
    assert lib().rald_op_attention_pick_ksplit(128, nk, 1, 1) == 4
    d = _attn_data(form, 128, nk, 1, 1, 3500 + nk, ksplits=(4,), strict=False)
    got = _run_attention(H, d, "plain", ksplit=-1)
    _measure(chk, f"{form} nk {nk} ksplit -1 (4)", got, _attn_ref(d), uP, "f16" if FORMS[form]["f16"] else "bf16")
    chk.done()


# ---- attn_self_proj / xattn_q2_proj ----------------------------------------------------------------------------------------------------
def _slab_buffer(heads, M, f16):
    """[heads][M][512] slabs, NaN, inside a buffer with a sentinel block before and behind"""
    dt = torch.float16 if f16 else torch.float32
    n = heads * M * 512
    buf = torch.full((n + 4096,), SENT, dtype=dt, device=DEV)
    buf[2048:2048 + n] = float("nan")
    return buf, buf[2048:2048 + n].view(heads, M, 512)


def _slab_read(buf, heads, M):
    n = heads * M * 512
    out = buf.cpu()
    ok = torch.equal(_bits(out[:2048]), _bits(torch.full_like(out[:2048], SENT))) and torch.equal(_bits(out[2048 + n:]), _bits(torch.full_like(out[2048 + n:], SENT)))
    assert ok, "slabs: sentinel overwritten"
    v = out[2048:2048 + n].view(heads, M, 512).double()
    return v * 64.0 if buf.dtype == torch.float16 else v


def _part_check(chk, name, got, O, allowO, Wo, f16, extra_abs=None):
    """got [8][M][512] (value units) against sum_d O_d Wo[n, 64h+d]: allowance sum_d (ulp16(O_d) + allowO_d) |Wo| (+ the fp16 slab rounding);
    prints the fraction of the allowance used and k of the remaining fp32 term"""
    M = O.shape[0]
    Wd = Wo.double()
    worst_k, worst_f = 0.0, 0.0
    for h in range(8):
        o, w = O[:, 64 * h:64 * h + 64], Wd[:, 64 * h:64 * h + 64]
        ref = o @ w.t()
        allow = (_ulp16(o) + allowO[:, 64 * h:64 * h + 64]) @ w.abs().t()
        if f16:
            allow = allow + 64.0 * torch.exp2(torch.floor(torch.log2((ref.abs() / 64.0).clamp_min(2.0 ** -14))) - 10)
        if extra_abs is not None:
            allow = allow + extra_abs
        terms = o.abs() @ w.abs().t()
        err = (got[h] - ref).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
        worst_k = max(worst_k, float(((err - allow).clamp_min(0) / (U * terms.clamp_min(2.0 ** -126))).max()))
        worst_f = max(worst_f, float((err / allow.clamp_min(2.0 ** -126)).max()))
    print(f"measured {name}: error / allowance {worst_f:.3g}")
    chk.le(f"{name} k", worst_k, K_PART)


def _self_data(B, ld, seed):
    """fused q|k|v rows [B*512][ld] (q pre-scaled, exp2 units): per head the four row kinds; peaked rows dominate the first and last key of
    each of the eight waves' tiles; ramp rows see per-tile maxima 160 exp2 units apart (column 0 of K = 160 x tile), so the merge weights
    underflow to zero"""
    g = _g(seed)
    NL, D = 512, 512
    K = torch.randn(B, 8, NL, 64, generator=g, dtype=torch.float64)
    K[..., 0] = 160.0 * (torch.arange(NL) // 64).double() + 0.5 * torch.rand(B, 8, NL, generator=g, dtype=torch.float64)
    K = _round_to(K, torch.bfloat16)
    V = _round_to(torch.randn(B, 8, NL, 64, generator=g, dtype=torch.float64) + 0.75, torch.bfloat16)
    Q = torch.zeros(B, 8, NL, 64, dtype=torch.float64)
    edge = [64 * w for w in range(8)] + [64 * w + 63 for w in range(8)]
    for b in range(B):
        for h in range(8):
            rows = torch.randperm(NL, generator=g).tolist()
            for i, q in enumerate(rows):
                kind = i % 4
                if kind == 0:
                    kj = K[b, h, edge[(i // 4) % 16]].clone()
                    kj[0] = 0.0
                    Q[b, h, q] = kj * (64.0 / float(kj @ kj))
                elif kind == 1:
                    Q[b, h, q] = torch.randn(64, generator=g, dtype=torch.float64) * 2.0 ** -6
                elif kind == 2:
                    Q[b, h, q] = torch.randn(64, generator=g, dtype=torch.float64) * (3.0 / 8.0)
                else:
                    Q[b, h, q] = torch.randn(64, generator=g, dtype=torch.float64) / 8.0
                Q[b, h, q, 0] = (1.0, -1.0)[(i // 4) % 2] if kind == 3 else 0.0
    Q = _round_to(Q, torch.bfloat16)
    Wo = _round_to(torch.randn(D, D, generator=g, dtype=torch.float64) / 22.0, torch.bfloat16)
    return dict(form="pre_vrow", nq=NL, nk=NL, H=8, B=B, c=1.0, Q=Q, K=K, V=V, Wo=Wo, hsk0=False, shared_q=False, f16=False, ld=ld)


def _self_launch(Hh, d, f16):
    B, ld = d["B"], d["ld"]
    rows = torch.cat([_flat_heads(d["Q"]), _flat_heads(d["K"]), _flat_heads(d["V"])], 2).reshape(B * 512, 1536)
    qkv = torch.full((B * 512, ld), float("nan"), dtype=torch.bfloat16)
    qkv[:, :1536] = rows.bfloat16()
    qkv = qkv.to(DEV)
    buf, part = _slab_buffer(8, B * 512, f16)
    assert Hh.f16_saturation_attn(True) >= 0
    Hh.op_attn_self_proj(qkv, d["Wo"].bfloat16().to(DEV), part, 512, 8, B)
    return buf, _slab_read(buf, 8, B * 512), Hh.f16_saturation_attn(True)


@gpu
@pytest.mark.parametrize("B,ld,f16", [(1, 1536, False), (1, 1536, True), (3, 1536 + 64, False), (3, 1536 + 64, True)])
def test_self_proj_per_element(H, B, ld, f16):
    """attn_self_proj on 512 latents, batch 1 and 3, ld 1536 and a wider fused buffer, fp32 and fp16 slabs, per element of every slab"""
    chk = _Checks()
    d = _self_data(B, ld, 4100 + B)
    ref = _attn_ref(d)
    _, got, sat = _self_launch(H, d, f16)
    chk.true(f"saturation counter {sat}", sat == 0)
    allowO = 2.0 ** -8 * ref["T"] + K_FP32 * U * (ref["T"] + ref["E"] * ref["A"])
    _part_check(chk, f"self_proj B {B} ld {ld} {'fp16' if f16 else 'fp32'} slabs", got, ref["O"].reshape(B * 512, 512), allowO.reshape(B * 512, 512), d["Wo"], f16)
    chk.done()


def _ternary(seed):
    return torch.randint(-1, 2, (512, 512), generator=_g(seed)).double()


@gpu
@pytest.mark.parametrize("f16", [False, True])
def test_self_proj_exact(H, f16):
    """one-hot softmax over the 512 keys (pair construction of _one_hot), integer V in [-8, 8], Wo in {-1, 0, 1}: |part| <= 512, bit-equal in
    fp32 slabs and, because such integers times 2^-6 are exact in fp16, in fp16 slabs"""
    B = 3
    d, want = _one_hot("pre_vrow", 512, 512, 8, B, 4200)
    d.update(Wo=_ternary(4201), ld=1536)
    _, got, sat = _self_launch(H, d, f16)
    O = want.reshape(B * 512, 512)
    ref = torch.stack([O[:, 64 * h:64 * h + 64] @ d["Wo"][:, 64 * h:64 * h + 64].t() for h in range(8)])
    assert sat == 0
    assert torch.equal(got, ref), int((got != ref).sum())


def _xattn_data(M, NL, seed, exact=False):
    g = _g(seed)
    B, L, li = M // NL, 3, 1
    qscale = float(torch.tensor(0.125 * LOG2E, dtype=torch.float32)) if not exact else 1.0
    Wo = _ternary(seed + 3) if exact else _round_to(torch.randn(512, 512, generator=g, dtype=torch.float64) / 22.0, torch.bfloat16)
    if exact:
        # integer h (32 on the dimension of key sel(row), per head), Wq = I / 2: q = 16 e_sel exactly; key j = 16 e_j: score 256 against 0
        sel = torch.randint(0, 64, (M, 8), generator=g)
        sel[0], sel[M - 1] = 63, 0
        hin = torch.zeros(M, 512, dtype=torch.float64)
        hin[torch.arange(M)[:, None], 64 * torch.arange(8)[None] + sel] = 32.0
        Wq = 0.5 * torch.eye(512, dtype=torch.float64)
        K = (16.0 * torch.eye(64, dtype=torch.float64)).expand(B, 8, 64, 64).clone()
        V = torch.randint(-8, 9, (B, 8, 64, 64), generator=g).double()
    else:
        hin = _round_to(torch.randn(M, 512, generator=g, dtype=torch.float64), torch.bfloat16)
        hin[1::4] = _round_to(hin[1::4] * 2.0 ** -5, torch.bfloat16)                                # flat rows
        hin[2::4] = _round_to(hin[2::4] * 4.0, torch.bfloat16)                                      # sharply peaked rows
        Wq = _round_to(torch.randn(512, 512, generator=g, dtype=torch.float64) / 22.0, torch.bfloat16)
        K = _round_to(torch.randn(B, 8, 64, 64, generator=g, dtype=torch.float64), torch.bfloat16)
        V = _round_to(torch.randn(B, 8, 64, 64, generator=g, dtype=torch.float64) + 0.75, torch.bfloat16)
        sel = None
    return dict(M=M, NL=NL, B=B, L=L, li=li, qscale=qscale, hin=hin, Wq=Wq, Wo=Wo, K=K, V=V, sel=sel)


def _xattn_launch(Hh, x, f16):
    """the condition cache of a 3-block model, block 1: Kc [B*64][3*512], Vt [B][3*512][64]; the other blocks' entries are NaN"""
    B, L, li, M = x["B"], x["L"], x["li"], x["M"]
    Kc = torch.full((B, 64, L * 512), float("nan"), dtype=torch.bfloat16)
    Kc[:, :, li * 512:(li + 1) * 512] = _flat_heads(x["K"]).bfloat16()
    Vt = torch.full((B, L * 512, 64), float("nan"), dtype=torch.bfloat16)
    Vt[:, li * 512:(li + 1) * 512] = _flat_heads(x["V"]).transpose(1, 2).bfloat16()
    Kc, Vt = Kc.to(DEV), Vt.to(DEV)
    buf, part = _slab_buffer(8, M, f16)
    assert Hh.f16_saturation_attn(True) >= 0
    Hh.op_xattn_q2_proj(x["hin"].bfloat16().to(DEV), x["Wq"].bfloat16().to(DEV), Kc[:, :, li * 512:(li + 1) * 512], Vt[:, li * 512:(li + 1) * 512],
                        x["Wo"].bfloat16().to(DEV), part, x["NL"], x["qscale"])
    return buf, _slab_read(buf, 8, M), Hh.f16_saturation_attn(True)


@gpu
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("M,NL", [(32, 32), (96, 32), (512, 512), (1024, 256)])
def test_xattn_per_element(H, M, NL, f16):
    """xattn_q2_proj per element of every slab: the attention bound of the float64 q, the q-rounding term of the module docstring, the
    out-projection; cache slice li = 1 of a 3-block cache, sentinels around the slabs"""
    chk = _Checks()
    x = _xattn_data(M, NL, 4300 + M + NL)
    B = x["B"]
    q = x["qscale"] * (x["hin"] @ x["Wq"].t())                                                      # [M, 512] float64
    qabs = x["qscale"] * (x["hin"].abs() @ x["Wq"].abs().t())
    d = dict(B=B, H=8, nq=NL, nk=64, c=1.0, Q=q.view(B, NL, 8, 64).permute(0, 2, 1, 3), K=x["K"], V=x["V"], hsk0=False, shared_q=False, f16=False)
    ref = _attn_ref(d)
    dq = (2.0 ** -8 * q.abs() + 2.0 ** -21 * qabs).view(B, NL, 8, 64).permute(0, 2, 1, 3)           # [B, 8, NL, 64]
    Dl = torch.einsum("bhqd,bhkd->bhqk", dq, x["K"].abs()).amax(-1)                                 # [B, 8, NL]
    Dl = Dl.permute(0, 2, 1)[..., None].expand(B, NL, 8, 64).reshape(B, NL, 512)
    print(f"measured xattn M {M}: largest score allowance D {float(Dl.max()):.3g} exp2 units (second-order factor {2 ** (2 * float(Dl.max())):.3g})")
    allowO = 2.0 ** -8 * ref["T"] + K_FP32 * U * (ref["T"] + ref["E"] * ref["A"]) + LN2 * Dl * torch.exp2(2 * Dl) * ref["A"]
    _, got, sat = _xattn_launch(H, x, f16)
    chk.true(f"saturation counter {sat}", sat == 0)
    _part_check(chk, f"xattn M {M} NL {NL} {'fp16' if f16 else 'fp32'} slabs", got, ref["O"].reshape(M, 512), allowO.reshape(M, 512), x["Wo"], f16)
    chk.done()


@gpu
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("M,NL", [(96, 32), (1024, 256)])
def test_xattn_exact(H, M, NL, f16):
    """integer h, Wq = I / 2 (q exact in bf16: no q-rounding term), one-hot softmax over the 64 keys, integer V, Wo in {-1, 0, 1}: bit-equal"""
    x = _xattn_data(M, NL, 4400 + M, exact=True)
    _, got, sat = _xattn_launch(H, x, f16)
    b = torch.arange(M) // NL
    O = torch.cat([x["V"][b, h, x["sel"][:, h]] for h in range(8)], 1)                              # [M, 512]
    ref = torch.stack([O[:, 64 * h:64 * h + 64] @ x["Wo"][:, 64 * h:64 * h + 64].t() for h in range(8)])
    assert sat == 0
    assert torch.equal(got, ref), int((got != ref).sum())


@gpu
def test_fp16_slab_saturation_counts_and_clamps(H):
    """heads 0-3: V = +-2^17 per key and Wo = 1, so |part| = 64 x 2^17 = 8.4e6 > 65504 x 64: those fp16 slab values are clamped to +-65504 (no
    inf) and the counter counts their 4-element groups; heads 4-7 hold |V| = 8 and are not clamped.  The reading reset clears the counter,
    and the fp32 slabs of the same data are exact and count nothing."""
    B = 1
    d, _ = _one_hot("pre_vrow", 512, 512, 8, B, 4500)
    sg = torch.randint(0, 2, (B, 8, 512, 1), generator=_g(4501)).double() * 2 - 1
    V = (sg * 2.0 ** 17).expand(B, 8, 512, 64).clone()
    V[:, 4:] = (sg[:, 4:] * 8.0).expand(B, 4, 512, 64)
    d.update(V=V, Wo=torch.ones(512, 512, dtype=torch.float64), ld=1536)
    buf, got, sat = _self_launch(H, d, True)
    assert sat > 0 and H.f16_saturation_attn(True) == 0
    raw = buf[2048:2048 + 8 * 512 * 512].cpu().double()
    assert bool(torch.isfinite(raw).all()) and bool((raw.abs() <= 65504).all())
    _, got32, sat32 = _self_launch(H, d, False)
    assert sat32 == 0 and bool((got32[:4].abs() == 64 * 2.0 ** 17).all()) and bool((got32[4:].abs() == 512).all())
    big = got32.abs() >= 65504 * 64
    assert torch.equal(got[big], got32[big].sign() * 65504 * 64) and torch.equal(got[~big], got32[~big])
    assert sat == int(big.view(-1, 4).any(1).sum()), (sat, int(big.view(-1, 4).any(1).sum()))


@gpu
@pytest.mark.parametrize("kind", ["rand", "int"])
def test_reduce_eight_fp16_slabs(H, kind):
    """reduce_resid_ln_kernel<8, fp16>: x += bias + sum of eight fp16 slabs (2^-6 x the value) and the next AdaLN, M = 1000 (ragged last
    block of 4 rows), two modulation groups.  x per element against float64 of the widened slabs (integers: bit-equal), h within the
    bound of test_gpu_resid_ln.py."""
    chk = _Checks()
    g = _g(4600)
    M = 1000
    if kind == "int":
        part = torch.randint(-200, 201, (8, M, 512), generator=g).double()
        bias, x0 = torch.randint(-8, 9, (512,), generator=g).double(), torch.randint(-8, 9, (M, 512), generator=g).double()
    else:
        part = torch.randn(8, M, 512, generator=g, dtype=torch.float64) * 30.0
        part[:, 1::4] *= 2.0 ** -12                                   # rows whose slab values are subnormal in fp16 after the 2^-6
        bias, x0 = torch.randn(512, generator=g).double(), (torch.randn(M, 512, generator=g) * 2 + 0.5).double()
    ph = (part / 64.0).half()
    pv = ph.double() * 64.0                                            # exactly what the kernel widens
    mod = torch.randn(2, 1024, generator=g) * 0.5
    buf = torch.full((8 * M * 512 + 1024,), float("nan"), dtype=torch.float16)
    buf[:8 * M * 512] = ph.flatten()
    buf = buf.to(DEV)
    xb, hb = _guarded(M * 512, 2048), _guarded(M * 512, 2048, torch.bfloat16)
    xb[:M * 512] = x0.float().flatten().to(DEV)
    modd = torch.cat([mod, torch.full((1, 1024), float("nan"))]).to(DEV).flatten()
    H.op_reduce_resid_ln(buf[:8 * M * 512].view(8, M, 512), bias.float().to(DEV), xb[:M * 512].view(M, 512), hb, modd, modd[512:], gstride=1024,
                         rows_per_group=512, add_one=1.0)
    torch.cuda.synchronize()
    assert _guard_ok(xb, M * 512) and _guard_ok(hb, M * 512)
    x, h = xb[:M * 512].view(M, 512).cpu(), hb[:M * 512].view(M, 512).cpu()
    v = x0 + bias + pv.sum(0)
    tx = pv.abs().sum(0) + bias.abs() + x0.abs()
    if kind == "int":
        chk.true("x exact", torch.equal(x.double(), v))
    chk.le(f"reduce {kind} x", _ratio(x, v, tx), K_REDUCE_X)
    grp = torch.arange(M) // 512
    gg, bb = mod[grp, :512].double(), mod[grp, 512:].double()
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + 1e-5).rsqrt()
    href = (v - mean) * rstd * (1 + gg) + bb
    T = rstd * (1 + gg).abs() * ((v - mean).abs() * (1 + (v * v).mean(1, keepdim=True) / (var + 1e-5)) + v.abs().mean(1, keepdim=True)) + bb.abs()
    chk.le(f"reduce {kind} h", _ratio16(h, href, T), K_REDUCE_H)
    chk.done()


# ---- argument checks (CPU: each fires before the entry's first HIP call) ---------------------------------------------------------------
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


DUMMY = 1 << 20


def test_attention_argument_checks_refuse_before_any_launch(L_cpu):
    """every RALD_CHECK of attention_d64, attn_self_proj and xattn_q2_proj (and of the entries in front of them) on fake aligned pointers"""
    L, d = L_cpu, DUMMY

    def att(Q=d, Qf=None, ldq=512, K=d, ldk=512, k_rows=64, Vt=d, ldvt=64, V=None, ldv=0, O=d, ldo=512, nq=128, nk=64, heads=8, batch=1, pre=0,
            f16=0, hsk=64, v_padded=0, ksplit=0, scratch=None, sbytes=0):
        return L.rald_op_attention_args(Q, Qf, ldq, nq * ldq, K, ldk, k_rows * ldk, k_rows, Vt, ldvt, 512 * ldvt, V, ldv, k_rows * ldv, O, ldo, nq * ldo,
                                        nq, nk, heads, batch, 0.125, pre, f16, hsk, v_padded, ksplit, scratch, sbytes, None)

    _refused(L, att(nq=0), "empty problem")
    _refused(L, att(nq=100), "multiple of 32")
    _refused(L, att(ldq=516), "leading dimensions")
    _refused(L, att(ldk=516), "leading dimensions")
    _refused(L, att(ldo=516), "leading dimensions")
    _refused(L, att(nk=65), "rows allocated up to a multiple of 64")
    _refused(L, att(K=d + 8), "16-byte aligned")
    _refused(L, att(O=d + 8), "16-byte aligned")
    _refused(L, att(hsk=32), "64 columns apart")
    _refused(L, att(Q=None, Qf=d, f16=1, Vt=None, V=d, ldv=64, pre=0), "fp16 form")
    _refused(L, att(Q=None, Qf=d, f16=1, pre=1), "fp16 form")                       # Vt instead of a row-major V
    _refused(L, att(Q=None, Qf=d + 8, f16=1, Vt=None, V=d, ldv=64, pre=1), "fp16 form")
    _refused(L, att(Q=d + 8), "Q must be 16-byte aligned")
    _refused(L, att(Vt=None, V=d, ldv=64, nk=33), "row-major V")
    _refused(L, att(Vt=None, V=d, ldv=68), "row-major V")
    _refused(L, att(Vt=None, V=d + 8, ldv=64), "row-major V")
    _refused(L, att(Vt=d + 8), "Vt must be 16-byte aligned")
    _refused(L, att(ldvt=68), "Vt must be 16-byte aligned")
    _refused(L, att(nk=65, k_rows=128, ldvt=72), "Vt rows must be padded")
    _refused(L, att(ksplit=4, scratch=None, sbytes=1 << 40), "key split needs a scratch")
    _refused(L, att(ksplit=65, scratch=d, sbytes=1 << 40), "key split needs a scratch")
    _refused(L, att(ksplit=4, scratch=d + 4, sbytes=1 << 40), "key split needs a scratch")
    _refused(L, att(ksplit=4, scratch=d, sbytes=4 * 8 * 128 * 66 * 4 - 4), "scratch too small")
    _refused(L, att(nq=128 * 1024, heads=1024, batch=2048), "too many workgroups")
    _refused(L, att(Q=None), "one of Q")
    _refused(L, att(Q=d, Qf=d), "one of Q")
    _refused(L, att(V=d, ldv=64), "not both")
    _refused(L, att(Vt=None), "not both")
    _refused(L, att(f16=1), "fp32 queries belong to the fp16 form")

    def sp(qkv=d, ld=1536, Wo=d, part=d, NL=512, heads=8, batch=1, f16=0):
        return L.rald_op_attn_self_proj_slabs(qkv, ld, Wo, part, NL, heads, batch, f16, None)

    for f16 in (0, 1):
        _refused(L, sp(qkv=None, f16=f16), "bad arguments")
        _refused(L, sp(batch=0, f16=f16), "bad arguments")
        _refused(L, sp(batch=65536, f16=f16), "bad arguments")
        _refused(L, sp(heads=4, f16=f16), "8 heads")
        _refused(L, sp(ld=1528, f16=f16), "fused q|k|v")
        _refused(L, sp(ld=1540, f16=f16), "fused q|k|v")
        _refused(L, sp(NL=256, f16=f16), "512 latents")
        _refused(L, sp(part=d + 8, f16=f16), "16-byte alignment")
        _refused(L, sp(Wo=d + 8, f16=f16), "16-byte alignment")
    _refused(L, L.rald_op_attn_self_proj(d, 1536, d, d, 256, 8, 1, None), "512 latents")

    def xa(hin=d, Wq=d, Kc=d, ldk=1536, sK=64 * 1536, Vt=d, ldvt=64, sVt=1536 * 64, Wo=d, part=d, M=512, NL=512, heads=8, nkeys=64, f16=0):
        return L.rald_op_xattn_q2_proj_slabs(hin, Wq, Kc, ldk, sK, Vt, ldvt, sVt, Wo, part, M, NL, heads, nkeys, 0.18, f16, None)

    for f16 in (0, 1):
        _refused(L, xa(part=None, f16=f16), "bad arguments")
        _refused(L, xa(M=0, NL=32, f16=f16), "bad arguments")
        _refused(L, xa(heads=4, f16=f16), "64 condition tokens")
        _refused(L, xa(nkeys=128, f16=f16), "64 condition tokens")
        _refused(L, xa(M=520, f16=f16), "whole 32-row blocks")
        _refused(L, xa(M=512, NL=48, f16=f16), "whole 32-row blocks")
        _refused(L, xa(M=96, NL=64, f16=f16), "whole 32-row blocks")
        _refused(L, xa(ldk=1540, f16=f16), "16-byte alignment")
        _refused(L, xa(sVt=1536 * 64 + 4, f16=f16), "16-byte alignment")
        _refused(L, xa(Wq=d + 8, f16=f16), "16-byte alignment")
    _refused(L, L.rald_op_reduce_resid_ln_slabs(d, 3, 512 * 512, d, d, d, 512, d, d, 0, 512, 0.0, 1e-5, 1, None), "fp16 slabs come in eights")
    _refused(L, L.rald_op_reduce_resid_ln_slabs(None, 8, 512 * 512, d, d, d, 512, d, d, 0, 512, 0.0, 1e-5, 1, None), "bad arguments")
