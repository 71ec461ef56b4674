"""Float64 references of the decoder's field gradient (rald_amd/csrc/ae_decode.hip), shared by
test_decode_grad_host.py, test_gpu_ae_decode_grad.py and test_gpu_oriented_points.py.  Nothing here rounds to fp16 or imitates the
kernel's order of operations; the inputs are the fp32 values handed to the entry, widened exactly.

  formula_grad    the closed form on ARBITRARY tables (the `case` dicts of test_gpu_ae_decode.py), and its error unit
  model_grad      autograd through oracle.rald_oracle.ae_decode_queries on a float64 state dict
  newton_replay   the projected output's step rule from a logit and a gradient
  xform64 / normals64   xform_point restated in float64 (differentiable) and the closed-form normal of post.hip

Error unit of the gradient.  With p = softmax2(S), ubar = p.u, the gradient's component x is

    ln2 [ rstd sum_k D_kx sum_l p_l (u_l - ubar) H_lk  -  rstd^3 (sum_l p_l (u_l - ubar) A_l) sum_i (L f~)_i sum_k L_ik D~_kx ]

a sum of products whose factors the kernel holds in fp16 (H, f~, L, D~, and a_l = p_l (u_l - ubar) itself) or computes from fp16
products (A_l, L f~).  Rounding one factor of a product to 11 bits moves it by 2^-11 of its size, so the unit charges every product
once at that rate, with a_l written as its two terms p_l u_l and p_l ubar and A_l as its own (sum_k |f_k| |H_lk| + |h0_l|):

    W_l  = p_l (|u_l| + |ubar|)
    Tg_x = 2^-11 ln2 [ rstd sum_k |D_kx| sum_l W_l |H_lk|  +  rstd^3 (sum_l W_l Aabs_l) sum_i |(L f~)_i| sum_k |L_ik| |D~_kx| ]

It is absolute: where the softmax saturates (a_l ~ 1e-14) the unit stays at the size of the terms that cancel, which is what fp32's
ubar and fp16's a_l can resolve.  Not charged: the movement of p itself under the scores' rounding (2 ln2 times the score error in
log2 units, the T_q of test_gpu_ae_decode.py), which multiplies every term alike - so the measured k grows with the size of the
scores (measured on an MI355X: 0.05 .. 0.4 on the plain fixtures, 2 .. 10 on the peaked ones, 14 with scores of 2^28); the bounds, not
the unit, are what is tight."""
import math

import torch

from oracle import rald_oracle as O
from test_gpu_ae_decode import SLOT_ONE, SLOT_STD, SLOT_U, U16, _context, _features, _L_of, _slot

LN2 = math.log(2.0)


def dfeatures(q, basis):
    """d features / d q in slot order: [Q,64,3] float64 (rows 51.. are zero: the constant and the std slots)"""
    proj = q @ basis                                               # [Q,24]
    bt = basis.t()[None]                                           # [1,24,3]
    D = torch.zeros(q.shape[0], 64, 3, dtype=torch.float64)
    D[:, [_slot(f) for f in range(24)]] = proj.cos()[:, :, None] * bt
    D[:, [_slot(f) for f in range(24, 48)]] = -proj.sin()[:, :, None] * bt
    for a in range(3):
        D[:, _slot(48 + a), a] = 1.0
    return D


def formula_grad(case, block=4096):
    """(logit [B,Q], grad [B,Q,3], Tg [B,Q,3]) in float64 from a case dict (x, gamma, beta, t2, limg, basis, c0, q)"""
    Y, q, c0 = (case["Y"] if "Y" in case else _context(case)), case["q"].double(), case["c0"]                # "Y": a context given directly
    basis, Lm = case["basis"].double(), (case["L"] if "L" in case else _L_of(case["limg"]))       # "L": a float64 factor instead of the image
    B, Q = q.shape[:2]
    out = torch.zeros(B, Q, dtype=torch.float64)
    grad, Tg = torch.zeros(B, Q, 3, dtype=torch.float64), torch.zeros(B, Q, 3, dtype=torch.float64)
    for b in range(B):
        H, h0, hb, u = Y[b][:, :51], Y[b][:, SLOT_ONE], Y[b][:, SLOT_STD], Y[b][:, SLOT_U]
        for s in range(0, Q, block):
            qq = q[b, s:s + block]
            Fm, D = _features(qq, basis), dfeatures(qq, basis)
            Lf = Fm @ Lm.t()                                       # [n,64]
            rstd = (Lf ** 2).sum(1).add(1e-5).rsqrt()
            A = Fm[:, :51] @ H.t() + h0                            # [n,M]
            S = rstd[:, None] * A + hb
            P = torch.exp2(S - S.max(1, keepdim=True).values)
            P = P / P.sum(1, keepdim=True)
            ubar = (P * u).sum(1)
            a = P * (u[None] - ubar[:, None])
            G = a @ H                                              # [n,51]
            LD = torch.einsum("ik,nkx->nix", Lm, D)                # L . D~   [n,64,3]
            dvar = torch.einsum("ni,nix->nx", Lf, LD)              # half of d var / d q
            sA = (a * A).sum(1)
            t1 = rstd[:, None] * torch.einsum("nk,nkx->nx", G, D[:, :51])
            t2 = (rstd ** 3 * sA)[:, None] * dvar
            out[b, s:s + block] = ubar + c0
            grad[b, s:s + block] = LN2 * (t1 - t2)
            W = P * (u.abs()[None] + ubar.abs()[:, None])
            Aabs = Fm[:, :51].abs() @ H.abs().t() + h0.abs()
            u1 = rstd[:, None] * torch.einsum("nk,nkx->nx", W @ H.abs(), D[:, :51].abs())
            LDa = torch.einsum("ik,nkx->nix", Lm.abs(), D.abs())
            u2 = (rstd ** 3 * (W * Aabs).sum(1))[:, None] * torch.einsum("ni,nix->nx", Lf.abs(), LDa)
            Tg[b, s:s + block] = U16 * LN2 * (u1 + u2)
    return out, grad, Tg


def context_of_blob(ctx, B, M):
    """Y [B,M,64] float64 (the columns formula_grad reads) of a decoder context as AeHandle.decode_latents writes it: a 64-byte header,
    then per sample the fp16 image [M][64] (128-byte rows, 16-byte chunks XOR-swizzled by the row; h0 in slots 51 + 52, hb in 53 (= 54)
    + 55, all times the sample's power-of-two scale), u [M] fp32 and 1 / scale: exactly the numbers the kernels read"""
    import numpy as np
    raw = ctx.detach().cpu().numpy()[64:]
    stride = M * 128 + M * 4 + 16
    assert raw.size == B * stride
    idx = np.array([[row * 64 + ((((k >> 3) ^ (row & 7)) << 3) + (k & 7)) for k in range(64)] for row in range(M)])
    Y = torch.zeros(B, M, 64, dtype=torch.float64)
    for b in range(B):
        blob = raw[b * stride:(b + 1) * stride]
        img = torch.from_numpy(blob[:M * 128].view(np.float16)[idx].astype(np.float64))
        tail = blob[M * 128:].view(np.float32)
        inv = float(tail[M])
        Y[b, :, :51] = img[:, :51] * inv
        Y[b, :, SLOT_ONE] = (img[:, 51] + img[:, 52]) * inv
        Y[b, :, SLOT_STD] = (img[:, 53] + img[:, 55]) * inv
        Y[b, :, SLOT_U] = torch.from_numpy(tail[:M].astype(np.float64))
    return Y


def model_grad(sd, x, q, block=2048):
    """(logits [B,Q], d logit / d q [B,Q,3]) by autograd through the float64 oracle (each logit depends on its own query only)"""
    sd64 = {k: v.double() for k, v in sd.items()}
    x = x.double()
    outs, grads = [], []
    for s in range(0, q.shape[1], block):
        qq = q[:, s:s + block].double().clone().requires_grad_(True)
        o = O.ae_decode_queries(sd64, x, qq).squeeze(-1)
        (g,) = torch.autograd.grad(o.sum(), qq)
        outs.append(o.detach())
        grads.append(g)
    return torch.cat(outs, 1), torch.cat(grads, 1)


def k_grad(got, ref, Tg):
    """worst |got - ref| / Tg over every component of every query; NaN counts as infinite"""
    r = (got.detach().cpu().double() - ref).abs() / Tg
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


def newton_replay(q, logit, g, max_step):
    """The projected output's rule in float64: s = -logit g / |g|^2, scaled by min(1, max_step / |s|), s = 0 when |g|^2 is not > 1e-20
    or the step is not finite; q' = clamp(q + s, -1, 1).  Returns (q', clamped [..] bool: the steps that were scaled)."""
    q, logit, g = q.double(), logit.double(), g.double()
    g2 = (g * g).sum(-1, keepdim=True)
    ok = g2 > 1e-20
    s = -logit[..., None] / torch.where(ok, g2, torch.ones_like(g2)) * g
    n = (s * s).sum(-1, keepdim=True).sqrt()
    scaled = n > max_step
    s = torch.where(scaled, s * (max_step / torch.where(scaled, n, torch.ones_like(n))), s)
    fin = torch.isfinite(s).all(-1, keepdim=True) & ok
    s = torch.where(fin, s, torch.zeros_like(s))
    return (q + s).clamp(-1.0, 1.0), (scaled & fin).squeeze(-1)


# ---- post.hip: the transform and the normal ------------------------------------------------------------------------------------------------
D2R = 0.017453292519943295


def _scales(pc_range, aniso, iso):
    r = [float(v) for v in pc_range]
    off = torch.tensor([(r[3] + r[0]) / 2, (r[4] + r[1]) / 2, (r[5] + r[2]) / 2], dtype=torch.float64)
    sc = torch.tensor([(r[3] - r[0]) / 2, (r[4] - r[1]) / 2, (r[5] - r[2]) / 2], dtype=torch.float64)
    if iso:
        sc = torch.full((3,), float(sc.max()), dtype=torch.float64)
    elif not aniso:
        sc = torch.zeros(3, dtype=torch.float64)
        off = torch.zeros(3, dtype=torch.float64)
    return sc, off


def xform64(p, pc_range, aniso, iso, view_cone):
    """xform_point (post.hip) in float64, differentiable: inverse_norm_points (isotropic wins when both are set) + polar2cartesian"""
    sc, off = _scales(pc_range, aniso, iso)
    m = p * sc + off
    if view_cone:
        r, az, el = m[..., 0], -(m[..., 1] * D2R), m[..., 2] * D2R
        m = torch.stack([r * el.cos() * az.cos(), r * el.cos() * az.sin(), r * el.sin()], -1)
    return m


def normals64(p, g, pc_range, aniso, iso, view_cone):
    """the closed form of post.hip's normal_of in float64: -J^-T g normalised; zero where r = 0, |cos el| < 2^-20, the length is zero or
    anything is not finite"""
    p, g = p.double(), g.double()
    sc, off = _scales(pc_range, aniso, iso)
    m = p * sc + off
    n = g / sc
    bad = torch.zeros(p.shape[:-1], dtype=torch.bool)
    if view_cone:
        r, az, el = m[..., 0], -(m[..., 1] * D2R), m[..., 2] * D2R
        ce, se, ca, sa = el.cos(), el.sin(), az.cos(), az.sin()
        a, b, c = n[..., 0], n[..., 1] / (-D2R * r * ce), n[..., 2] / (D2R * r)
        n = torch.stack([a * ce * ca - b * sa - c * se * ca, a * ce * sa + b * ca - c * se * sa, a * se + c * ce], -1)
        bad = (r == 0) | (ce.abs() < 2.0 ** -20)
    ln = (n * n).sum(-1).sqrt()
    bad = bad | ~(ln > 0) | ~torch.isfinite(ln)
    out = -n / torch.where(bad, torch.ones_like(ln), ln)[..., None]
    return torch.where(bad[..., None], torch.zeros_like(out), out)
