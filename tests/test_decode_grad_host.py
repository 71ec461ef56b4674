"""The decoder's field gradient on the CPU: the mathematics behind ae_decode_grad_stream_kernel, the normal of
post.hip's oriented points, the Newton step rule, and the refusals of the new C entries.  No GPU."""
import math

import pytest
import torch

from conftest import rel_l2
from decode_grad_ref import dfeatures, formula_grad, model_grad, newton_replay, normals64, xform64
from test_gpu_ae_decode import SLOT_ONE, SLOT_STD, SLOT_U, _g, _queries, _rotated_basis, _sd, _slot
from test_gpu_train_ops import DUMMY, L_cpu, _refused  # noqa: F401  (L_cpu is a fixture)


def _tables64(sd, d):
    """ae_decode_tables (ae_decode.hip) in float64, nothing rounded: (t2aug [d,64], L [64,64] with L^T L = the Gram matrix of the centred
    point embedding / d, c0)"""
    D = lambda k: sd[k].double()
    Wq, Wkv = D("decoder_cross_attn.fn.to_q.weight"), D("decoder_cross_attn.fn.to_kv.weight")
    Wk, Wv = Wkv[:d], Wkv[d:]
    ng, nb = D("decoder_cross_attn.norm.weight"), D("decoder_cross_attn.norm.bias")
    Wa = torch.cat([D("point_embed.mlp.weight"), D("point_embed.mlp.bias")[:, None]], 1)            # [d,52]
    Wc = Wa - Wa.mean(0, keepdim=True)
    R = torch.linalg.qr(Wc / math.sqrt(d)).R                                                           # [52,52]
    s = 1.4426950408889634 / math.sqrt(d)
    T = s * (Wq * ng[None]) @ Wc                                                                      # [d,52]
    tb = s * (Wq @ nb)
    cols = [_slot(f) for f in range(51)] + [SLOT_ONE]
    t2 = torch.zeros(d, 64, dtype=torch.float64)
    t2[:, cols] = Wk.t() @ T
    t2[:, SLOT_STD] = Wk.t() @ tb
    w_out, b_out = D("to_outputs.weight")[0], D("to_outputs.bias")[0]
    wo, bo = D("decoder_cross_attn.fn.to_out.weight"), D("decoder_cross_attn.fn.to_out.bias")
    t2[:, SLOT_U] = Wv.t() @ (wo.t() @ w_out)
    Lm = torch.zeros(64, 64, dtype=torch.float64)
    Lm[:52, cols] = R
    return t2, Lm, float(bo @ w_out + b_out)


@pytest.mark.parametrize("dim,M", [(256, 64), (512, 128)])
@pytest.mark.parametrize("kind", ["plain", "peaked"])
@pytest.mark.parametrize("basis_kind", ["shipped", "dense"])
def test_formula_gradient_equals_autograd_through_the_model(dim, M, kind, basis_kind):
    """The closed form of DESIGN section 18 in float64 on exact (float64) tables against autograd through the oracle's decoder: logits and
    gradients to 1e-9 relative (rel-L2 over all queries), for the shipped basis and a rotated one, plain and peaked weights."""
    basis = None if basis_kind == "shipped" else _rotated_basis("dense")
    sd = _sd(dim, M, kind, basis)
    t2, Lm, c0 = _tables64(sd, dim)
    B, Q = 3, 200
    x = torch.randn(B, M, dim, generator=_g(dim + M), dtype=torch.float64)
    q = _queries(B, Q, 17)
    case = dict(x=x, gamma=sd["decoder_cross_attn.norm_context.weight"], beta=sd["decoder_cross_attn.norm_context.bias"], t2=t2, L=Lm,
                basis=sd["point_embed.basis"], c0=c0, q=q)
    out, grad, Tg = formula_grad(case)
    ref, gref = model_grad(sd, x, q)
    e0, e1 = rel_l2(out, ref), rel_l2(grad, gref)
    print(f"formula vs autograd {dim}/{M} {kind} {basis_kind}: logits {e0:.3g}, gradient {e1:.3g}; |grad| min {float(gref.norm(dim=-1).min()):.3g} "
          f"median {float(gref.norm(dim=-1).median()):.3g}")
    assert e0 <= 1e-9 and e1 <= 1e-9
    assert bool(torch.isfinite(Tg).all()) and bool((Tg > 0).all())


def test_feature_jacobian_equals_autograd():
    q = _queries(1, 50, 3)[0].double().requires_grad_(True)
    basis = _rotated_basis("dense").double()
    from test_gpu_ae_decode import _features
    Fm = _features(q, basis)
    J = torch.stack([torch.autograd.grad(Fm[:, k].sum(), q, retain_graph=True)[0] for k in range(64)], 1)
    assert float((J - dfeatures(q.detach(), basis)).abs().max()) < 1e-12


RANGES = {"cone": [0.0, -60.0, -90.0, 100.0, 60.0, 90.0], "box": [-40.0, -30.0, -2.0, 60.0, 30.0, 6.0]}


@pytest.mark.parametrize("aniso,iso", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("view_cone", [True, False])
def test_closed_form_normal_equals_autograd_through_the_transform(aniso, iso, view_cone):
    """normals64 (the closed form of post.hip's normal_of) against -J^-T g normalised with J by autograd through xform64, to 1e-9; points at
    r = 0 and el = +-90 degrees (view cone) and a zero gradient give the zero normal."""
    rng = RANGES["cone" if view_cone else "box"]
    g = _g(5)
    p = (torch.rand(300, 3, generator=g, dtype=torch.float64) * 1.9 - 0.95).requires_grad_(True)
    gr = torch.randn(300, 3, generator=g, dtype=torch.float64) * 20
    m = xform64(p, rng, aniso, iso, view_cone)
    J = torch.stack([torch.autograd.grad(m[:, i].sum(), p, retain_graph=True)[0] for i in range(3)], 1)     # [n, i, j] = d m_i / d p_j
    v = torch.linalg.solve(J.transpose(1, 2), gr[:, :, None])[:, :, 0]                                      # J^T v = g
    ref = -v / v.norm(dim=1, keepdim=True)
    got = normals64(p.detach(), gr, rng, aniso, iso, view_cone)
    assert float((got - ref).abs().max()) < 1e-9
    assert float((got.norm(dim=1) - 1).abs().max()) < 1e-12
    # degenerate inputs
    pd = torch.tensor([[-1.0, 0.2, 0.3], [0.5, 0.1, 1.0], [0.5, 0.1, -1.0], [0.3, 0.3, 0.3]], dtype=torch.float64)
    gd = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    nd = normals64(pd, gd, rng, aniso, iso, view_cone)
    assert torch.equal(nd[3], torch.zeros(3, dtype=torch.float64))
    zero = torch.zeros(3, dtype=torch.float64)
    if view_cone:                # the cone's ranges put el = +-90 degrees at p2 = +-1 (either normalisation) and r = 0 at p0 = -1 (anisotropic)
        assert torch.equal(nd[1], zero) and torch.equal(nd[2], zero)
        assert torch.equal(nd[0], zero) if not iso else abs(float(nd[0].norm()) - 1) < 1e-12
    else:
        assert float((nd[:3].norm(dim=1) - 1).abs().max()) < 1e-12


def test_normals_point_from_occupied_to_empty():
    """a logit that falls along +x of the metric box: the normal is +x"""
    n = normals64(torch.zeros(1, 3), torch.tensor([[-3.0, 0.0, 0.0]]), RANGES["box"], True, False, False)
    assert torch.equal(n, torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64))


def test_newton_step_rule():
    """newton_replay: the free step lands on the linearised zero, a long step is cut to max_step, |g|^2 <= 1e-20 and non-finite inputs leave
    the point alone, and the result stays in the box"""
    q = torch.tensor([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.99, -0.99, 0.0], [0.1, 0.2, 0.3]], dtype=torch.float64)
    logit = torch.tensor([0.5, 5.0, 1.0, 1.0, -3.0, float("nan")], dtype=torch.float64)
    g = torch.tensor([[10.0, 0.0, 0.0], [10.0, 0.0, 0.0], [1e-11, 0.0, 0.0], [float("nan"), 1.0, 0.0], [10.0, -10.0, 0.0], [1.0, 0.0, 0.0]],
                     dtype=torch.float64)
    qn, cut = newton_replay(q, logit, g, 0.05)
    assert torch.allclose(qn[0], torch.tensor([0.05, 0.2, 0.3], dtype=torch.float64), atol=1e-15) and not bool(cut[0])
    assert torch.allclose(qn[1], torch.tensor([0.05, 0.2, 0.3], dtype=torch.float64), atol=1e-15) and bool(cut[1])
    assert torch.equal(qn[2], q[2]) and torch.equal(qn[3], q[3]) and torch.equal(qn[5], q[5])
    assert torch.equal(qn[4], torch.tensor([1.0, -1.0, 0.0], dtype=torch.float64)) and bool(cut[4])
    assert float((qn - q).norm(dim=1).max()) <= 0.05 * (1 + 1e-12)


def test_gradient_entries_refuse_bad_arguments(L_cpu):
    """every check of rald_op_ae_decode_grad and rald_post_oriented_points[_ragged] comes before the first HIP call and names the constraint"""
    L, d = L_cpu, DUMMY
    call = lambda B=2, Q=10, M=128, dim=256, x=d, q=d, out=d, grad=d, proj=None, step=0.05, scratch=d, nbytes=1 << 40: \
        L.rald_op_ae_decode_grad(x, d, d, d, d, d, 0.0, q, None, out, grad, proj, step, B, Q, M, dim, scratch, nbytes, None)
    for M in (0, 48, 544, 1024):
        _refused(L, call(M=M), "num_latents", "[32,512]")
    _refused(L, call(dim=384), "dim", "256 or 512")
    _refused(L, call(Q=0), "n_queries")
    _refused(L, call(B=0), "batch")
    _refused(L, call(B=65536), "batch", "65535")
    for kw in (dict(x=None), dict(q=None), dict(out=None), dict(grad=None), dict(scratch=None)):
        _refused(L, call(**kw), "null pointer")
    for step in (0.0, -0.1, float("nan"), float("inf")):
        _refused(L, call(proj=d, step=step), "max_step", "finite and > 0")
    _refused(L, call(nbytes=L.rald_op_ae_decode_scratch_bytes(2, 128) - 1), "scratch too small")
    _refused(L, call(scratch=d + 4), "16-byte aligned")
    _refused(L, L.rald_ae_decode_queries_grad(None, d, d, 1, 10, d, d, None, 0.05, None), "null handle")
    _refused(L, L.rald_ae_decode_queries_grad_ragged(None, d, d, d, 1, 10, d, d, None, 0.05, None), "null handle")
    import ctypes as C
    rng = (C.c_double * 6)(-1, -1, -1, 1, 1, 1)
    for kw in ((None, d, d, d), (d, None, d, d), (d, d, None, d), (d, d, d, None)):
        _refused(L, L.rald_post_oriented_points(kw[0], kw[1], 5, rng, 1, 0, 0, kw[2], kw[3], None), "post_oriented_points", "null pointer")
    _refused(L, L.rald_post_oriented_points(d, d, 0, rng, 1, 0, 0, d, d, None), "post_oriented_points", "bad argument")
    _refused(L, L.rald_post_oriented_points(d, d, 5, None, 1, 0, 0, d, d, None), "post_oriented_points", "bad argument")
    _refused(L, L.rald_post_oriented_points_ragged(d, d, None, 2, 5, rng, 1, 0, 0, d, d, None), "null offsets")
    _refused(L, L.rald_post_oriented_points_ragged(d, d, d, 0, 5, rng, 1, 0, 0, d, d, None), "post_oriented_points", "bad argument")
