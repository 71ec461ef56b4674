"""The gradient decoder (ae_decode_grad_stream_kernel, rald_amd/csrc/ae_decode.hip) through its op entry
rald_op_ae_decode_grad: per query, every element of every output.

References (tests/decode_grad_ref.py, float64, from the fp32 values handed to the entry): autograd through the oracle's decoder on the
real tables ("model") and the closed form on arbitrary tables ("formula").  The logit must equal rald_op_ae_decode's bit for bit.
The gradient's error is counted in the per-component unit Tg derived in decode_grad_ref.py's docstring: 2^-11 times the sum of the
absolute values of the products that make up the component (a_l taken as its two terms p_l u_l and p_l ubar), so it is absolute and
covers the peaked fixtures, where |grad| falls to 1e-14, without leaving a query out.  k = worst |got - ref| / Tg is measured on an
MI355X and every bound is at most 2.5 times the worst k measured (docstrings).  The unit does not charge the movement of the softmax
weights under the scores' own rounding, so k grows with the size of the scores; see decode_grad_ref.py.

Conventions of test_gpu_ae_decode.py: outputs start as NaN and are followed by 64 sentinels that must survive; the queries sit before a
NaN tail; B = 3 distinct samples.  GRAD_NW is the kernel's waves per workgroup (8): 64 * GRAD_NW + 1 queries need a second workgroup."""
import pytest
import torch

from rald_amd import weights
from decode_grad_ref import formula_grad, k_grad, model_grad, newton_replay
from test_gpu_ae_decode import (CRAFTED, SLOT_STD, SLOT_U, _exact_rows, _g, _guard_ok, _guarded, _le, _limg_of, _L_of, _queries, _real_case,
                                _rotated_basis, _run, _sd, _tables)

gpu = pytest.mark.gpu
GRAD_NW = 8
SPECIAL = torch.tensor([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)] + [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])


def _with_special(case):
    """the eight corners, the origin and a face centre in front of every sample's queries"""
    q = case["q"].clone()
    q[:, :SPECIAL.shape[0]] = SPECIAL
    return dict(case, q=q)


def _run_grad(case, Q=None, rows=None, project=False, max_step=0.05, segments=None):
    """the entry on the first Q queries (of the samples `rows`) -> (logits [B,Q], grad [B,Q,3], projected or None) on the CPU.  With
    `segments` (one length per sample) the ragged form: sample b's first segments[b] queries, concatenated -> [T], [T,3]."""
    from rald_amd import _handles as Hd
    sel = slice(None) if rows is None else rows
    x, q = case["x"][sel], case["q"][sel]
    q = q if Q is None else q[:, :Q]
    B = q.shape[0]
    offsets = None
    if segments is None:
        n = B * q.shape[1]
        flat = q.reshape(-1)
    else:
        assert len(segments) == B
        flat = torch.cat([q[b, :segments[b]].reshape(-1) for b in range(B)])
        n = sum(segments)
        offsets = torch.tensor([0] + list(torch.tensor(segments).cumsum(0)), dtype=torch.int64).cuda()
    qbuf = torch.full((n * 3 + 192,), float("nan"), device="cuda")
    qbuf[:n * 3] = flat.cuda()
    out, grad = _guarded(n, 64), _guarded(n * 3, 64)
    proj = _guarded(n * 3, 64) if project else None
    dev = lambda t: t.contiguous().cuda()
    qv = qbuf[:n * 3].view(B, -1, 3) if segments is None else qbuf[:n * 3].view(n, 3)
    Hd.op_ae_decode_grad(dev(x), dev(case["gamma"]), dev(case["beta"]), dev(case["t2"]), dev(case["limg"]), dev(case["basis"]), case["c0"],
                         qv, out[:n], grad[:n * 3], None if proj is None else proj[:n * 3], max_step, offsets,
                         None if segments is None else max(segments))
    torch.cuda.synchronize()
    assert _guard_ok(out, n) and _guard_ok(grad, n * 3) and (proj is None or _guard_ok(proj, n * 3)), "the decoder wrote past an output"
    shape = (B, -1) if segments is None else (n,)
    return out[:n].view(*shape).cpu(), grad[:n * 3].view(*shape, 3).cpu(), None if proj is None else proj[:n * 3].view(*shape, 3).cpu()


def _rel_l2(a, b):
    return float((a.double() - b).norm() / b.norm())


# ---- 1. the logit is the plain kernel's ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("basis_kind", ["shipped", "dense"])
def test_logits_equal_the_plain_decoder_bit_for_bit(basis_kind):
    """B = 3, 256/128, Q = 1, 63, 64, 65 and 64 * GRAD_NW + 1 (a second workgroup), with and without the projected output: torch.equal with
    rald_op_ae_decode on the same inputs.  Both kernel forms (block-diagonal and general basis)."""
    basis = None if basis_kind == "shipped" else _rotated_basis("dense")
    sd, case = _real_case(256, 128, 3, 64 * GRAD_NW + 1, basis=basis, seed=21)
    for Q in (1, 63, 64, 65, 64 * GRAD_NW + 1):
        plain = _run(case, Q)
        for project in (False, True):
            out, grad, proj = _run_grad(case, Q, project=project)
            assert torch.equal(out, plain), (Q, project)
            assert bool(torch.isfinite(grad).all()) and (proj is None or bool(torch.isfinite(proj).all()))


@gpu
def test_grid_stride_second_pass_is_the_first_pass_elsewhere():
    """B = 3: 256 / 3 = 85 workgroups of GRAD_NW waves per sample take 680 chunks in one pass; Q = 680 * 64 + 65 gives two waves a second
    chunk, one of them a single query.  Logits equal the plain kernel's; and since a chunk's outputs do not depend on where in the grid it
    runs, all three outputs of the queries from row 680 * 64 on equal the launch of those queries alone, bit for bit."""
    first = 85 * GRAD_NW * 64
    sd, case = _real_case(256, 128, 3, first + 65, seed=27)
    out, grad, proj = _run_grad(case, project=True)
    assert torch.equal(out, _run(case))
    o2, g2, p2 = _run_grad(dict(case, q=case["q"][:, first:].contiguous()), project=True)
    assert torch.equal(out[:, first:], o2) and torch.equal(grad[:, first:], g2) and torch.equal(proj[:, first:], p2)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(proj).all())


SEGMENTS = (0, 1, 64, 65, 700)


@gpu
def test_ragged_equals_dense_on_the_segment_alone():
    """Five samples with segments of 0, 1, 64, 65 and 700 queries (an empty one; the segments start at rows 0, 0, 1, 65 and 130: unaligned):
    every segment's logits equal rald_op_ae_decode on that sample alone and all three outputs equal the dense gradient call on that
    sample alone, bit for bit.  Peaked weights, 512/96 (an odd number of tiles)."""
    sd, case = _real_case(512, 96, 5, 700, "peaked", seed=22)
    out, grad, proj = _run_grad(case, segments=list(SEGMENTS), project=True, max_step=0.05)
    assert out.shape == (sum(SEGMENTS),)
    at = 0
    for b, n in enumerate(SEGMENTS):
        if n:
            o1, g1, p1 = _run_grad(case, n, rows=slice(b, b + 1), project=True, max_step=0.05)
            assert torch.equal(out[at:at + n], _run(case, n, rows=slice(b, b + 1))[0]), b
            assert torch.equal(out[at:at + n], o1[0]) and torch.equal(grad[at:at + n], g1[0]) and torch.equal(proj[at:at + n], p1[0]), b
        at += n


# ---- 2. the gradient against float64 ------------------------------------------------------------------------------------------------------
# (dim, M, kind, basis): bound; measured k in the docstring below, in this order
REAL = [
    ((256, 32, "plain", "shipped"), 0.78), ((256, 32, "plain", "dense"), 0.51), ((256, 96, "plain", "shipped"), 0.48),
    ((256, 96, "plain", "dense"), 0.24), ((256, 512, "plain", "shipped"), 0.18), ((256, 512, "plain", "dense"), 0.12),
    ((512, 32, "plain", "shipped"), 0.9), ((512, 32, "plain", "dense"), 0.83), ((512, 96, "plain", "shipped"), 0.39),
    ((512, 96, "plain", "dense"), 0.32), ((512, 512, "plain", "shipped"), 0.17), ((512, 512, "plain", "dense"), 0.14),
    ((256, 96, "peaked", "shipped"), 23), ((256, 512, "peaked", "dense"), 5.8), ((512, 32, "peaked", "dense"), 8.4),
    ((512, 512, "peaked", "shipped"), 7.6),
]


@gpu
@pytest.mark.parametrize("cfg,bound", REAL, ids=["-".join(map(str, c)) for c, _ in REAL])
def test_gradient_on_real_tables_against_the_model_and_the_formula(cfg, bound):
    """B = 3, Q = 330 (two workgroups' worth of chunks is covered by the identity tests; here 5 chunks + a tail of 10), the first ten
    queries of every sample the eight corners, the origin and a face centre.  M = 32 is one score tile, 96 an odd number of tiles, 512
    the largest the entry takes; both kernel forms; plain and peaked weights.  k against the model (autograd through the float64
    oracle) and against the formula, the larger one bounded; the gradient's rel-L2 over all queries is printed for the plain weights.
    Measured k (the larger of the two), in the order of REAL: 0.315, 0.207, 0.195, 0.0979, 0.074, 0.0518, 0.363, 0.332, 0.157, 0.128, 0.0689, 0.0581, 9.52, 2.33, 3.39, 3.04;
    bounds 0.78, 0.51, 0.48, 0.24, 0.18, 0.12, 0.9, 0.83, 0.39, 0.32, 0.17, 0.14, 23, 5.8, 8.4, 7.6.  Measured rel-L2 against the model: 3.1e-4 .. 4.7e-4 on the plain weights (one fp16 rounding), 2.7e-3 .. 3.2e-3 on the
    peaked ones; smallest / median |grad| there: 0.27 .. 4.5 / 9.5 .. 36 (plain), down to 1e-13 / 60 .. 260 (peaked)."""
    dim, M, kind, basis_kind = cfg
    basis = None if basis_kind == "shipped" else _rotated_basis("dense")
    sd, case = _real_case(dim, M, 3, 330, kind, basis=basis, seed=23)
    case = _with_special(case)
    _, gref, Tg = formula_grad(case)
    _, gmod = model_grad(sd, case["x"], case["q"])
    out, grad, _ = _run_grad(case)
    assert torch.equal(out, _run(case))
    kf, km = k_grad(grad, gref, Tg), k_grad(grad, gmod, Tg)
    print(f"gradient {cfg}: k formula {kf:.3g}, k model {km:.3g}, rel-L2 vs model {_rel_l2(grad, gmod):.3g}, |grad| min "
          f"{float(gmod.norm(dim=-1).min()):.3g} median {float(gmod.norm(dim=-1).median()):.3g}")
    _le(f"decode grad {cfg}", max(kf, km), bound)


# ---- 3. crafted edges, formula reference ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,bound", [("rise", 0.8), ("fall", 0.92), ("half1", 5.7e-11)])
def test_gradient_when_the_maximum_moves_between_tiles(kind, bound):
    """_ramp_case of test_gpu_ae_decode.py (hb steps of up to 300 log2 units from tile to tile, rising to the last tile or falling from the
    first; one latent of an h = 1 row 60 above the rest): pass 2 must form a_l from the FINAL maximum and denominator.  Finite, logits
    identical to the plain kernel's.  Measured k: 0.322, 0.371, 2.29e-11 (half1: the one latent 60 above the rest takes the whole softmax, a_l
    underflows and the unit keeps the size of the cancelling terms); bounds 0.8, 0.92, 5.7e-11."""
    case = CRAFTED["ramp_" + kind]()
    _, gref, Tg = formula_grad(case)
    out, grad, _ = _run_grad(case)
    assert torch.equal(out, _run(case)) and bool(torch.isfinite(grad).all())
    _le(f"decode grad ramp {kind}", k_grad(grad, gref, Tg), bound)


def _const_u_case(M=64, Q=300, seed=31):
    """u_l = 2 for every latent, exactly (LN(x) = x bit for bit by _exact_rows, channel 0 holds 1.0 and is the only one that feeds the u
    column), under scores that differ from latent to latent: every p_l u_l is an exact doubling, so num = 2 den and ubar = u bit for bit:
    a_l = 0, the gradient is exactly zero, the logit exactly 2 + c0."""
    g = _g(seed)
    B = 3
    design = torch.zeros(B, M, 256, dtype=torch.float64)
    design[:, :, 0] = 1.0
    design[:, :, 1:60] = torch.randint(-64, 65, (B, M, 59), generator=g).double() / 128
    x = torch.stack([_exact_rows(design[b]) for b in range(B)])
    t2 = torch.zeros(256, 64)
    t2[1:60, :52] = torch.randn(59, 52, generator=g) * 0.5
    t2[1:60, SLOT_STD] = torch.randn(59, generator=g)
    t2[0, SLOT_U] = 2.0
    _, limg, _ = _tables(_sd(256, 128), 256)
    return dict(x=x, gamma=torch.full((256,), 2.0), beta=torch.zeros(256), t2=t2, limg=limg, basis=weights.point_embed_basis(), c0=0.375,
                q=_queries(B, Q, seed + 1))


@gpu
def test_constant_u_and_equal_scores_give_exactly_zero():
    """(a) u constant (+ c0) under varying scores (_const_u_case): logit == 2.375, gradient == 0 and projected == q, all exactly.
    (b) all coefficient columns zero (CRAFTED scale_zero: all scores equal, G = sum_l a_l 0): gradient == 0 exactly, projected == q."""
    case = _const_u_case()
    Y = (case["x"].double() @ case["t2"].double())
    assert torch.equal(Y[:, :, SLOT_U], torch.full_like(Y[:, :, SLOT_U], 2.0))
    ref, gref, _ = formula_grad(case)
    assert float(gref.abs().max()) < 1e-9 and float((ref - 2.375).abs().max()) < 1e-7       # float64 sees LayerNorm's eps: LN(x) = x (1 + 1e-9)
    out, grad, proj = _run_grad(case, project=True)
    assert torch.equal(out, torch.full_like(out, 2.375)) and torch.equal(out, _run(case))
    assert torch.equal(grad, torch.zeros_like(grad)) and torch.equal(proj, case["q"])
    case = CRAFTED["scale_zero"]()
    out, grad, proj = _run_grad(case, project=True)
    assert torch.equal(out, _run(case))
    assert torch.equal(grad, torch.zeros_like(grad)) and torch.equal(proj, case["q"])


def _tiny_variance_case():
    """the real variance factor times 2^-9 (var = 2^-18 of the real one, below eps = 1e-5 for every query: rstd ~ 300 is set by eps) with
    the coefficient columns scaled down by 2^-7 to keep the scores at their usual size.  var is still a tenth of eps or more for the
    median query, so the rstd^3 term (3e7 times d var / d q) is a material part of the gradient"""
    sd, case = _real_case(256, 128, 3, 300, seed=24)
    Lm = _L_of(case["limg"]).numpy() * 2.0 ** -9
    t2 = case["t2"].clone()
    t2[:, :52] *= 2.0 ** -7
    return dict(case, limg=_limg_of(Lm), t2=t2)


@gpu
def test_tiny_variance_row_where_eps_dominates():
    """_tiny_variance_case: var < eps / 2 for every query and > eps / 10 for the median one (asserted on the reference).
    Measured k: 0.378; bound 0.94."""
    case = _tiny_variance_case()
    from test_gpu_ae_decode import _context, _scores
    rstd = _scores(case, _context(case)[0], case["q"][0])[1]
    var = rstd ** -2 - 1e-5
    assert float(var.max()) < 0.5e-5 and float(var.median()) > 1e-6
    _, gref, Tg = formula_grad(case)
    out, grad, _ = _run_grad(case)
    assert torch.equal(out, _run(case))
    _le("decode grad tiny variance", k_grad(grad, gref, Tg), 0.94)


@gpu
def test_scores_near_the_domain_limit_stay_finite():
    """CRAFTED scale_mixed: four samples whose coefficients are 2^-30, 1, 2^12 and 2^30 times a common table (the last one's scores reach
    2^26 .. 2^28, next to the documented 2^29): every output finite, logits the plain kernel's.  Measured k: 13.8 (scores of 2^28 move the softmax
    weights by far more than the unit charges); bound 34."""
    case = CRAFTED["scale_mixed"]()
    _, gref, Tg = formula_grad(case)
    out, grad, proj = _run_grad(case, project=True)
    assert torch.equal(out, _run(case))
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(proj).all())
    _le("decode grad scale mixed", k_grad(grad, gref, Tg), 34)


# ---- 4. the projected output ------------------------------------------------------------------------------------------------------------------
PROJ_BOUND = {0.05: 8.5e-8, 0.125: 1.0e-7}


@gpu
@pytest.mark.parametrize("max_step", [0.05, 0.125])
def test_projected_point_against_the_float64_replay(max_step):
    """512/128 plain, B = 3, Q = 2000 with the special points: q' against newton_replay (float64) of the kernel's OWN logit and gradient (so
    the comparison isolates the step rule: fp32 products, one division, one square root, the scale and the clamp, about ten roundings of
    numbers below max_step plus the rounding of q + s, 2^-25 for |q'| < 1).  Per axis |q' - q'_ref| <= PROJ_BOUND (measured: 3.43e-8 at max_step 0.05, 4.13e-8 at 0.125; bounds 8.5e-8, 1.0e-7);
    every q' in [-1,1]; a step that was cut has |q' - q| <= max_step (1 + 2^-20), asserted for max_step = 0.125, where 2^-20 max_step =
    1.2e-7 is above the 5.2e-8 that rounding q + s to fp32 coordinates of size up to 1 can add to the length (3^0.5 2^-25); at 0.05 the
    allowance would be 4.8e-8, below it.  Both clamped and free steps occur (asserted)."""
    sd, case = _real_case(512, 128, 3, 2000, seed=25)
    case = _with_special(case)
    out, grad, proj = _run_grad(case, project=True, max_step=max_step)
    ref, cut = newton_replay(case["q"], out, grad, max_step)
    assert bool(cut.any()) and bool((~cut).any())
    assert float(proj.abs().max()) <= 1.0
    err = float((proj.double() - ref).abs().max())
    if max_step == 0.125:
        moved = (proj.double() - case["q"].double()).norm(dim=-1)
        assert float(moved[cut].max()) <= max_step * (1 + 2.0 ** -20), float(moved[cut].max())
    _le(f"projected max_step {max_step}: per-axis error", err, PROJ_BOUND[max_step])


# ---- 5. refusals leave the outputs alone ---------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_the_outputs_untouched():
    """num_latents above 512 (the transposed image would not fit in LDS) and a misaligned scratch raise and write nothing: the outputs keep
    their NaN prefill and their sentinels."""
    from rald_amd import _handles as Hd
    from rald_amd._lib import lib
    sd, case = _real_case(256, 128, 1, 10, seed=26)
    dev = lambda t: t.contiguous().cuda()
    out, grad, proj = _guarded(10, 64), _guarded(30, 64), _guarded(30, 64)
    untouched = lambda: (bool(torch.isnan(out[:10]).all()) and bool(torch.isnan(grad[:30]).all()) and bool(torch.isnan(proj[:30]).all())
                         and _guard_ok(out, 10) and _guard_ok(grad, 30) and _guard_ok(proj, 30))
    for M in (544, 1024):
        x = torch.randn(1, M, 256, generator=_g(M))
        with pytest.raises(RuntimeError, match="num_latents"):
            Hd.op_ae_decode_grad(dev(x), dev(case["gamma"]), dev(case["beta"]), dev(case["t2"]), dev(case["limg"]), dev(case["basis"]),
                                 case["c0"], dev(case["q"]), out[:10], grad[:30], proj[:30], 0.05)
        torch.cuda.synchronize()
        assert untouched()
    L = lib()
    nbytes = L.rald_op_ae_decode_scratch_bytes(1, 128)
    scratch = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
    args = [dev(case[k]) for k in ("x", "gamma", "beta", "t2", "limg", "basis")]
    q = dev(case["q"])
    rc = L.rald_op_ae_decode_grad(*[t.data_ptr() for t in args], case["c0"], q.data_ptr(), None, out.data_ptr(), grad.data_ptr(),
                                  proj.data_ptr(), 0.05, 1, 10, 128, 256, scratch.data_ptr() + 4, nbytes, None)
    assert rc != 0 and "16-byte aligned" in L.rald_last_error().decode()
    rc = L.rald_op_ae_decode_grad(*[t.data_ptr() for t in args], case["c0"], q.data_ptr(), None, out.data_ptr(), grad.data_ptr(),
                                  proj.data_ptr(), float("nan"), 1, 10, 128, 256, scratch.data_ptr(), nbytes, None)
    assert rc != 0 and "max_step" in L.rald_last_error().decode()
    torch.cuda.synchronize()
    assert untouched()
