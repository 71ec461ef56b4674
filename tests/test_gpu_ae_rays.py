"""First-return beam casting (ae_decode_rays_kernel, rald_amd/csrc/ae_rays.hip) through its op entry
rald_op_ae_cast_rays.

Yardstick: a host replay of the rule - march t_k = k / S, first logit > 0, bisection between that sample and the one before - that
obtains every logit from the EXISTING dense decode entry (rald_op_ae_decode), one call on the [B,R,3] sample points per march step and
per bisection step, so the 64-point chunks are the kernel's 64-ray chunks and every comparison is torch.equal.  The sample points are
computed on the CPU in fp32, one rounding per operation (a division for t_k, a product and a sum per coordinate), which is the kernel's
stated order.  The geometry test at the end does not replay the decoder: it compares with an analytic crossing.

Conventions of test_gpu_ae_decode.py: outputs start as sentinels and are followed by 64 more that must survive; B = 3 distinct samples
wherever B is not the subject."""
import math

import pytest
import torch

from test_gpu_ae_decode import SLOT_U, _g, _guard_ok, _guarded, _onehot_case, _real_case, _rotated_basis

gpu = pytest.mark.gpu
NAN = float("nan")


# ---- the entry and its replay -------------------------------------------------------------------------------------------------------------
def _dev(case, rows=None):
    """the case's tables on the device, once"""
    sel = slice(None) if rows is None else rows
    up = lambda t: t.contiguous().cuda()
    return dict(x=up(case["x"][sel]), gamma=up(case["gamma"]), beta=up(case["beta"]), t2=up(case["t2"]), limg=up(case["limg"]),
                basis=up(case["basis"]), c0=case["c0"])


def _dense(dc, pts):
    """rald_op_ae_decode on pts [B,R,3] (CPU) -> logits [B,R] (CPU); a dc with a 'decode' entry (the module tests) calls that instead"""
    from rald_amd import _handles as Hd
    if "decode" in dc:
        return dc["decode"](pts.contiguous().cuda()).cpu()
    out = Hd.op_ae_decode(dc["x"], dc["gamma"], dc["beta"], dc["t2"], dc["limg"], dc["basis"], dc["c0"], pts.contiguous().cuda())
    return out.cpu()


def _cast(dc, o, d, S, n_refine, points=True):
    """the entry on origins / dirs [R,3] (shared table, stride 0) or [B,R,3] -> (t, logit, step, points or None) on the CPU; the ray tables
    sit before a NaN tail, the outputs are pre-filled and followed by 64 sentinels"""
    from rald_amd import _handles as Hd
    from rald_amd._lib import check
    B = dc["x"].shape[0]
    R = o.shape[-2]
    stride = 3 * R if o.dim() == 3 else 0
    n = o.numel()
    ob, db = (torch.full((n + 192,), NAN, device="cuda") for _ in range(2))
    ob[:n], db[:n] = o.reshape(-1).cuda(), d.reshape(-1).cuda()
    t, lg, pt = _guarded(B * R, 64), _guarded(B * R, 64), (_guarded(B * R * 3, 64) if points else None)
    st = _guarded(B * R, 64, dtype=torch.int32, fill=-7)
    check(Hd.op_ae_cast_rays(dc["x"], dc["gamma"], dc["beta"], dc["t2"], dc["limg"], dc["basis"], dc["c0"], ob[:n], db[:n], stride, S, n_refine,
                             t[:B * R], lg[:B * R], st[:B * R], None if pt is None else pt[:B * R * 3]))
    torch.cuda.synchronize()
    assert _guard_ok(t, B * R) and _guard_ok(lg, B * R) and _guard_ok(st, B * R) and (pt is None or _guard_ok(pt, B * R * 3)), "wrote past an output"
    return (t[:B * R].view(B, R).cpu(), lg[:B * R].view(B, R).cpu(), st[:B * R].view(B, R).cpu(),
            None if pt is None else pt[:B * R * 3].view(B, R, 3).cpu())


def _at(o, t, d):
    """o + t * d in fp32 on the CPU: a rounded product, then a rounded sum (t a 0-dim tensor or [B,R])"""
    return o + (t[..., None] if t.dim() else t) * d


def _march_logits(dc, o, d, S):
    """the dense logits of every march sample: [S+1,B,R]"""
    B = dc["x"].shape[0]
    o, d = (v.expand(B, *v.shape[-2:]) for v in (o, d))
    return torch.stack([_dense(dc, _at(o, torch.tensor(float(k)) / torch.tensor(float(S)), d)) for k in range(S + 1)])


def _replay(dc, o, d, S, n_refine, march=None):
    """The rule of DESIGN section 19 on the host, every logit from the dense decode entry -> (t, logit, step, points) [B,R(,3)]."""
    B = dc["x"].shape[0]
    o, d = (v.expand(B, *v.shape[-2:]).contiguous() for v in (o, d))
    R = o.shape[1]
    step = torch.full((B, R), -1, dtype=torch.int32)
    lo, hi = torch.zeros(B, R), torch.zeros(B, R)
    lh = torch.full((B, R), NAN)
    t_prev = torch.tensor(0.0)
    for k in range(S + 1):
        t = torch.tensor(float(k)) / torch.tensor(float(S))                     # fp32, correctly rounded
        lg = march[k] if march is not None else _dense(dc, _at(o, t, d))
        new = (step < 0) & (lg > 0)                                             # NaN > 0 is False
        step[new], hi[new], lo[new], lh[new] = k, t, t_prev, lg[new]
        t_prev = t
    cross = step >= 1
    for _ in range(n_refine):
        mid = 0.5 * (lo + hi)
        te = torch.where(cross, mid, torch.where(step == 0, hi, torch.ones_like(hi)))
        lg = _dense(dc, _at(o, te, d))
        up, down = cross & (lg > 0), cross & ~(lg > 0)
        hi[up], lh[up] = te[up], lg[up]
        lo[down] = te[down]
    hit = step >= 0
    t_out = torch.where(hit, hi, torch.full_like(hi, -1.0))
    pts = torch.where(hit[..., None], _at(o, hi, d), torch.full_like(o, NAN))
    return t_out, lh, step, pts


def _same(got, want):
    """torch.equal with NaN == NaN (misses carry NaN logits and points)"""
    return got.dtype == want.dtype and got.shape == want.shape and bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all()) \
        if got.is_floating_point() else torch.equal(got, want)


def _assert_equal(got, want, what):
    for name, g, w in zip(("t", "logit", "step", "points"), got, want):
        if g is not None:
            assert _same(g, w), (what, name, int((~((g == w) | ((g != g) & (w != w)))).sum()))


def _rays(B, R, seed, per_sample):
    """segments between two uniform points of the cube: [B,R,3] (per sample) or [R,3] (shared)"""
    shape = (B, R, 3) if per_sample else (R, 3)
    a = torch.rand(shape, generator=_g(seed)) * 2 - 1
    b = torch.rand(shape, generator=_g(seed + 1)) * 2 - 1
    return a, b - a


def _centre(case, dc, o, d, S, quantile):
    """c0 := minus the given quantile of the march's own dense logits (decoded with c0 = 0), so that the level logit = 0 cuts the rays"""
    dc["c0"] = 0.0
    lg = _march_logits(dc, o, d, S)
    dc["c0"] = case["c0"] = -float(torch.quantile(lg.double().flatten(), quantile))
    return dc


def _shares(step):
    n = step.numel()
    return float((step == 0).sum()) / n, float((step >= 1).sum()) / n, float((step < 0).sum()) / n


# ---- 1. equal to the replay -----------------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(dim, M, basis_kind):
    if (dim, M, basis_kind) not in _CASES:
        basis = None if basis_kind == "shipped" else _rotated_basis("dense")
        _CASES[(dim, M, basis_kind)] = _real_case(dim, M, 3, 1, basis=basis, seed=31)[1]
    return dict(_CASES[(dim, M, basis_kind)])


@gpu
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
@pytest.mark.parametrize("basis_kind", ["shipped", "dense"])
@pytest.mark.parametrize("dim,M", [(256, 64), (512, 512)])
def test_equal_to_the_replay(dim, M, basis_kind, per_sample):
    """B = 3, R = 1, 64 and 200 (three full chunks + a tail of 8: the clamp and a nearly empty half), S = 24, n_refine = 6, shared and
    per-sample ray tables, both kernel forms: t, step, logit and points torch.equal to the replay.  c0 is minus the 0.72 quantile of the
    R = 200 march's dense logits; the replay must then hold at least 10 % of the rays in each class (hit at k = 0, hit at k >= 1, miss)."""
    S, n_refine = 24, 6
    case = _case(dim, M, basis_kind)
    o, d = _rays(3, 200, 400 + M, per_sample)
    dc = _centre(case, _dev(case), o, d, S, 0.72)
    for R in (200, 64, 1):
        oo, dd = o[..., :R, :].contiguous(), d[..., :R, :].contiguous()
        want = _replay(dc, oo, dd, S, n_refine)
        if R == 200:
            shares = _shares(want[2])
            print(f"shares {dim}/{M} {basis_kind} per_sample={per_sample}: hit at 0 {shares[0]:.3f}, hit later {shares[1]:.3f}, miss {shares[2]:.3f}")
            assert min(shares) >= 0.10, shares
            assert bool(((want[0][want[2] >= 1] > 0) & (want[0][want[2] >= 1] <= 1)).all())
        _assert_equal(_cast(dc, oo, dd, S, n_refine), want, (R,))
        if R == 64:                                              # without the optional output the others are the same
            _assert_equal(_cast(dc, oo, dd, S, n_refine, points=False), want, (R, "no points"))


@gpu
def test_wave_level_exit_next_to_a_chunk_of_misses():
    """One chunk whose 64 rays all start inside the occupied region (the wave leaves the march at k <= 1) next to a chunk of 64 misses
    (that wave marches to k = S and skips the bisection): equal to the replay.  The rays are picked from a pool of 3000 by the pool's own
    dense march with a margin of 0.01 on the logits, so that other wave-mates (1e-6 on a logit) cannot change a ray's class."""
    S, n_refine = 24, 6
    case = _case(256, 64, "shipped")
    case["x"] = case["x"][:1]
    o, d = _rays(1, 3000, 77, False)
    dc = _centre(case, _dev(case), o, d, S, 0.9)                 # this sample's logits are above the 0.9 quantile somewhere on most rays
    lg = _march_logits(dc, o, d, S)[:, 0]                        # [S+1, 3000]
    inside = torch.nonzero(lg[0] > 0.01)[:, 0]
    never = torch.nonzero(lg.max(0).values < -0.01)[:, 0]
    assert inside.numel() >= 64 and never.numel() >= 64, (inside.numel(), never.numel())
    pick = torch.cat([inside[:64], never[:64]])
    oo, dd = o[pick].contiguous(), d[pick].contiguous()
    want = _replay(dc, oo, dd, S, n_refine)
    assert bool((want[2][0, :64] == 0).all()) and bool((want[2][0, 64:] == -1).all())
    _assert_equal(_cast(dc, oo, dd, S, n_refine), want, "exit")
    # and the other order: the misses first
    pick = torch.cat([never[:64], inside[:64]])
    oo, dd = o[pick].contiguous(), d[pick].contiguous()
    _assert_equal(_cast(dc, oo, dd, S, n_refine), _replay(dc, oo, dd, S, n_refine), "exit, swapped")


@gpu
def test_grid_stride_second_pass_is_the_first_pass_elsewhere():
    """B = 3: 256 / 3 = 85 workgroups of 8 waves per sample take 680 chunks in one pass; R = 680 * 64 + 65 gives two waves a second chunk,
    one of them a single ray.  S = 3, n_refine = 2.  Equal to the replay; and since a chunk's outputs do not depend on where in the grid
    (or in which workgroup width) it runs, the rays from 680 * 64 on equal the launch of those 65 rays alone, bit for bit."""
    S, n_refine = 3, 2
    first = 85 * 8 * 64
    case = _case(256, 64, "shipped")
    o, d = _rays(3, first + 65, 91, False)
    dc = _centre(case, _dev(case), o[:2000], d[:2000], S, 0.72)
    got = _cast(dc, o, d, S, n_refine)
    _assert_equal(got, _replay(dc, o, d, S, n_refine), "grid stride")
    alone = _cast(dc, o[first:].contiguous(), d[first:].contiguous(), S, n_refine)
    _assert_equal([g[:, first:] for g in got], alone, "tail alone")
    assert min(_shares(got[2])) > 0.02


@gpu
@pytest.mark.parametrize("S,n_refine", [(24, 0), (1, 6), (1, 0)])
def test_no_refinement_and_a_single_step(S, n_refine):
    """n_refine = 0 (t is a march sample) and n_steps = 1 (the two end points only): equal to the replay."""
    case = _case(256, 64, "dense")
    o, d = _rays(3, 130, 55, True)
    dc = _centre(case, _dev(case), o, d, 24, 0.72)
    want = _replay(dc, o, d, S, n_refine)
    _assert_equal(_cast(dc, o, d, S, n_refine), want, (S, n_refine))
    if n_refine == 0:
        hit = want[2] >= 0
        assert bool((want[0][hit] == want[2][hit].float() / S).all())


@gpu
def test_nan_origins_miss():
    """Rays with a NaN origin (one coordinate or all) return the miss outputs (-1, NaN, -1, NaN); their chunk-mates equal the replay."""
    S, n_refine = 12, 4
    case = _case(256, 64, "shipped")
    o, d = _rays(3, 100, 66, False)
    dc = _centre(case, _dev(case), o, d, S, 0.72)
    o[3, 1] = NAN
    o[40] = NAN
    o[99, 2] = NAN
    t, lg, st, pt = _cast(dc, o, d, S, n_refine)
    for r in (3, 40, 99):
        assert bool((t[:, r] == -1).all()) and bool(torch.isnan(lg[:, r]).all()) and bool((st[:, r] == -1).all()) and bool(torch.isnan(pt[:, r]).all())
    _assert_equal((t, lg, st, pt), _replay(dc, o, d, S, n_refine), "nan")
    assert int((st >= 0).sum()) > 30


@gpu
def test_1024_latents_are_accepted():
    """num_latents = 1024 (the plain kernel's LDS budget, 140 KiB): B = 2, R = 70, S = 3, n_refine = 2, equal to the replay."""
    case = _real_case(256, 1024, 2, 1, seed=33)[1]
    o, d = _rays(2, 70, 12, False)
    dc = _centre(case, _dev(case), o, d, 3, 0.72)
    _assert_equal(_cast(dc, o, d, 3, 2), _replay(dc, o, d, 3, 2), "M = 1024")


@gpu
def test_refusals_leave_the_outputs_untouched():
    """Bad step counts, a stride that is neither 0 nor 3 R, a ray count of 0, null required pointers: an error through the status / last-error
    path, and every output (sentinel-filled) as it was.  A null out_points is not an error."""
    from rald_amd import _handles as Hd
    from rald_amd._lib import lib
    case = _case(256, 64, "shipped")
    dc = _dev(case)
    B, R = 3, 70
    o, d = (v.cuda() for v in _rays(B, R, 5, False))
    outs = lambda: (torch.full((B * R,), 7.5, device="cuda"), torch.full((B * R,), 7.5, device="cuda"),
                    torch.full((B * R,), 75, device="cuda", dtype=torch.int32), torch.full((B * R * 3,), 7.5, device="cuda"))

    def call(o_=o, d_=d, stride=0, S=8, n_refine=2, drop=None, n_rays=R):
        t, lg, st, pt = outs()
        args = [t, lg, st, pt]
        if drop is not None:
            args[drop] = None
        rc = Hd.op_ae_cast_rays(dc["x"], dc["gamma"], dc["beta"], dc["t2"], dc["limg"], dc["basis"], dc["c0"], o_, d_, stride, S, n_refine,
                                *args, n_rays=n_rays)
        torch.cuda.synchronize()
        return rc, (t, lg, st, pt)

    bad = [dict(S=0), dict(S=65536), dict(S=-3), dict(n_refine=-1), dict(n_refine=31), dict(stride=3), dict(stride=3 * R + 3), dict(stride=-3 * R),
           dict(n_rays=0), dict(n_rays=-5), dict(o_=None), dict(d_=None), dict(drop=0), dict(drop=1), dict(drop=2)]
    for kw in bad:
        rc, (t, lg, st, pt) = call(**kw)
        assert rc != 0 and lib().rald_last_error(), kw
        assert bool((t == 7.5).all()) and bool((lg == 7.5).all()) and bool((st == 75).all()) and bool((pt == 7.5).all()), kw
    rc, (t, lg, st, pt) = call(drop=3)
    assert rc == 0 and bool((t != 7.5).all()) and bool((st != 75).all()) and bool((pt == 7.5).all())
    rc, (t, lg, st, pt) = call(o_=o.expand(B, R, 3).contiguous(), d_=d.expand(B, R, 3).contiguous(), stride=3 * R)
    assert rc == 0 and bool((st != 75).all())


# ---- 2. geometry, without the decoder as its own reference ---------------------------------------------------------------------------------
# the fp16 term of the geometry bound, in t.  Measured on an MI355X: worst |t_hit - t*| 8.902e-5 with a bracket of 4.246e-5, so 4.656e-5
# beyond the bracket; the bound is 2.47 x that.  (A priori the term cannot exceed 2^-12 / 1.9375 = 1.26e-4, see the docstring.)
FP16_TERM_MEASURED = 4.656e-5
FP16_TERM_BOUND = 1.15e-4


@gpu
def test_first_return_lies_on_the_mid_plane_of_a_sign_grid():
    """The _onehot_case field (M = 128: a grid of 8 x 4 x 4 points, the softmax one-hot on the nearest) with u_l = +-1 by a seeded pattern
    and c0 = 0: the logit is the sign of the nearest grid point's u, and the zero level sits on the mid-planes x = j / 4 between cells of
    different sign (the score gap grows by 2^13 log2 units per unit of distance from the plane).  128 rays along axis 0, both directions,
    from |x| = 0.96875 over a length of 1.9375, at (y, z) = cell centre +- 0.2 cell; S = 23 makes a step of 0.084, a third of the cell
    width in x, and no sample lies within 0.03 of a mid-plane.  For every ray: the step, and with it the hit cell, equal the
    float64 nearest-cell walk over the samples (first sample whose cell has u = +1; a row without such a cell is a miss); the returned
    point lies between that cell's near face and the hit sample; and
    |t_hit - t*| <= 1 / (S 2^n_refine) + FP16_TERM_BOUND against the analytic crossing t* of that cell's near mid-plane (t* = 0 for a
    ray that starts inside a positive cell).  The second term is the fp16 rounding of the x feature: the field sees fl16(x), and the
    mid-planes with |x| in [0.5, 1) sit half an fp16 ulp = 2^-12 wide, 2^-12 / 1.9375 = 1.26e-4 in t at the most; measured 4.656e-5, bound
    1.15e-4 (2.47 x)."""
    M, S, n_refine = 128, 23, 10
    case, _, perm, _ = _onehot_case(M)
    nx = M // 16
    sign = torch.where(torch.rand(M, generator=_g(808)) < 0.5, -1.0, 1.0)                    # by grid cell (ix, iy, iz), row-major
    sign.view(nx, 4, 4)[:, 0, 0] = -1.0                                                      # two rows without a positive cell: misses
    sign.view(nx, 4, 4)[:, 3, 2] = -1.0
    u = sign[perm]                                                                           # latent l owns grid cell perm[l]
    t2 = case["t2"].clone()
    for l in range(M):
        t2[4 + l, SLOT_U] = float(u[l])
    case = dict(case, t2=t2, c0=0.0)
    gy = torch.tensor([-0.75, -0.25, 0.25, 0.75], dtype=torch.float64)
    rows = []
    for iy in range(4):
        for iz in range(4):
            for sy, sz in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
                for direction in (1.0, -1.0):
                    rows.append((iy, iz, float(gy[iy]) + sy * 0.1, float(gy[iz]) + sz * 0.1, direction))
    R = len(rows)
    assert R == 128
    o = torch.tensor([[-0.96875 * dr, y, z] for _, _, y, z, dr in rows], dtype=torch.float32)
    d = torch.tensor([[1.9375 * dr, 0.0, 0.0] for *_, dr in rows], dtype=torch.float32)
    t, lg, st, pt = _cast(_dev(case), o, d, S, n_refine)
    # float64 walk over the samples
    cell_sign = sign.view(nx, 4, 4).double()
    worst, gap = 0.0, 1.0
    for r, (iy, iz, _, _, dr) in enumerate(rows):
        xs = [-0.96875 * dr + (k / S) * 1.9375 * dr for k in range(S + 1)]
        ix = [min(max(int(math.floor((x + 1) * nx / 2)), 0), nx - 1) for x in xs]
        gap = min(gap, min(abs(x - (2 * j / nx - 1)) for x in xs for j in range(1, nx)))
        first = next((k for k in range(S + 1) if cell_sign[ix[k], iy, iz] > 0), None)
        if first is None:
            assert st[0, r] == -1 and t[0, r] == -1 and math.isnan(lg[0, r]) and bool(torch.isnan(pt[0, r]).all()), r
            continue
        assert int(st[0, r]) == first, (r, int(st[0, r]), first)
        assert ix[int(st[0, r])] == ix[first] and float(lg[0, r]) > 0, (r, ix[int(st[0, r])], ix[first])       # the hit cell
        px = float(pt[0, r, 0])
        if first == 0:
            assert float(t[0, r]) == 0.0 and px == xs[0]
            continue
        plane = 2 * (ix[first] if dr > 0 else ix[first] + 1) / nx - 1                        # the positive cell's face towards the origin
        t_star = (plane - (-0.96875 * dr)) / (1.9375 * dr)
        worst = max(worst, abs(float(t[0, r]) - t_star))
        # the returned point: between that face (the field sees fl16(x): up to the fp16 term in front of it) and the hit sample
        assert (px - plane) * dr >= -FP16_TERM_BOUND * 1.9375 and (xs[first] - px) * dr >= -1e-6, (r, px, plane, xs[first])
    bracket = 1.0 / (S * 2 ** n_refine)
    n_hit0, n_cross, n_miss = int((st == 0).sum()), int((st >= 1).sum()), int((st < 0).sum())
    print(f"ratio geometry: worst |t_hit - t*| {worst:.4g}, bracket {bracket:.4g}, fp16 term (worst - bracket) {worst - bracket:.4g}, "
          f"bound {bracket + FP16_TERM_BOUND:.4g}; {n_hit0} start inside, {n_cross} cross, {n_miss} miss; nearest sample to a mid-plane {gap:.3g}")
    assert gap > 0.03 and n_cross >= 32 and n_hit0 >= 16 and n_miss >= 2
    assert worst <= bracket + FP16_TERM_BOUND
