"""The ICP reference (tests/icp_ref.py) held against its independent second route by bits on every case of tests/test_gpu_icp.py
(the candidates from the grid's scan range, the dense term array summed at once, the factorisation row by row), what each
construction is for shown on the reference alone (so the GPU test needs no tolerance: it compares with a reference that is known to
recover the planted motion), the five one-line mutations of DESIGN.md section 27 shown to change the named construction's result,
and the argument rules of the new postprocess entries (ValueError before any device use).  No GPU, no library."""
import numpy as np
import pytest
import torch

import icp_ref as REF
import knn_ref

F32, F64 = np.float32, np.float64
KEYS = ("transform", "stats", "info", "corr", "moved")


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint64) if v.dtype == F64 else (v.view(np.uint32) if v.dtype == F32 else v)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS)


def _one(pair, **kw):
    return REF.icp_one(pair["src"], pair["tgt"], pair["grid"], pair["max_dist"], normals=pair["normals"], **kw)


@pytest.mark.parametrize("name", list(REF.CASES))
def test_two_routes_agree(name):
    pair, kw, ref = REF.case(name)
    assert _same(ref, _one(pair, route=1, **kw)), name


def test_fixed_sum_routes():
    """The dense sum at once against knn_ref.fixed_sum per column, on values whose sum depends on the order."""
    rs = np.random.RandomState(1)
    for n in (0, 1, 1023, 1024, 1025, 3000):
        v = np.where(rs.rand(n, REF.NS) < 0.01, 2.0 ** 53, 1.0) * rs.choice([-1.0, 1.0], (n, REF.NS))
        assert np.array_equal(REF.sums(v, 0), REF.sums(v, 1))
        assert REF.sums(v, 1)[3] == knn_ref.fixed_sum(v[:, 3])


def test_solve_and_update():
    """The fixed-order Cholesky against numpy's solver on a well-conditioned system; the Cayley update is a rotation for every step,
    and for a small step the rotation by |w| about w to second order."""
    rs = np.random.RandomState(2)
    J = rs.normal(size=(50, 6))
    A, g = J.T @ J, J.T @ rs.normal(size=50)
    S = np.concatenate([[A[i, j] for i in range(6) for j in range(i, 6)], g, [0.0, 0.0]])
    x = REF.solve(S)
    assert np.allclose(x, np.linalg.solve(A, -g), rtol=1e-12, atol=0) and np.array_equal(x, REF.solve(S, route=1))
    for scale in (1e-3, 1.0, 1e3):
        step = np.concatenate([rs.normal(size=3) * scale, rs.normal(size=3)])
        T = REF.update(REF.IDENTITY, step)
        Rm = T[:9].reshape(3, 3)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rm) - 1) < 1e-14 and np.array_equal(T[9:], step[3:])
    w = np.array([1e-3, -2e-3, 5e-4])
    Rm = REF.update(REF.IDENTITY, np.concatenate([w, np.zeros(3)]))[:9].reshape(3, 3)
    assert np.abs(Rm - REF.rotation(w, np.degrees(np.linalg.norm(w)))).max() < 1e-8      # the Cayley angle is 2 atan(|w| / 2)


@pytest.mark.parametrize("motion", list(REF.MOTIONS))
@pytest.mark.parametrize("mode", ("plane", "point"))
def test_faces_recover_the_motion(motion, mode):
    """Status 1 within 30 iterations, the motion to within 1e-3 degrees and 1e-5 m (the source is rounded to fp32 at coordinates below
    8 m, 2.4e-7 m a row; the bounds are about 40 times that and its lever over 4 m), fitness exactly 1, R R^T = I to 1e-14."""
    pair, kw, ref = REF.case(f"faces_{motion}_{mode}")
    assert np.abs(pair["src"]).max() < 8 and len(pair["tgt"]) == 3000 and len(pair["src"]) == 1000
    deg, metres = REF.motion_error(ref["transform"], pair["Rm"], pair["tm"])
    print(f"faces {motion} {mode}: status {ref['info'][0]}, {ref['info'][1]} iterations, {deg:.2e} degrees, {metres:.2e} m, rmse {ref['stats'][1]:.2e}")
    assert ref["info"][0] == 1 and ref["info"][1] < 30 and ref["info"][2] == 1000
    assert deg < 1e-3 and metres < 1e-5
    assert ref["stats"][0] == 1.0
    M = ref["transform"].reshape(4, 4)
    assert np.abs(M[:3, :3] @ M[:3, :3].T - np.eye(3)).max() < 1e-14 and M[3].tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("mode", ("plane", "point"))
def test_overlap(mode):
    """The 300 extra rows are farther than max_distance from every target row at EVERY iteration (their correspondence is -1 in every
    step 2 of the trace), fitness is exactly 1000 / 1300, and the transform is the one without them."""
    pair, kw, ref = REF.case(f"overlap_{mode}")
    trace = []
    again = _one(pair, trace=trace, **kw)
    assert _same(ref, again) and len(trace) == ref["info"][1] and all((corr[1000:] == -1).all() for corr, _ in trace)
    assert ref["stats"][0] == 1000 / 1300 and (ref["corr"][1000:] == -1).all() and ref["info"][2] == 1000
    assert np.array_equal(ref["transform"], REF.case(f"faces_small_{mode}")[2]["transform"])


def test_tie():
    """Midway between two and between eight lattice rows the candidates' d2 are equal in fp32 (shown), and the lowest row wins."""
    pair, kw, ref = REF.case("tie_eval")
    d2 = REF._d2(pair["src"], pair["tgt"])
    ties = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
    assert (ties[:60] == 2).all() and (ties[60:] == 8).all()
    assert np.array_equal(ref["corr"], d2.argmin(axis=1)) and ref["info"].tolist() == [2, 0, 120]
    assert (np.diff(np.sort(ref["corr"])) >= 0).all() and len(set(ref["corr"].tolist())) > 30


def test_edge():
    """Even source rows lie at exactly d2 == fl(max_dist^2) and count; odd ones, one float farther along the axis (d2 one part in 2^21
    or 2^20 larger), do not."""
    pair, kw, ref = REF.case("edge_eval")
    d2 = REF._d2(pair["src"], pair["tgt"]).min(axis=1)
    r2 = F32(F32(0.5) * F32(0.5))
    assert (d2[0::2] == r2).all() and (d2[1::2] > r2).all() and (d2[1::2] <= r2 * F32(1 + 2.0 ** -20)).all()
    assert ref["corr"].tolist() == [0, -1, 1, -1, 2, -1, 3, -1, 4, -1, 5, -1, 6, -1] and ref["stats"][0] == 0.5 and ref["stats"][1] == 0.5


def test_planar_and_line():
    """Plane mode on an exact plane: three columns of J are exactly zero, the pivot rule refuses at iteration 0 and the transform is
    the identity's bits; point mode converges to the motion.  The line: the smallest eigenvalue of the normal matrix is about 1e-13 of
    the largest - positive, above the rounding noise, below the floor."""
    pair, kw, ref = REF.case("planar_plane")
    assert ref["info"].tolist() == [3, 0, 600] and ref["transform"].tolist() == np.eye(4).reshape(-1).tolist() and ref["stats"][2] == 0.0
    pair, kw, ref = REF.case("planar_point")
    deg, metres = REF.motion_error(ref["transform"], pair["Rm"], pair["tm"])
    assert ref["info"][0] == 1 and deg < 1e-3 and metres < 1e-5
    pair, kw, ref = REF.case("line_point")
    assert ref["info"].tolist() == [3, 0, 400]
    pp, pf = REF.move(REF.IDENTITY, pair["src"])
    corr = REF.correspond(pf, np.ones(400, bool), pair["tgt"], np.ones(400, bool), pair["grid"], pair["max_dist"])
    ev = np.linalg.eigvalsh(REF._matrix(REF.sums(REF.terms(pp, corr, pair["tgt"], None, 0)[0])))
    assert 1e-16 * ev[-1] < ev[0] < 2.0 ** -30 * ev[-1]


def test_few_and_bad_rows():
    for n, status in ((0, 2), (1, 2), (5, 2), (6, 1)):
        pair, kw, ref = REF.case(f"few_{n}")
        assert ref["info"][0] == status and ref["info"][2] == n and (status == 1 or ref["transform"].tolist() == np.eye(4).reshape(-1).tolist())
        assert ref["stats"][0] == F64(n) / F64(6 + n) and np.isfinite(pair["src"]).all(axis=1).sum() == 6 + n
    for tgt, src in ((0, 10), (10, 0), (0, 0)):
        f = REF.faces()
        one = REF.icp_one(f["src"][:src], f["tgt"][:tgt], f["grid"], f["max_dist"], 1, f["normals"][:tgt], init=np.arange(12.0))
        assert one["info"].tolist() == [2, 0, 0] and one["stats"].tolist() == [0, 0, 0, 0]
        assert one["transform"].tolist() == [0, 1, 2, 9, 3, 4, 5, 10, 6, 7, 8, 11, 0, 0, 0, 1]
    pair, kw, ref = REF.case("bad_rows_plane")
    point = REF.case("bad_rows_point")[2]
    bad_n = ~(np.isfinite(pair["normals"]).all(axis=1) & (pair["normals"] != 0).any(axis=1))
    out_t = ~np.isfinite(pair["tgt"]).all(axis=1) | (pair["tgt"] > 50).any(axis=1)
    assert ref["info"][0] == 1 and point["info"][0] == 1 and bad_n.sum() > 400 and out_t.sum() == 4
    assert (ref["corr"][[3, 500, 999]] == -1).all() and not out_t[ref["corr"][ref["corr"] >= 0]].any()
    assert ref["info"][2] == (~bad_n[ref["corr"][ref["corr"] >= 0]]).sum() < point["info"][2] == 997     # the normal decides in plane mode only


def test_layout_cases():
    """A pair's result does not depend on its place in a batch; counts and bounds cut the clouds; init is where the iteration starts."""
    f, g = REF.faces("small"), REF.faces("large")
    r = REF.ragged_of([f, dict(f, src=f["src"][:0]), g])
    kw = dict(grid=REF.FACES_GRID, max_dist=REF.FACES_DIST, mode=1)
    out = REF.icp_ragged(r["src"], r["src_off"], r["tgt"], r["tgt_off"], max_src=r["max_src"], max_tgt=r["max_tgt"], normals=r["normals"],
                         src_counts=r["src_counts"], tgt_counts=r["tgt_counts"], **kw)
    assert np.array_equal(out["transform"][0], REF.case("faces_small_plane")[2]["transform"])
    assert np.array_equal(out["transform"][2], REF.case("faces_large_plane")[2]["transform"]) and out["info"][1].tolist() == [2, 0, 0]
    assert out["untouched"].sum() == 9 and np.isnan(r["src"][out["untouched"]]).all()
    short = REF.icp_ragged(r["src"], r["src_off"], r["tgt"], r["tgt_off"], max_src=400, max_tgt=r["max_tgt"], normals=r["normals"],
                           tgt_counts=r["tgt_counts"], **kw)
    assert short["info"][:, 2].tolist() == [400, 0, 400] and short["untouched"].sum() == len(r["src"]) - 803     # without counts the gap is the middle cloud


# ---- the mutation checks of DESIGN.md section 27 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation, names", (("lt", ("edge_eval", "edge_step")), ("tie_high", ("tie_eval", "tie_step_point")),
                                             ("converge_before", ("faces_small_plane", "faces_large_point")),
                                             ("no_floor", ("line_point",))))
def test_mutations_change_the_named_cases(mutation, names):
    for name in names:
        pair, kw, ref = REF.case(name)
        assert not _same(ref, _one(pair, mutate=mutation, **kw)), (mutation, name)


def test_mutation_batch_blocks():
    """Blocks counted from the batch's first row instead of the cloud's: the sums of a cloud that does not start at a multiple of 1024
    take another shape, and the transform's bits change for the pairs of the GPU test's batch behind the first."""
    f, g = REF.faces("small", n_src=1000), REF.faces("large")
    src, so = np.concatenate([f["src"], g["src"]]), [0, 1000, 2000]
    tgt, to = np.concatenate([f["tgt"], g["tgt"]]), [0, 3000, 6000]
    kw = dict(grid=REF.FACES_GRID, max_dist=REF.FACES_DIST, max_src=1000, max_tgt=3000, mode=0)
    a = REF.icp_ragged(src, so, tgt, to, **kw)
    b = REF.icp_ragged(src, so, tgt, to, mutate="batch_blocks", **kw)
    assert np.array_equal(a["transform"][0], b["transform"][0]) and not np.array_equal(a["transform"][1], b["transform"][1])


# ---- the argument rules of the Python layer --------------------------------------------------------------------------------------------
def test_python_argument_errors():
    from rald_amd import postprocess as PP
    p, q = torch.zeros(10, 3), torch.zeros(20, 3)
    off = torch.tensor([0, 10]), torch.tensor([0, 20])
    grid = PP.voxel_grid((0, 0, 0), (1, 1, 1), 0.5)
    good = dict(max_distance=0.5, grid=grid, max_source=10, max_target=20)
    call = lambda **kw: PP.register_icp_ragged(p, off[0], q, off[1], **dict(good, **kw))
    for bad in (dict(max_distance=0), dict(max_distance=float("nan")), dict(max_distance="1"), dict(max_distance=1e39), dict(max_distance=0.6),
                dict(max_source=0), dict(max_target=2 ** 24 + 1), dict(grid=(grid[0], grid[1])), dict(mode="plane"), dict(mode=2), dict(mode=True),
                dict(target_normals=torch.zeros(19, 3)), dict(init=torch.zeros(1, 12)), dict(init=torch.zeros(2, 12, dtype=torch.float64)),
                dict(max_iterations=0), dict(max_iterations=65), dict(max_iterations=1.5), dict(tolerance=-1e-9), dict(tolerance=float("nan")),
                dict(min_correspondences=0), dict(chunk=1000), dict(source_counts=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):
        PP.register_icp_ragged(p, off[0], q, torch.tensor([0, 10, 20]), **good)
    with pytest.raises(ValueError):
        PP.register_icp_ragged(p[:, :2], off[0], q, off[1], **good)
    with pytest.raises(RuntimeError):                                   # every rule passed: only now the device is asked for
        call()
    for bad in (dict(max_distance=-1), dict(mode="planes"), dict(init=torch.zeros(3, 4, dtype=torch.float64)), dict(max_iterations=100),
                dict(lo=(0, 0, 0)), dict(target_normals=torch.zeros(3, 3), mode="plane")):
        with pytest.raises(ValueError):
            PP.register_icp(p, q, **dict(dict(max_distance=0.5), **bad))
    with pytest.raises(ValueError):
        PP.register_icp(p, q, 0.5, mode="plane")
    M = torch.eye(4, dtype=torch.float64)
    for bad in (dict(transforms=M), dict(transforms=M[None].float()), dict(max_per_sample=0), dict(normals=torch.zeros(9, 3))):
        with pytest.raises(ValueError):
            PP.transform_points_ragged(p, off[0], **dict(dict(transforms=M[None], max_per_sample=10), **bad))
    for bad in ((p, M.float()), (p, M[:3]), (p[:, :2], M)):
        with pytest.raises(ValueError):
            PP.transform_points(*bad)
    with pytest.raises(RuntimeError):
        PP.transform_points(p, M)
