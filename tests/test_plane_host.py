"""The plane segmentation's reference (tests/plane_ref.py) held against an independent route on every construction of
tests/test_gpu_plane.py, what each construction is for shown on the reference alone (so the GPU test needs no tolerance: it compares
with a reference that is known to find the planted planes), the four one-line mutations of DESIGN.md section 26 shown to change
the named construction's result, the argument rules of the new postprocess / engine_generation entries (ValueError before any
device use), and the tail's option lattice with `remove_planes` on stubs.  No GPU, no library."""
import itertools

import numpy as np
import pytest
import torch

import plane_ref as REF

F32, F64 = np.float32, np.float64
KEYS = ("labels", "planes", "num_planes", "inliers", "best")


def _same(a, b):
    bits = lambda v: np.asarray(v, F64).view(np.uint64) if np.asarray(v).dtype == F64 else np.asarray(v)
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in KEYS)


def _both(p, **kw):
    one = REF.segment_one(p, **kw)
    assert _same(one, REF.segment_one_alt(p, **kw)), kw
    return one


def test_philox_known_answer():
    """Random123's known-answer vector of philox4x32_10 for counter 0, key 0, and for all-ones; both routes."""
    import churn_ref
    kat = {(0, 0): [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], (0xFFFFFFFF, 0xFFFFFFFF): [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]}
    for (c, k), want in kat.items():
        assert REF.philox_int((c,) * 4, (k, k)) == want
        assert churn_ref.philox4x32_10(np.full((1, 4), c, np.uint64), np.full((1, 2), k, np.uint64))[0].tolist() == want


def test_fixed_sum_is_the_header_shape():
    """The restated sum against knn_ref.fixed_sum, on values whose sum depends on the order (2^53 beside ones)."""
    import knn_ref
    rs = np.random.RandomState(1)
    for n in (0, 1, 1023, 1024, 1025, 3000):
        v = np.where(rs.rand(n) < 0.01, 2.0 ** 53, 1.0) * rs.choice([-1.0, 1.0], n)
        assert REF.fixed_sum(v) == knn_ref.fixed_sum(v)


def test_tiny():
    p, off = REF.tiny_clouds()
    assert off == [0, 0, 1, 3, 6, 9, 12]
    for refine in (False, True):
        found = [_both(p[off[b]:off[b + 1]], **dict(REF.TINY, refine=refine)) for b in range(6)]
        assert [f["num_planes"] for f in found] == [0, 0, 0, 1, 0, 0]
        assert found[3]["labels"].tolist() == [0, 0, 0] and found[3]["inliers"].tolist() == [3, 0] and found[3]["best"][0] >= 0
        for b in (0, 1, 2, 4, 5):
            assert np.isnan(found[b]["planes"]).all() and (found[b]["best"] == -1).all() and (found[b]["labels"] == -1).all()
    hyp = REF.hypotheses(p[6:9], 0, 64, 0, 0.01)                          # collinear: every hypothesis is degenerate, none is valid
    assert not hyp["valid"].any() and (hyp["len2"] == 0).all()


@pytest.mark.parametrize("n", REF.SLAB_SIZES)
def test_slab_rows_at_the_bound(n):
    """Without refine the winner has n = (0, 0, nz) exactly; rows at +-t are inliers (equality in fp32), rows one part in 2^22 farther
    are not, and `<` in place of `<=` loses the former."""
    p, far = REF.slab_cloud(n)
    one = _both(p, **REF.SLAB)
    z = np.abs(p[:, 2])
    assert far > F32(REF.T_SLAB) and far == F32(REF.T_SLAB) * (F32(1) + F32(2.0 ** -22))
    assert one["num_planes"] == 1 and one["planes"][0, :2].tolist() == [0.0, 0.0] and abs(one["planes"][0, 2]) == 1.0 and one["planes"][0, 3] == 0.0
    assert (one["labels"][z <= F32(REF.T_SLAB)] == 0).all() and (one["labels"][z == far] == -1).all()
    assert (z == F32(REF.T_SLAB)).sum() > 20 and (z == far).sum() > 10
    hyp = REF.hypotheses(p, 0, REF.SLAB["H"], 0, REF.SLAB["t"])           # every row is usable: the live rows are the cloud
    assert not REF.inliers_of(p, hyp, one["best"][0], strict=True)[z == F32(REF.T_SLAB)].any()
    assert not np.array_equal(REF.segment_one(p, strict=True, **REF.SLAB)["labels"], one["labels"])
    _both(p, **dict(REF.SLAB, refine=True))


def test_tie_goes_to_the_smaller_hypothesis():
    p = REF.tie_cloud()
    one = _both(p, **REF.TIE)
    tied = one["ties"][0]
    hyp = REF.hypotheses(p, 0, REF.TIE["H"], 0, REF.TIE["t"])
    on_upper = [bool(hyp["p0"][h][2] == 4.0) for h in tied]
    assert one["top"] == [300] and len(tied) >= 2 and any(on_upper) and not all(on_upper)      # both planes reach the top score
    assert one["best"][0] == tied[0] == 0 and not on_upper[0] and one["planes"][0].tolist() == [0.0, 0.0, 1.0, 0.0]
    other = REF.segment_one(p, tie="largest", **REF.TIE)
    assert other["best"][0] == tied[-1] and on_upper[-1] and not np.array_equal(other["labels"], one["labels"])


@pytest.mark.parametrize("order", ("built", "reversed", "shuffled"))
def test_faces_come_by_size(order):
    p, truth = REF.faces_cloud(order)
    one = _both(p, **REF.FACES)
    assert one["num_planes"] == 3 and np.array_equal(one["labels"], truth) and one["inliers"].tolist() == [576, 400, 256, 0]
    for k, axis in enumerate((2, 1, 0)):                                  # every face found: its normal is its axis, it passes through 0
        assert abs(abs(one["planes"][k][axis]) - 1.0) < 1e-12 and abs(one["planes"][k][3]) < 1e-12
    assert np.isnan(one["planes"][3]).all() and one["best"][3] == -1
    # min_inliers is the smallest face's size exactly: compared with `>` the third plane is lost
    assert REF.FACES["min_inliers"] == 256 and REF.segment_one(p, min_cmp="not_above", **REF.FACES)["num_planes"] == 2


@pytest.mark.parametrize("refine", (False, True))
def test_noisy_plane_is_found(refine):
    """The planted plane's normal within 1 degree at H = 256, turned to the view on either side; NaN / inf rows are -2."""
    p, nrm, centre = REF.noisy_cloud()
    for side in (1.0, -1.0):
        one = _both(p, **dict(REF.NOISY, refine=refine, view=(centre + side * 5.0 * nrm).astype(F32).tolist()))
        cos = float(one["planes"][0, :3] @ nrm)
        assert one["num_planes"] == 1 and side * cos > np.cos(np.radians(1.0)) and one["inliers"][0] > 1300
        assert abs(np.linalg.norm(one["planes"][0, :3]) - 1.0) < 1e-12
        assert (one["labels"] == -2).sum() == 12 and (one["labels"][~np.isfinite(p).all(axis=1)] == -2).all()
    for H in (1, 63, 65):
        _both(p, **dict(REF.NOISY, refine=refine, H=H, min_inliers=3))
    low = REF.segment_one(p, **dict(REF.NOISY, refine=refine, seed=5))
    assert _same(low, REF.segment_one(p, **dict(REF.NOISY, refine=refine, seed=(7 << 32) + 5)))
    assert low["best"][0] != REF.segment_one(p, **dict(REF.NOISY, refine=refine, seed=6))["best"][0]


def test_batch_position_does_not_show():
    """The batch of tests/test_gpu_plane.py: every cloud's result is its one-cloud result (segment_ragged runs segment_one per cloud: the
    reference cannot see a batch position), clouds behind the first find planes, and the trimmed and dense forms are what the GPU test
    expects."""
    faces, _ = REF.faces_cloud("shuffled")
    noisy, _, _ = REF.noisy_cloud()
    slab, _ = REF.slab_cloud(1025)
    clouds = [faces, np.zeros((0, 3), F32), noisy[:1400], np.zeros((0, 3), F32), slab]
    off = [0] + np.cumsum([len(c) for c in clouds]).tolist()
    kw = dict(t=0.05, H=128, K=3, min_inliers=200, refine=True, seed=11)
    ref = REF.segment_ragged(np.concatenate(clouds), off, max_per_sample=1500, **kw)
    assert ref["num_planes"].tolist() == [3, 0, 1, 0, 1] and not ref["untouched"].any()
    assert all(ref["best"][b, 0] >= 0 for b in (0, 2, 4))               # clouds behind the first have planes: a counter that held b would show
    cut = REF.segment_ragged(np.concatenate(clouds), off, max_per_sample=1000, counts=[1000, 5, 1024, 0, 1025], **kw)
    assert cut["untouched"].sum() == (1332 - 1000) + 400 + 25
    dense = np.concatenate([faces[:700], noisy[:700], slab[:700], faces[500:1200]])
    assert REF.segment_ragged(dense, [0, 700, 1400, 2100, 2800], max_per_sample=700, **kw)["num_planes"].min() >= 1
    keep = REF.filter_ragged(np.concatenate(clouds), off, max_per_sample=1500, keep_planes=True, labelled=ref, **kw)
    drop = REF.filter_ragged(np.concatenate(clouds), off, max_per_sample=1500, keep_planes=False, labelled=ref, **kw)
    assert keep["offsets"][-1] + drop["offsets"][-1] == off[-1] - 12 + (~np.isfinite(noisy[1400:]).all(axis=1)).sum()
    assert (keep["labels"] >= 0).all() and (drop["labels"] == -1).all()


# ---- the argument rules -----------------------------------------------------------------------------------------------------------------------
def test_postprocess_argument_rules():
    """Every rule is a ValueError raised before anything asks where a tensor lives: the tensors here are on the host."""
    from rald_amd import postprocess as PP
    p, off = torch.zeros(10, 3), torch.tensor([0, 10])
    ok = dict(threshold=0.1, max_per_sample=10)
    bad = [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold="0.1"),
           dict(threshold=True), dict(threshold=1e-60), dict(num_hypotheses=0), dict(num_hypotheses=65537), dict(num_hypotheses=2.5),
           dict(num_hypotheses=True), dict(max_planes=0), dict(max_planes=9), dict(min_inliers=2), dict(min_inliers=3.5), dict(refine=2),
           dict(refine="yes"), dict(seed=1.5), dict(seed=2 ** 63), dict(view=(0, 0)), dict(view=(0, float("nan"), 0)), dict(view=(1e39, 0, 0)),
           dict(max_per_sample=0), dict(counts=torch.zeros(2, dtype=torch.int32))]
    for fn in (PP.segment_planes_ragged, PP.remove_planes_ragged):
        for b in bad:
            with pytest.raises(ValueError):
                fn(p, off, **{**ok, **b})
        with pytest.raises(ValueError):
            fn(torch.zeros(10, 2), off, **ok)
        with pytest.raises(ValueError):
            fn(p, torch.tensor([0.0, 10.0]), **ok)
    for fn in (PP.segment_plane, PP.remove_planes):
        for b in (dict(threshold=0.0), dict(num_hypotheses=0), dict(min_inliers=1), dict(refine=None), dict(seed="a"), dict(view=(1, 2))):
            with pytest.raises(ValueError):
                fn(p, **{**dict(threshold=0.1), **b})
        with pytest.raises(ValueError):
            fn(torch.zeros(10), 0.1)
    with pytest.raises(ValueError):
        PP.remove_planes(p, 0.1, max_planes=9)
    assert PP.PLANE_MAX_HYPOTHESES == 65536 and PP.PLANE_MAX_PLANES == 8
    plane, idx = PP.segment_plane(torch.zeros(0, 3), 0.1)                 # an empty cloud needs no device
    assert plane.dtype == torch.float64 and bool(torch.isnan(plane).all()) and idx.numel() == 0 and idx.dtype == torch.int64
    assert PP.remove_planes(torch.zeros(0, 3), 0.1).shape == (0, 3)


def test_engine_argument_rules():
    from rald_amd import engine_generation as E
    gen = torch.Generator().manual_seed((9 << 32) + 77)
    assert E._check_remove_planes(None, None, None, None, gen) is None
    assert E._check_remove_planes((0.2, 256), None, None, None, None) == ("plane", 0.2, 256, 1, False, 0)
    assert E._check_remove_planes([0.2, 256.0, 3], None, None, None, gen) == ("plane", 0.2, 256, 3, False, 77)
    assert E._check_remove_planes((0.2, 256, 3, True), None, None, None, gen) == ("plane", 0.2, 256, 3, True, 77)
    for bad in (0.2, (0.2,), (0.2, 256, 1, False, 0), (0.0, 256), (0.2, 0), (0.2, 65537), (0.2, 256, 0), (0.2, 256, 9), (0.2, 256, 1, "no"),
                ("a", 256), (float("nan"), 256)):
        with pytest.raises(ValueError):
            E._check_remove_planes(bad, None, None, None, None)
    for others in ((object(), None, None), (None, object(), None), (None, None, object())):
        with pytest.raises(ValueError, match="excludes"):
            E._check_remove_planes((0.2, 256), *others, None)


# ---- the tail on stubs ------------------------------------------------------------------------------------------------------------------------
def _stub_planes(monkeypatch):
    from rald_amd import postprocess as real
    from test_infer_tail_host import _stub_all
    E, calls, reads, pos, kw = _stub_all(monkeypatch)
    seen = {}

    def planes(pts, off, threshold, max_per_sample, num_hypotheses=1024, max_planes=1, min_inliers=3, refine=True, seed=0, view=None,
               counts=None, keep_planes=False, return_index=False, return_labels=False):
        calls.append("remove_planes_ragged")
        seen.update(args=(threshold, max_per_sample, num_hypotheses, max_planes, min_inliers, refine, seed, view, keep_planes), pts=pts, off=off)
        assert return_index and return_labels
        pl = torch.arange(2 * max_planes * 4, dtype=torch.float64).reshape(2, max_planes, 4) / 8
        pl[1, max_planes - 1] = float("nan")
        return (torch.full((pts.shape[0], 3), 3.0), torch.tensor([0, 4, 6]), torch.arange(pts.shape[0]) * 2,
                torch.arange(pts.shape[0], dtype=torch.int32) % 3 - 1, pl, torch.tensor([max_planes, max_planes - 1], dtype=torch.int32))
    E.PP.remove_planes_ragged = planes
    E.PP.PLANE_MAX_HYPOTHESES, E.PP.PLANE_MAX_PLANES = real.PLANE_MAX_HYPOTHESES, real.PLANE_MAX_PLANES
    return E, calls, reads, pos, kw, seen


def test_tail_lattice_with_remove_planes(monkeypatch):
    """{Chamfer, metric_thresholds} x {no normals, normals} x thin x resample x {surfaces, none} with remove_planes: every key of the
    dict is the slice or the host copy of the device tuple's element, one host read per call, none in the device form; thin and
    resample run on the filter's result."""
    from test_infer_tail_host import _metrics_match, _same as same
    E, calls, reads, pos, kw, seen = _stub_planes(monkeypatch)
    B, combos = 2, 0
    for taus, normals, thin, resample, surf in itertools.product((None, (0.1, 0.2)), (False, True), (None, 4.0), (None, 5), (True, False)):
        opts = dict(remove_planes=(0.25, 128, 2, True), metric_thresholds=taus, thin=thin, resample=resample, normals=normals)
        k = {**kw, **opts, **({} if surf else {"surfaces": None})}
        del reads[:], calls[:]
        dev = list(E.infer_point_clouds_device(*pos, **k))
        assert not reads and calls.count("remove_planes_ragged") == 1, opts
        assert seen["args"] == (0.25, 50, 128, 2, 3, True, 0, (0.0, 0.0, 0.0), True)
        after = calls[calls.index("remove_planes_ragged") + 1:]
        assert [c for c in after if c in ("voxel_downsample_ragged", "resample_points_ragged")] == \
            (["voxel_downsample_ragged"] if thin else []) + (["resample_points_ragged"] if resample else []), opts
        out = E.infer_point_clouds(*pos, **k)
        assert len(reads) == 1, opts
        keys = {"pred", "cd", "n_queries", "denoised", "denoise_index", "denoise_labels", "planes", "num_planes"}
        at = 3 + (taus is not None)
        o = dev[1].tolist()
        per_frame = lambda t, oo: [t[oo[b]:oo[b + 1]] for b in range(B)]
        equal = lambda got, want: len(got) == len(want) and all(torch.equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
        if taus is not None:
            keys.add("metrics")
        nrm = None
        if normals:
            keys.add("normals")
            nrm = dev[at]
            at += 1
        d_pts, d_off, d_idx, d_cd = dev[at:at + 4]
        at += 4
        do = d_off.tolist()
        assert equal(out["denoised"], per_frame(d_pts, do)) and equal(out["denoise_index"], per_frame(d_idx, do)), opts
        if surf:
            keys.add("cd_denoised")
            assert same(out["cd_denoised"], d_cd), opts
        if taus is not None:
            keys.add("metrics_denoised")
            assert (out["metrics_denoised"] is None and dev[at] is None and not surf) or _metrics_match(out["metrics_denoised"], dev[at], B)
            at += 1
        if nrm is not None:
            keys.add("denoised_normals")
            assert equal(out["denoised_normals"], [nrm[o[b] + per_frame(d_idx, do)[b]] for b in range(B)]), opts
        labels, planes, num = dev[at:at + 3]
        at += 3
        assert equal(out["denoise_labels"], per_frame(labels, do)) and out["num_planes"] == num.tolist() == [2, 1], opts
        assert all(isinstance(v, int) for v in out["num_planes"]) and planes.dtype == torch.float64 and tuple(planes.shape) == (B, 2, 4)
        assert [len(f) for f in out["planes"]] == [2, 1] and all(out["planes"][b][j] == tuple(planes[b, j].tolist())
                                                                  for b in range(B) for j in range(out["num_planes"][b])), opts
        if thin is not None:
            keys |= {"thinned", "thin_count", "thin_first"} | ({"thinned_normals"} if normals else set())
            at += 4
        if resample is not None:
            keys |= {"resampled", "resample_index"}
            at += 2
        assert at == len(dev) and set(out) == keys, (opts, set(out) ^ keys)
        combos += 1
    assert combos == 32
    gen = torch.Generator().manual_seed(41)                               # the seed is the generator's, read on the host
    E.infer_point_clouds_device(*pos, **{**kw, "rng": gen, "remove_planes": (0.25, 128)})
    assert seen["args"][6] == 41 and seen["args"][3] == 1 and seen["args"][8] is False
    for other in (dict(denoise=(0.5, 2)), dict(denoise_statistical=(8, 2.0, 0.5)), dict(denoise_cluster=(0.5, 2, 30))):
        del calls[:], reads[:]
        with pytest.raises(ValueError, match="excludes"):
            E.infer_point_clouds(*pos, remove_planes=(0.25, 128), **other, **kw)
        assert not calls and not reads
    del calls[:]
    out = E.infer_point_clouds(*pos, **kw)                                # without the option nothing changes
    assert "remove_planes_ragged" not in calls and set(out) == {"pred", "cd", "n_queries"}
