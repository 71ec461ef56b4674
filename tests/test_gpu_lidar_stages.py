"""The LiDAR front end (rald_amd/csrc/lidar.hip, rald_amd/lidar.py) stage by stage and across its configuration space, against the
plain reference of tests/lidar_ref.py (shown right in tests/test_lidar_ref.py).

Each stage's reference consumes the DEVICE's output of the stage before (the polar rows, then the coords, kept keys and counts), so
a 1-ulp difference in a transcendental cannot leak into the integer stages: crop and polar are held to 1 ulp, everything behind
them to bit equality.  Frames have at most 4 099 points and num_samples is at most 512.

    crop       strides 3 / 4 / 6, frame lengths around the 256-point chunk, an empty frame inside a batch, rows planted on the
               inclusive FOV bounds with their float32 neighbours, zero / NaN / inf rows
    polar      axes, -0.0 components, the origin (NaN elevation), overflowing rows
    voxelize   grids of 255 .. 1290^3 cells (1, 2, 3 and 4 radix passes, the outside key in a digit of its own), frame lengths
               around the 64-element wave slices, one segment across every wave, both caps binding, F = 4 and 6, `counts`,
               points on cell faces
    queries    the four (anisotropic, isotropic) flag pairs on a cone and a Cartesian grid, in_num 0 / S/16 / S, the first and the
               last empty rank, key runs at both ends of the grid, offsets at +-v/2, out-of-range indices
    batch      the reference loader's dicts of g25_lidar_configs.npz, bit for bit
    drop-ins   remove_empty_points, transform_lidar_data, cartesian2polar, filter_points_polar against numpy
"""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

import lidar_ref as REF
from conftest import GOLDEN
from test_lidar import SHIPPED, _cfg
from test_lidar_ref import CONFIGS, config25

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _g25():
    with np.load(os.path.join(GOLDEN, "g25_lidar_configs.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _ordered(a) -> np.ndarray:
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulp(a, b) -> int:
    """largest distance in float32 steps; NaN only where the other side has NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    return int(np.abs(_ordered(a)[ok] - _ordered(b)[ok]).max()) if ok.any() else 0


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _pack(frames, cols=3):
    from rald_amd.lidar import _pack
    flat, offs, _ = _pack(frames, cols)
    return torch.from_numpy(flat).cuda(), offs


def _fov(cfg):
    return [[float(v) for v in row] for row in cfg.fov]


# ==================================================================================================== crop
def _scan(seed, n):
    from rald_amd import synth
    return synth.lidar_scan(1, seed, 4096)[0][:n]


def _check_crop(cfg, frames):
    """device crop of a batch against REF.crop per frame: the same kept set, rows within 1 ulp.  Returns the worst ulp."""
    from rald_amd.lidar import LidarFrames
    h = LidarFrames(cfg)
    x, offs = _pack(frames)
    out, counts = h.crop(x, offs)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    worst = 0
    for b, f in enumerate(frames):
        keep, rows, polar = REF.crop(f, cfg.extrinsic, _fov(cfg))
        assert (REF.bound_distance(polar, _fov(cfg)) >= 1e-9).all(), "a point within 1e-9 of a FOV bound: choose another seed"
        assert counts[b] == keep.sum() == len(rows), f"frame {b}: {counts[b]} kept, the reference keeps {len(rows)}"
        worst = max(worst, _ulp(out[offs[b]:offs[b] + counts[b]], rows))
    assert worst <= 1, f"cropped rows differ by {worst} ulp"
    return worst


@pytest.mark.parametrize("stride", [3, 4, 6])
def test_crop_random_scans_at_strides(stride):
    """[N, 3], raw [N, 4] and [N, 6] rows; the columns past z are never read as coordinates (NaN there changes nothing)"""
    frames = []
    for seed in (2601, 2602):
        s = _scan(seed, 4096)
        extra = np.full((len(s), max(stride - 3, 0)), np.nan, dtype=np.float32)
        frames.append(np.ascontiguousarray(np.concatenate([s[:, :3], extra], axis=1)))
    assert frames[0].shape[1] == stride
    worst = _check_crop(_cfg(), frames)
    print(f"crop stride {stride}: worst {worst} ulp")


@pytest.mark.parametrize("lengths", [[0], [1], [255], [256], [257], [4096], [300, 0, 257], [0, 0], [1, 0, 4096, 0]],
                         ids=lambda v: "-".join(str(n) for n in v))
def test_crop_frame_lengths(lengths):
    """around the 256-point chunk; a frame of no points alone, in the middle and at the end of a batch"""
    frames = [_scan(2610 + i, 4096)[4096 - n:] for i, n in enumerate(lengths)]
    worst = _check_crop(_cfg(), frames)
    print(f"crop lengths {lengths}: worst {worst} ulp")


def _planted_cfg(fov):
    cfg = _cfg()
    cfg.extrinsic = np.eye(4)
    cfg.fov = fov
    return cfg


def test_crop_inclusive_bounds_planted():
    """Rows whose float64 polar lies exactly on a bound (exact in any libm: sqrt(25), atan2(-2, 0), asin(1), atan2(0, -3), asin(0)),
    each with a float32 neighbour inside and, where the geometry has one, outside.  On the bound and inside are kept, outside is
    dropped.  Elevation cannot exceed 90 degrees, so the el = 90 row has no outside neighbour; the el = 0 bound of the second
    handle has both."""
    from rald_amd.lidar import LidarFrames
    f32 = np.float32
    up, down = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
    e2, e3, tiny = np.spacing(f32(2)), np.spacing(f32(3)), np.nextafter(f32(0), f32(1))
    fov_a = [[0, 5], [-180, 90], [-90, 90]]
    rows_a = [  # (x, y, z), kept
        ((5, 0, 0), True), ((down(5), 0, 0), True), ((up(5), 0, 0), False),                       # r = max_range
        ((0, 0, 5), True), ((0, 0, up(5)), False), ((0, down(-5), 0), False), ((0, -5, 0), True),
        ((0, -2, 0), True), ((e2, -2, 0), True), ((-e2, -2, 0), False), ((-tiny, -2, 0), True),   # az = 90; -tiny rounds onto it
        ((-0.0, -2, 0), True),
        ((0, 0, 2), True), ((e2, 0, 2), True), ((0, -e2, 2), True),                               # el = 90
        ((0, 0, -2), True), ((e2, 0, -2), True),                                                  # el = -90
        ((-3, 0, 0), True), ((-3, e3, 0), True), ((-3, tiny, 0), True),                           # az = -180
        ((-3, -tiny, 0), False), ((-3, -e3, 0), False),                                           # atan2(-y, -3) -> -pi: az = +180
        ((-3, -0.0, 0), True),                                               # the transform's sum turns -0.0 into +0.0: az = -180
        ((0, 2, 0), True), ((-e2, 2, 0), True),                                                   # az = -90, inside
    ]
    fov_b = [[0, 5], [-90, 0], [-20, 0]]
    rows_b = [
        ((3, 0, 0), True), ((3, 0, -tiny), True), ((3, 0, tiny), False), ((3, 0, -0.0), True),    # el = 0 = el_range[1]
        ((3, 0, -e3), True), ((3, 0, e3), False),
        ((3, tiny, 0), True), ((3, -tiny, 0), False), ((3, -0.0, 0), True), ((3, e3, 0), True),   # az = 0 = az_range[1]
        ((3, -e3, 0), False),
    ]
    for fov, planted in ((fov_a, rows_a), (fov_b, rows_b)):
        cfg = _planted_cfg(fov)
        pts = np.array([p for p, _ in planted], dtype=np.float32)
        want = np.array([k for _, k in planted])
        keep, rows, polar = REF.crop(pts, cfg.extrinsic, fov)
        assert np.array_equal(keep, want), f"the reference itself: {np.nonzero(keep != want)[0]}"
        assert (want & (REF.bound_distance(polar, fov) == 0)).sum() >= 6     # kept rows that lie exactly on a bound
        h = LidarFrames(cfg)
        # the same rows alone, and spread over a 700-row frame of dropped rows so that they sit in different chunks and waves
        filler = np.tile(np.array([[9, 0, 0]], dtype=np.float32), (700, 1))
        spread = filler.copy()
        at = np.arange(len(pts)) * 23 + 5
        spread[at] = pts
        for frame, k in ((pts, keep), (spread, None)):
            x, offs = _pack([frame, frame[::-1].copy()])
            out, counts = h.crop(x, offs)
            out, counts = out.cpu().numpy(), counts.cpu().numpy()
            for b, f in enumerate((frame, frame[::-1])):
                rk, rrows, _ = REF.crop(f, cfg.extrinsic, fov)
                if k is not None and b == 0:
                    assert np.array_equal(rk, k)
                assert counts[b] == rk.sum(), f"fov {fov}: {counts[b]} kept, {rk.sum()} expected"
                got = out[offs[b]:offs[b] + counts[b]]
                assert _ulp(got, rrows) <= 1
                # which rows survived: the planted rows are distinct, so match them through the reference's rows
                assert len(got) == len(rrows)


def test_crop_drops_zero_nan_and_inf_rows():
    """remove_empty_points on the float32 sum of squares (NaN > 0 is False, a square that underflows to 0 is empty, a denormal
    square is not), inf rows fail the range test; the survivors around them keep their order and the counts stay right"""
    from rald_amd.lidar import LidarFrames
    cfg = _planted_cfg([[0, 40], [-180, 180], [-90, 90]])
    nan, inf = np.nan, np.inf
    good = _scan(2630, 600)[:, :3].copy()
    good = good[(good * good).sum(axis=1) > 0][:300]
    bad = np.array([[0, 0, 0], [-0.0, 0.0, -0.0], [nan, 1, 1], [1, nan, 1], [1, 1, nan], [nan, nan, nan], [inf, 0, 0], [0, -inf, 1],
                    [inf, inf, inf], [-inf, 1, nan], [1e-23, 1e-23, 0], [3e38, 3e38, 0]], dtype=np.float32)
    small = np.array([[1e-20, 0, 0], [0, -1e-20, 1e-21]], dtype=np.float32)       # squares are float32 denormals: not empty, kept
    frame = good.copy()
    pos = np.arange(len(bad)) * 19 + 3
    frame = np.insert(frame, pos, bad, axis=0)
    frame = np.concatenate([bad[:3], frame, small, bad[-3:]], axis=0).astype(np.float32)
    keep, rows, _ = REF.crop(frame, cfg.extrinsic, _fov(cfg))
    assert keep.sum() == len(good) + len(small)                                  # the reference keeps exactly the finite rows
    h = LidarFrames(cfg)
    x, offs = _pack([frame, bad, frame[::-1].copy()])
    out, counts = h.crop(x, offs)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    assert counts.tolist() == [len(rows), 0, len(rows)]
    assert _ulp(out[:counts[0]], rows) <= 1
    assert _ulp(out[offs[2]:offs[2] + counts[2]], rows[::-1]) <= 1
    assert np.isfinite(out[:counts[0]]).all()


# ==================================================================================================== polar
def test_polar_edges_and_random_rows():
    from rald_amd.lidar import LidarFrames
    inf = np.inf
    edge = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, -0.0, 0], [-1, -0.0, 0], [-1, 0, -0.0],
                     [-0.0, 1, 0], [-0.0, -1, -0.0], [1, 1, -0.0], [0, 0, 0], [-0.0, -0.0, -0.0], [0, -0.0, 0], [-0.0, 0, 0],
                     [3, 4, 0], [1e-30, 0, 0], [0, 1e-30, 1e-30], [1e-20, -1e-20, 1e-20], [2e19, 0, 0], [1e30, 1e30, 0], [0, 0, 1e30],
                     [inf, 0, 0], [inf, inf, 0], [1, 1, inf], [np.nan, 1, 1], [1, np.nan, 0]], dtype=np.float32)
    rows = _g25()["crop_b0"]
    h = LidarFrames(_cfg())
    frames = [edge, rows, np.concatenate([rows[:100], edge, rows[100:163]])]
    x, offs = _pack(frames)
    pol = h.voxelize(x, offs, to_polar=True, with_voxels=False)["polar"].cpu().numpy()
    worst, differ = 0, 0
    for b, f in enumerate(frames):
        got, want = pol[offs[b]:offs[b + 1]], REF.polar_f32(f)
        worst = max(worst, _ulp(got, want))                                      # also: NaN in the same places
        zero = want == 0
        assert np.array_equal(np.signbit(got[zero]), np.signbit(want[zero]))
        assert np.array_equal(np.isinf(got), np.isinf(want))
        differ += int(((_bits(got) != _bits(want)) & ~np.isnan(want)).any(axis=1).sum())     # a NaN's sign and payload are free
    assert np.isnan(REF.polar_f32(edge)[12:16, 2]).all() and not np.isnan(REF.polar_f32(edge)[12:16, :2]).any()   # the origin rows
    print(f"polar: worst {worst} ulp, {differ} rows differ from the correctly rounded value")
    assert worst <= 1
    # The device rounds a double atan2 / asin once and multiplies in float32, as polar_f32 does.  The two can only differ where the
    # two double libraries' results fall on either side of a float32 rounding boundary: a double within one of its own ulps of the
    # boundary, 2^-28 of all values.  Among the 6 100 values here that is 2e-5 rows; more than 2 mean another formula.
    assert differ <= 2


# ==================================================================================================== voxelize
def _cart(grid, v=(0.5, 0.25, 2.0), lo=(-3.0, 2.0, 0.5), **over):
    """a Cartesian config of `grid` cells per axis; lo and v are binary fractions, so every face is an exact float32"""
    hi = [lo[k] + grid[k] * v[k] for k in range(3)]
    over.setdefault("max_number_of_voxels", 5000)
    return _cfg(view_cone_mode=False, pc_range=[*lo, *hi], voxel_size=list(v), **over)


def _cloud(rng, cfg, n, ncells=None, outside=0.25):
    """n float32 points in `ncells` random cells (the first and the last cell of the grid among them, several points per cell) and a
    share outside the grid on either side"""
    grid = REF.grid_of(cfg.pc_range, cfg.voxel_size)
    lo, v = np.array(cfg.pc_range[:3], dtype=np.float64), np.array(cfg.voxel_size, dtype=np.float64)
    ncells = ncells or max(2, n // 3)
    cells = np.stack([rng.integers(0, g, ncells) for g in grid], axis=1)
    cells[0], cells[-1] = 0, grid - 1
    pick = rng.integers(0, ncells, n)
    pick[:2] = [0, ncells - 1][:len(pick[:2])]
    p = lo + (cells[pick] + rng.uniform(0.1, 0.9, (n, 3))) * v
    out = rng.random(n) < outside
    out[:2] = False
    k = int(out.sum())
    side = rng.random((k, 3)) < 0.5
    p[out] = np.where(side, lo - rng.uniform(0.1, 2, (k, 3)) * v, lo + (grid + rng.uniform(0.1, 2, (k, 3))) * v)
    return p.astype(np.float32)


def _check_vox(cfg, frames, counts=None, to_polar=False):
    """voxelize on the device against REF.point_to_voxel per frame, bit for bit.  In view-cone mode the reference reads the device's
    polar rows.  Returns (handle, [(voxels, coords, num_points)] of the reference)."""
    from rald_amd.lidar import LidarFrames
    h = LidarFrames(cfg)
    grid = REF.grid_of(cfg.pc_range, cfg.voxel_size)
    assert grid.tolist() == h.grid.tolist() and int(np.prod(grid)) == h.cells
    x, offs = _pack(frames, h.F)
    ct = None if counts is None else torch.tensor(counts, dtype=torch.int32).cuda()
    res = h.voxelize(x, offs, ct, to_polar=to_polar)
    out = {k: t.cpu().numpy() for k, t in res.items() if t is not None}
    refs = []
    for b, f in enumerate(frames):
        n = len(f) if counts is None else min(max(int(counts[b]), 0), len(f))
        src = out["polar"][offs[b]:offs[b] + n] if to_polar else np.asarray(f, dtype=np.float32)[:n]
        v, c, num = REF.point_to_voxel(src, cfg.voxel_size, cfg.pc_range, h.F, h.maxp, h.maxv)
        V = len(c)
        assert out["voxel_counts"][b] == V, f"frame {b}: {out['voxel_counts'][b]} voxels, the reference has {V}"
        assert np.array_equal(out["coords"][b, :V], c), f"frame {b}: coords"
        assert np.array_equal(out["num_points"][b, :V], num), f"frame {b}: num_points"
        assert np.array_equal(_bits(out["voxels"][b, :V]), _bits(v)), f"frame {b}: voxels"
        assert np.array_equal(out["kept_keys"][b, :V].astype(np.int64), np.sort(REF.linear_keys(c, grid))), f"frame {b}: kept_keys"
        refs.append((v, c, num))
    return h, refs


# name: (config, radix passes of its keys, view-cone mode)
def _grid_cases():
    return {
        "c255":     (_cart((15, 17, 1)), 1, False),
        "c256":     (_cart((16, 16, 1)), 2, False),                  # the outside key 256 alone has a second digit
        "c65535":   (_cart((255, 257, 1)), 2, False),
        "c65536":   (_cart((256, 256, 1)), 3, False),                # the outside key alone has a third digit
        "c2p24m1":  (_cart((4095, 4097, 1)), 3, False),
        "c2p24":    (_cart((256, 256, 256)), 4, False),              # the outside key alone has a fourth digit
        "cart36M":  (_cfg(view_cone_mode=False, pc_range=[0, -15, -5, 15, 15, 5], voxel_size=[0.05, 0.05, 0.05],
                          max_number_of_voxels=5000), 4, False),
        "cone":     (_cfg(max_number_of_voxels=5000), 4, True),      # the shipped view cone, 316 x 720 x 80
        "c1290":    (_cfg(view_cone_mode=False, pc_range=[0, -6.45, -6.45, 12.9, 6.45, 6.45], voxel_size=[0.01, 0.01, 0.01],
                          max_number_of_voxels=5000), 4, False),     # 1290^3 = 2 146 689 000 cells, 99.96 % of 2^31
    }


GRID_NAMES = ["c255", "c256", "c65535", "c65536", "c2p24m1", "c2p24", "cart36M", "cone", "c1290"]


@pytest.mark.parametrize("name", GRID_NAMES)
def test_voxelize_grids(name):
    cases = _grid_cases()
    assert list(cases) == GRID_NAMES and {p for _, p, _ in cases.values()} == {1, 2, 3, 4}      # no pass class silently dropped
    cfg, npass, cone = cases[name]
    from rald_amd.lidar import LidarFrames
    h = LidarFrames(cfg)
    assert REF.passes(h.cells) == npass, f"{name}: {h.cells} cells need {REF.passes(h.cells)} passes"
    rng = np.random.default_rng(2700 + GRID_NAMES.index(name))
    if cone:
        frames = [_g25()["crop_b0"], _g25()["crop_b1"][:777]]
    else:
        frames = [_cloud(rng, cfg, 1500), _cloud(rng, cfg, 777, ncells=40)]
    _, refs = _check_vox(cfg, frames, to_polar=cone)
    for v, c, num in refs:
        assert len(c) > 30 and num.max() > 1
    if not cone:
        keys = REF.linear_keys(refs[0][1], h.grid)
        assert keys.min() == 0 and keys.max() == h.cells - 1                        # cell 0 and the last cell are occupied
        if name == "c1290":
            assert h.cells == 1290 ** 3 and keys.max() >= 1 << 30 and ((keys >> 24) > 0).sum() > 100


LENGTHS = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4099]


@pytest.mark.parametrize("name", ["c255", "c256", "c65536", "c2p24"])
def test_voxelize_frame_lengths(name):
    """one batch of every length around the 64-element slices of the 16 waves (0 and 1 skip the sort), per pass class 1 .. 4"""
    cfg, npass, _ = _grid_cases()[name]
    assert npass == {"c255": 1, "c256": 2, "c65536": 3, "c2p24": 4}[name]
    rng = np.random.default_rng(2800 + npass)
    frames = [_cloud(rng, cfg, n, ncells=max(2, n // 8)) if n else np.zeros((0, 3), np.float32) for n in LENGTHS]
    frames[1] = frames[4][:1].copy()                                              # the 1-point frame holds a point inside the grid
    _, refs = _check_vox(cfg, frames)
    assert [len(c) for _, c, _ in refs][:3] == [0, 1, 2]
    # and each frame alone: the buffer the sorted pairs end in depends on the pass count and on n > 1
    for b in (1, 2, 5, 8):
        _check_vox(cfg, [frames[b]])


@pytest.mark.parametrize("pattern", ["one_cell_maxp5", "one_cell_maxp_n", "distinct", "all_outside", "half_outside"])
def test_voxelize_key_patterns(pattern):
    n = 3000
    rng = np.random.default_rng(2900)
    if pattern.startswith("one_cell"):                                            # one segment that spans every wave's slice
        maxp = 5 if pattern.endswith("5") else n + 8
        cfg = _cart((16, 16, 1), max_points_per_voxel=maxp, max_number_of_voxels=4)
        p = (np.array([-3.0, 2.0, 0.5]) + (np.array([7, 11, 0]) + rng.uniform(0.05, 0.95, (n, 3))) * [0.5, 0.25, 2.0]).astype(np.float32)
        _, refs = _check_vox(cfg, [p, p[:1500]])
        assert [r[2].tolist() for r in refs] == [[min(n, maxp)], [min(1500, maxp)]]
        return
    cfg = _cart((256, 256, 1), max_points_per_voxel=3)
    lo, v = np.array(cfg.pc_range[:3]), np.array(cfg.voxel_size)
    cells = rng.permutation(65536)[:n]
    c = np.stack([cells // 256, cells % 256, np.zeros(n, dtype=np.int64)], axis=1)
    p = lo + (c + rng.uniform(0.1, 0.9, (n, 3))) * v
    if pattern == "all_outside":
        p[:, 0] += 256 * v[0] * np.where(rng.random(n) < 0.5, 1, -1)
    elif pattern == "half_outside":
        p[::2, 1] -= 256 * v[1]
    _, refs = _check_vox(cfg, [p.astype(np.float32)])
    assert len(refs[0][1]) == {"distinct": n, "all_outside": 0, "half_outside": n // 2}[pattern]


def test_voxelize_caps_bind():
    """max_voxels of 1, of exactly the occupied cells, and of one fewer; max_points of 1 and 2 with up to ~10 points per cell"""
    rng = np.random.default_rng(3000)
    base = _cart((16, 16, 4))
    frames = [_cloud(rng, base, 2049, ncells=300), _cloud(rng, base, 500, ncells=300)]
    full = [len(REF.point_to_voxel(f, base.voxel_size, base.pc_range, 3, 1, 10 ** 6)[1]) for f in frames]
    assert min(full) > 100
    for maxv in (1, full[0], full[0] - 1, full[1]):
        for maxp in (1, 2, 10):
            _, refs = _check_vox(_cart((16, 16, 4), max_number_of_voxels=maxv, max_points_per_voxel=maxp), frames)
            assert [len(c) for _, c, _ in refs] == [min(maxv, f) for f in full]


@pytest.mark.parametrize("F", [4, 6])
def test_voxelize_point_features(F):
    """columns past z travel into the voxel tensor at their own stride; each column holds values no other column has"""
    rng = np.random.default_rng(3100 + F)
    cfg = _cart((16, 16, 4), num_point_features=F, max_points_per_voxel=4)
    frames = []
    for n in (1025, 300):
        xyz = _cloud(rng, cfg, n, ncells=200)
        extra = (np.arange(n)[:, None] + 10000.0 * np.arange(1, F - 2)[None, :]).astype(np.float32)
        frames.append(np.ascontiguousarray(np.concatenate([xyz, extra], axis=1)))
    _, refs = _check_vox(cfg, frames)
    v = refs[0][0]
    assert v.shape[2] == F and all((v[..., k][v[..., k] != 0] >= 10000.0 * (k - 2)).all() for k in range(3, F))


def test_voxelize_counts_shorter_zero_and_clamped():
    rng = np.random.default_rng(3200)
    cfg = _cart((16, 16, 4))
    frames = [_cloud(rng, cfg, n, ncells=100) for n in (1025, 700, 64, 300, 513)]
    _, refs = _check_vox(cfg, frames, counts=[1000, 0, 65, 1 << 30, -3])
    assert [len(c) > 0 for _, c, _ in refs] == [True, False, True, True, False]
    _check_vox(cfg, frames, counts=[1, 700, 63, 2, 512])


@pytest.mark.parametrize("grid", ["binary", "shipped_sizes"])
def test_voxelize_points_on_cell_faces(grid):
    """every face along each axis and the float32 just below it, -0.0, NaN and inf rows.  binary: faces are exact float32 values, so
    a face belongs to the cell above it and the grid's upper face is outside; shipped_sizes: 0.05 / 0.25 / 0.5 steps, where the
    float32 quotient decides (the reference's and the device's must be the same)."""
    if grid == "binary":
        cfg = _cart((12, 9, 5), max_points_per_voxel=4)
    else:
        cfg = _cfg(view_cone_mode=False, max_number_of_voxels=5000, max_points_per_voxel=4)
    g = REF.grid_of(cfg.pc_range, cfg.voxel_size)
    lo, hi, v = np.array(cfg.pc_range[:3]), np.array(cfg.pc_range[3:]), np.array(cfg.voxel_size)
    mid = (lo + (g // 2 + 0.5) * v).astype(np.float32)
    rows = []
    for k in range(3):
        step = max(1, g[k] // 160)
        face = (lo[k] + np.arange(0, g[k] + 1, step) * v[k]).astype(np.float32)
        face = np.concatenate([face, [np.float32(hi[k])]])
        for vals in (face, np.nextafter(face, np.float32(-np.inf)), np.nextafter(face, np.float32(np.inf))):
            r = np.tile(mid, (len(vals), 1))
            r[:, k] = vals
            rows.append(r)
    nan, inf = np.nan, np.inf
    special = np.array([[-0.0, mid[1], mid[2]], [mid[0], -0.0, mid[2]], [mid[0], mid[1], -0.0], [0.0, 0.0, 0.0], [nan, mid[1], mid[2]],
                        [mid[0], nan, mid[2]], [mid[0], mid[1], nan], [inf, mid[1], mid[2]], [mid[0], -inf, mid[2]], [mid[0], mid[1], inf],
                        [nan, nan, nan], [-inf, -inf, -inf], [3e38, mid[1], mid[2]], [mid[0], -3e38, mid[2]]], dtype=np.float32)
    frame = np.concatenate(rows + [special], axis=0).astype(np.float32)
    assert len(frame) <= 4099
    _, refs = _check_vox(cfg, [frame, frame[::-1].copy()])
    if grid == "binary":
        c, inside = REF.cell_index(frame, cfg.voxel_size, cfg.pc_range)
        finite = np.isfinite(frame).all(axis=1)
        for k in range(3):
            upper = (frame[:, k] == np.float32(hi[k])) & finite
            assert upper.any() and not inside[upper].any()                         # the upper face of the grid is outside
            lower = (frame[:, k] == np.float32(lo[k])) & finite
            assert lower.any() and inside[lower].all() and (c[lower, k] == 0).all()   # the lower face is cell 0
            below = (frame[:, k] == np.nextafter(np.float32(lo[k]), np.float32(-np.inf))) & finite
            assert below.any() and not inside[below].any()
        assert not inside[-len(special) + 4:].any()                                # NaN / inf rows are outside


# ==================================================================================================== queries
def _query_grids():
    # a cone-shaped range (the shipped pc_range at 4 x the voxel sizes) and the Cartesian grid of g25_lidar_configs.npz; both are
    # small enough for the dense occupancy grid of REF.empty_cells
    return {"cone": dict(view_cone_mode=True, voxel_size=[0.2, 1.0, 2.0]),
            "cart": dict(view_cone_mode=False, pc_range=[0, -8, -2, 16, 8, 2], voxel_size=[0.25, 0.25, 0.125]),
            # 40 x 20 x 12 cells whose bounds and sizes are no binary fractions: float32(v / 2 + lo) is not float32(v / 2) +
            # float32(lo) on any axis (0.175 / -6.95 / -1.55 against 0.17500001 / -6.9500003 / -1.5500001)
            "offgrid": dict(view_cone_mode=False, pc_range=[0.1, -7.3, -1.7, 6.1, 6.7, 1.9], voxel_size=[0.15, 0.7, 0.3])}


def _device_voxels_of_keys(h, cfg, key_lists, rng):
    """voxelize one point per listed cell (cell centres, shuffled): the device's coords / kept_keys / voxel_counts for the queries"""
    grid = tuple(int(g) for g in h.grid)
    lo, v = np.array(cfg.pc_range[:3]), np.array(cfg.voxel_size)
    frames = []
    for keys in key_lists:
        c = np.stack(np.unravel_index(rng.permutation(np.asarray(keys, dtype=np.int64)), grid), axis=1)
        frames.append((lo + (c + 0.5) * v).astype(np.float32))
    x, offs = _pack(frames)
    vox = h.voxelize(x, offs, with_voxels=False)
    for b, keys in enumerate(key_lists):
        assert int(vox["voxel_counts"][b]) == len(keys)
        assert np.array_equal(vox["kept_keys"][b, :len(keys)].cpu().numpy(), np.sort(keys))
    return vox


def _draw_queries(rng, cfg, G, N, V, S, in_num):
    """per frame: sample indices, voxel indices, ranks and offsets, with the edges planted (first / last voxel and rank, +-v/2)"""
    B, out_num = len(N), S - in_num
    half = np.array(cfg.voxel_size, dtype=np.float64) / 2
    d = dict(sidx=np.stack([rng.integers(0, n, S) for n in N]))
    d["sidx"][:, 0], d["sidx"][:, 1] = 0, np.array(N) - 1
    d["u_in"] = rng.uniform(-half, half, (B, in_num, 3))
    d["vidx"] = np.stack([rng.integers(0, v, in_num) for v in V]).reshape(B, in_num)
    d["u_out"] = rng.uniform(-half, half, (B, out_num, 3))
    d["erank"] = np.stack([rng.integers(0, G - v, out_num) for v in V]).reshape(B, out_num)
    if in_num >= 4:
        d["vidx"][:, 0], d["vidx"][:, 1] = 0, np.array(V) - 1
        d["u_in"][:, 0], d["u_in"][:, 1], d["u_in"][:, 2] = -half, half, half * [1, -1, 1]
    if out_num >= 4:
        d["erank"][:, 0], d["erank"][:, 1] = 0, G - np.array(V) - 1
        d["u_out"][:, 0], d["u_out"][:, 1], d["u_out"][:, 2] = half, -half, half * [-1, 1, -1]
    return d


def _run_queries(h, x, offs, S, in_num, d, vox):
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda() if a.shape[1] else None
    lp, qp, lab = h.queries(x, offs, S, in_num, up(d["sidx"], torch.int64), up(d["u_in"], torch.float64), up(d["vidx"], torch.int64),
                            up(d["u_out"], torch.float64), up(d["erank"], torch.int64), vox)
    return lp.cpu().numpy(), qp.cpu().numpy(), lab.cpu().numpy()


def _ref_queries(cfg, h, frames, vox, d, in_num):
    out = []
    for b, f in enumerate(frames):
        V = int(vox["voxel_counts"][b])
        coords = vox["coords"][b, :V].cpu().numpy()
        empty = REF.empty_cells(coords[:, ::-1], h.grid, d["erank"][b]) if d["erank"].shape[1] else None
        out.append(REF.queries(f, d["sidx"][b], coords, d["vidx"][b], d["u_in"][b], empty, d["u_out"][b], cfg.voxel_size, cfg.pc_range,
                               bool(cfg.norm_anisotropy), bool(cfg.norm_isotropy)))
    return out


def _query_setup(grid, aniso, iso, seed):
    from rald_amd.lidar import LidarFrames
    cfg = _cfg(norm_anisotropy=aniso, norm_isotropy=iso, max_number_of_voxels=2000, num_samples=512, **_query_grids()[grid])
    h = LidarFrames(cfg)
    G = h.cells
    assert G < 1 << 24
    rng = np.random.default_rng(seed)
    scattered = np.unique(rng.integers(1, G - 1, 900))
    key_lists = [np.arange(0, 700),                                                # a run 0 .. k: rank 0 is cell k + 1
                 np.unique(np.concatenate([scattered, np.arange(G - 300, G)])),    # a run ending at G - 1: the last rank lies before it
                 np.array([G // 3]),                                               # a single key
                 np.unique(np.concatenate([[0, G - 1], scattered]))]               # both corner cells and scattered ones
    vox = _device_voxels_of_keys(h, cfg, key_lists, rng)
    lo, hi = np.array(cfg.pc_range[:3]), np.array(cfg.pc_range[3:])
    frames = [rng.uniform(lo, hi, (n, 3)).astype(np.float32) for n in (700, 513, 1, 1025)]
    frames[0][:3] = [lo, hi, (lo + hi) / 2]                                        # normalise to -1, 1 and 0
    return cfg, h, frames, vox, [len(k) for k in key_lists], rng


@pytest.mark.parametrize("iso", [False, True], ids=["", "iso"])
@pytest.mark.parametrize("aniso", [False, True], ids=["", "aniso"])
@pytest.mark.parametrize("grid", ["cone", "cart", "offgrid"])
def test_queries_bit_identical(grid, aniso, iso):
    S = 512
    cfg, h, frames, vox, V, rng = _query_setup(grid, aniso, iso, 3300)
    x, offs = _pack(frames)
    for in_num in (0, S // 16, S):
        d = _draw_queries(rng, cfg, h.cells, [len(f) for f in frames], V, S, in_num)
        lp, qp, lab = _run_queries(h, x, offs, S, in_num, d, vox)
        for b, (rlp, rqp, rlab) in enumerate(_ref_queries(cfg, h, frames, vox, d, in_num)):
            where = f"{grid} aniso={aniso} iso={iso} in_num={in_num} frame {b}"
            assert np.array_equal(_bits(lp[b]), _bits(rlp)), f"{where}: lidar_points"
            bad = np.nonzero((_bits(qp[b]) != _bits(rqp)).any(axis=1))[0]
            assert len(bad) == 0, f"{where}: query_points rows {bad[:8]}: {qp[b][bad[:2]]} for {rqp[bad[:2]]}"
            assert np.array_equal(lab[b], rlab) and lab[b, :in_num].all() and not lab[b, in_num:].any(), f"{where}: labels"
            assert np.isfinite(qp[b]).all()


def test_queries_out_of_range_indices_give_nan_rows():
    """sample_idx, voxel_idx and empty_rank of -1 and of N / V / G - V: NaN rows there, every other row and every label unchanged"""
    S, in_num = 512, 32
    cfg, h, frames, vox, V, rng = _query_setup("cart", True, True, 3400)
    x, offs = _pack(frames)
    N = [len(f) for f in frames]
    d = _draw_queries(rng, cfg, h.cells, N, V, S, in_num)
    good = _run_queries(h, x, offs, S, in_num, d, vox)
    bad = {k: a.copy() for k, a in d.items()}
    for b in range(len(frames)):
        bad["sidx"][b, 5], bad["sidx"][b, 6], bad["sidx"][b, 500] = -1, N[b], 1 << 40
        bad["vidx"][b, 3], bad["vidx"][b, 4] = -1, V[b]
        bad["erank"][b, 7], bad["erank"][b, 8], bad["erank"][b, 9] = -1, h.cells - V[b], 1 << 40
    lp, qp, lab = _run_queries(h, x, offs, S, in_num, bad, vox)
    lp_nan, qp_nan = np.zeros((len(frames), S), bool), np.zeros((len(frames), S), bool)
    lp_nan[:, [5, 6, 500]] = True
    qp_nan[:, [3, 4, in_num + 7, in_num + 8, in_num + 9]] = True
    assert np.array_equal(np.isnan(lp).all(axis=2), lp_nan) and np.array_equal(np.isnan(lp).any(axis=2), lp_nan)
    assert np.array_equal(np.isnan(qp).all(axis=2), qp_nan) and np.array_equal(np.isnan(qp).any(axis=2), qp_nan)
    assert np.array_equal(_bits(lp[~lp_nan]), _bits(good[0][~lp_nan])) and np.array_equal(_bits(qp[~qp_nan]), _bits(good[1][~qp_nan]))
    assert np.array_equal(lab, good[2]) and lab[:, :in_num].all() and not lab[:, in_num:].any()


# ==================================================================================================== batch
def _sha(a) -> np.ndarray:
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


@pytest.mark.parametrize("loader", ["train", "test"])
@pytest.mark.parametrize("tag", list(CONFIGS))
def test_batch_replays_reference_configs(tag, loader):
    """the reference loader's own dicts away from the shipped flags (g25_lidar_configs.npz), from numpy's float32 polar rows (cone
    tags) or the cartesian rows (cart tags): every value bit-identical"""
    from rald_amd.lidar import LidarFrames
    g25 = _g25()
    cfg = _cfg(**{k: v for k, v in config25(tag).items() if k not in SHIPPED or SHIPPED[k] != v})
    h = LidarFrames(cfg)
    B = int(g25["meta"][1])
    frames = [g25[f"polar_b{b}" if cfg.view_cone_mode else f"crop_b{b}"] for b in range(B)]
    torch.manual_seed(int(g25["seeds"][1]))
    d = h.batch(frames, loader, rng=np.random.default_rng(int(g25["seeds"][0])), polar=True)
    assert ("raw_lidar_points" in d) == (loader != "train")
    for b in range(B):
        key = f"ds_{tag}_{loader}_b{b}"
        if key + "_lidar_points" in g25:
            for name in ("lidar_points", "query_points", "query_labels"):
                got, want = d[name][b].cpu().numpy(), g25[f"{key}_{name}"]
                bad = np.nonzero((_bits(got) != _bits(want)).reshape(len(want), -1).any(axis=1))[0]
                assert len(bad) == 0, f"{key}: {name} rows {bad[:8]}: {got[bad[:2]]} for {want[bad[:2]]}"
        for name, want in zip(("lidar_points", "query_points", "query_labels"), g25[key + "_sha"]):
            assert np.array_equal(_sha(d[name][b]), want), f"{key}: {name} differ"
        assert int(d["in_voxel_num"][b]) == int(g25[key + "_in"])


def test_batch_raises_on_a_fully_occupied_grid():
    """'train' draws ranks with randint(0, G - V): on a grid without an empty cell the reference raises, and so does batch"""
    from rald_amd.lidar import LidarFrames
    cfg = _cfg(view_cone_mode=False, pc_range=[0, 0, 0, 2, 2, 1], voxel_size=[1, 1, 1], num_samples=8)
    pts = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 0.5]] * 3, dtype=np.float32)
    h = LidarFrames(cfg)
    with pytest.raises(RuntimeError):
        torch.randint(0, 0, (4,))
    with pytest.raises(RuntimeError):
        h.batch([pts], "train", rng=np.random.default_rng(0), polar=True)
    d = h.batch([pts], "test", rng=np.random.default_rng(0), polar=True)           # no out-of-voxel queries: nothing to draw
    assert d["query_labels"].eq(1).all() and d["query_points"].shape == (1, 8, 3)
    three = pts[np.arange(len(pts)) % 4 != 3]                                      # one cell empty: rank 0 is the only draw
    d = h.batch([three], "train", rng=np.random.default_rng(0), polar=True)
    assert torch.equal(d["query_labels"][0].cpu(), torch.zeros(8)) and torch.isfinite(d["query_points"]).all()


# ==================================================================================================== drop-ins
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dropin_remove_empty_points(dtype):
    from rald_amd.lidar import remove_empty_points
    rng = np.random.default_rng(3500)
    p = rng.uniform(-20, 20, (400, 4)).astype(dtype)
    p[::7, :3] = 0                                                                 # the 4th column does not make a row non-empty
    p[3, :3], p[10, :3], p[11, :3] = [-0.0, 0.0, -0.0], [1e-23, 0, 0], [0, 1e-20, 0]
    p[12, :3], p[13, :3] = [np.nan, 0, 0], [np.inf, 0, 0]
    with np.errstate(all="ignore"):
        want = p[np.linalg.norm(p[:, :3], axis=1) > 0]
    got = remove_empty_points(p)
    assert got.dtype == torch.from_numpy(p).dtype and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.int32 if dtype == np.float32 else np.int64), want.view(got.cpu().numpy().view(
        np.int32 if dtype == np.float32 else np.int64).dtype))
    assert 400 - 58 - 3 <= len(want) < 400


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dropin_filter_points_polar(dtype):
    """inclusive bounds hit exactly: in float32 the bound itself is compared as a float32, as numpy compares it"""
    from rald_amd.lidar import filter_points_polar
    rng = np.random.default_rng(3600)
    limits = [[0.1, 15.863025538680999], [-89.9, 90], [-20.3, 20]]
    p = np.stack([rng.uniform(0, 17, 600), rng.uniform(-95, 95, 600), rng.uniform(-22, 22, 600)], axis=1).astype(dtype)
    mid = np.array([5.0, 1.0, 1.0], dtype=dtype)
    planted = []
    for k in range(3):
        for bound in limits[k]:
            b = dtype(bound)
            for val in (b, np.nextafter(b, dtype(-np.inf)), np.nextafter(b, dtype(np.inf))):
                r = mid.copy()
                r[k] = val
                planted.append(r)
    p[:len(planted)] = np.array(planted, dtype=dtype)
    p[100] = [np.nan, 1, 1]
    with np.errstate(invalid="ignore"):
        want = p[REF.in_fov(p, limits)]
    got = filter_points_polar(p, limits).cpu().numpy()
    assert got.dtype == dtype and np.array_equal(got, want)
    kept = REF.in_fov(p[:len(planted)], limits)
    assert kept.reshape(6, 3)[:, 0].all() and 6 <= kept.sum() <= 12            # each bound itself is inside, one neighbour is not


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dropin_transform_lidar_data(dtype):
    """a four-term float64 sum of values up to 30 m: at most 4 eps 30 = 3e-14 between two summation orders"""
    from rald_amd.lidar import T_RADAR_TO_LIDAR, transform_lidar_data
    p = np.random.default_rng(3700).uniform(-30, 30, (1000, 3)).astype(dtype)
    p[0], p[1] = 0, [30, -30, 30]
    want = (np.hstack([p, np.ones((len(p), 1))]) @ T_RADAR_TO_LIDAR.T)[:, :3]
    got = transform_lidar_data(p)
    assert got.dtype == torch.float64 and tuple(got.shape) == (1000, 3)
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"transform_lidar_data {np.dtype(dtype).name}: max |error| {err:.2e}")
    assert err <= 1e-13


def test_dropin_cartesian2polar():
    from rald_amd.lidar import cartesian2polar
    rng = np.random.default_rng(3800)
    p = rng.uniform(-20, 20, (2000, 3))
    p[:8] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-3, 1e-9, 0], [3, 4, 12]]
    got = cartesian2polar(p)
    assert got.dtype == torch.float64
    err = float(np.abs(got.cpu().numpy() - REF.cartesian2polar(p)).max())
    f = p.astype(np.float32)
    got32 = cartesian2polar(f)
    assert got32.dtype == torch.float32
    u = _ulp(got32.cpu().numpy(), REF.polar_f32(f))
    print(f"cartesian2polar: float64 max |error| {err:.2e} degrees, float32 worst {u} ulp")
    assert err <= 1e-12 and u <= 1
