"""tests/lidar_ref.py shown right before it judges a kernel (tests/test_gpu_lidar_stages.py): it reproduces what the reference
project's own code wrote into g23_lidar.npz and g25_lidar_configs.npz (tests/golden/make_golden_lidar.py), its dense-grid empty
cells agree with the rank rule of rald_amd.lidar.empty_cell, and a hand-written frame shows the voxel order rules.  No GPU."""
import hashlib
import os

import numpy as np
import pytest
import torch

import lidar_ref as REF
from conftest import GOLDEN
from test_lidar import FRAMES, NPTS, NUMPY_SIMD_ULP, SEED, SHIPPED, VARIANTS

CART = dict(view_cone_mode=False, pc_range=[0, -8, -2, 16, 8, 2], voxel_size=[0.25, 0.25, 0.125])
CONFIGS = {"iso": dict(norm_anisotropy=False, norm_isotropy=True), "both": dict(norm_anisotropy=True, norm_isotropy=True),
           "none": dict(norm_anisotropy=False, norm_isotropy=False), "cart": dict(CART),
           "cart_iso": dict(CART, norm_anisotropy=False, norm_isotropy=True)}


def config25(tag: str) -> dict:
    return dict(SHIPPED, num_samples=512, **CONFIGS[tag])


def _load(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def g23():
    return _load("g23_lidar.npz")


@pytest.fixture(scope="module")
def g25():
    return _load("g25_lidar_configs.npz")


def _sha(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def _fov(g23):
    f = g23["fov"]
    return [[f[0], f[1]], [f[2], f[3]], [f[4], f[5]]]


def test_crop_reproduces_g23(g23):
    from rald_amd import synth
    for b, raw in enumerate(synth.lidar_scan(FRAMES, SEED, NPTS)):
        keep, rows, polar = REF.crop(raw, g23["extrinsic"], _fov(g23))
        assert np.array_equal(np.packbits(keep), g23[f"crop_keep_b{b}"])
        assert rows.dtype == np.float32 and np.array_equal(rows, g23[f"crop_b{b}"])
        assert np.array_equal(np.nonzero(REF.bound_distance(polar, _fov(g23)) < 1e-9)[0], g23[f"near_b{b}"])
        # numpy's own float32 polar may be ulps off the correctly rounded one (its SIMD kernels)
        d = np.abs(REF.polar_f32(rows).view(np.int32).astype(np.int64) - g23[f"polar_b{b}"].view(np.int32).astype(np.int64))
        assert d.max() <= NUMPY_SIMD_ULP


def test_crop_reproduces_g25(g23, g25):
    from rald_amd import synth
    seed, frames, npts = (int(v) for v in g25["meta"])
    for b, raw in enumerate(synth.lidar_scan(frames, seed, npts)):
        keep, rows, polar = REF.crop(raw, g23["extrinsic"], _fov(g23))
        assert np.array_equal(rows, g25[f"crop_b{b}"]) and keep.sum() == len(rows)
        assert (REF.bound_distance(polar, _fov(g23)) >= 1e-9).all()


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_point_to_voxel_reproduces_g23_digests(g23, tag):
    lc = dict(SHIPPED, **VARIANTS[tag])
    for b in range(FRAMES):
        v, c, n = REF.point_to_voxel(g23[f"polar_b{b}"], lc["voxel_size"], lc["pc_range"], 3, lc["max_points_per_voxel"],
                                     lc["max_number_of_voxels"])
        assert len(v) == int(g23[f"vox_{tag}_b{b}_V"])
        assert v.dtype == np.float32 and c.dtype == np.int32 and n.dtype == np.int32
        for a, want in zip((v, c, n), g23[f"vox_{tag}_b{b}_sha"]):
            assert np.array_equal(_sha(a), want)


def _replay(fix, key_of, cfg, loader, frames):
    """the loader's items 0 .. frames - 1 of one (config, loader) from the stored seeds; yields (key, lp, qp, lab, in_num)"""
    rng = np.random.default_rng(int(fix["seeds"][0]))
    torch.manual_seed(int(fix["seeds"][1]))
    for b in range(frames):
        pts = fix[f"polar_b{b}"] if cfg["view_cone_mode"] else fix[f"crop_b{b}"]
        yield (key_of(loader, b), *REF.replay_item(pts, cfg, loader, rng))


def _check_item(fix, key, lp, qp, lab, in_num):
    for a, want in zip((lp, qp, lab), fix[key + "_sha"]):
        assert a.dtype == np.float32 and np.array_equal(_sha(a), want), key
    assert in_num == int(fix[key + "_in"])
    if key + "_lidar_points" in fix:
        for name, a in (("lidar_points", lp), ("query_points", qp), ("query_labels", lab)):
            assert np.array_equal(a, fix[f"{key}_{name}"]), f"{key}: {name}"


def test_replay_reproduces_g23_ship_train(g23):
    """The shipped cone has 18.2 M cells; its dense grid (18 MB) is allocated here once, on the host, to pin replay_item and
    empty_cells on the full stored arrays ds_ship_train_b0_*."""
    key, lp, qp, lab, in_num = next(_replay(g23, lambda loader, b: f"ds_ship_{loader}_b{b}", dict(SHIPPED), "train", 1))
    assert key + "_lidar_points" in g23
    _check_item(g23, key, lp, qp, lab, in_num)


@pytest.mark.parametrize("loader", ["train", "test"])
@pytest.mark.parametrize("tag", list(CONFIGS))
def test_replay_reproduces_g25(g25, tag, loader):
    cfg = config25(tag)
    assert list(g25["tags"]) == list(CONFIGS)
    assert g25[f"cfg_{tag}_pc_range"].tolist() == [float(v) for v in cfg["pc_range"]]
    assert g25[f"cfg_{tag}_voxel_size"].tolist() == [float(v) for v in cfg["voxel_size"]]
    assert g25[f"cfg_{tag}_flags"].tolist() == [int(cfg[k]) for k in ("view_cone_mode", "norm_anisotropy", "norm_isotropy")]
    n = 0
    for key, lp, qp, lab, in_num in _replay(g25, lambda ld, b: f"ds_{tag}_{ld}_b{b}", cfg, loader, int(g25["meta"][1])):
        _check_item(g25, key, lp, qp, lab, in_num)
        n += key + "_lidar_points" in g25
    assert n == (loader == "train")                               # one frame per tag is stored in full


@pytest.mark.parametrize("seed", range(6))
def test_empty_cells_agrees_with_the_rank_rule(seed):
    """the dense grid against the searchsorted form of rald_amd.lidar.empty_cell: two formulations of nonzero(~occupied)[r]"""
    from rald_amd.lidar import empty_cell
    rng = np.random.default_rng(seed)
    grid = rng.integers(1, 12, 3)
    G = int(np.prod(grid))
    occ = rng.random(G) < [0.0, 0.1, 0.5, 0.9, 0.5, 0.5][seed]
    if seed == 4:
        occ[:3], occ[-2:] = True, True                            # runs at both ends of the grid
    if seed == 5:
        occ[0], occ[-1] = False, False
    keys = np.nonzero(occ)[0]
    if len(keys) == G:
        occ[G // 2] = False
        keys = np.nonzero(occ)[0]
    xyz = np.stack(np.unravel_index(keys, tuple(grid)), axis=1)
    ranks = np.concatenate([[0, G - len(keys) - 1], rng.integers(0, G - len(keys), 50)])
    got = REF.empty_cells(xyz, grid, ranks)
    cell = (got[:, 0] * grid[1] + got[:, 1]) * grid[2] + got[:, 2]
    assert np.array_equal(cell, empty_cell(keys, ranks))
    assert not occ[cell].any()
    assert cell[0] == np.nonzero(~occ)[0][0] and cell[1] == np.nonzero(~occ)[0][-1]


def test_point_to_voxel_order_rules_by_hand():
    """Ten points on a 4 x 1 x 1 grid of unit cells, max_voxels 2, max_points 2.  Cells by point: 2 0 2 3 0 2 out 3 0 out.
    Voxel 0 is cell 2 and voxel 1 is cell 0 (first appearance, not cell order); cell 3 arrives third and is dropped, both times;
    the later points of cells 2 and 0 still count, up to two each, the first two in point order."""
    x = np.array([2.5, 0.5, 2.25, 3.5, 0.25, 2.75, 4.0, 3.25, 0.75, -0.5], dtype=np.float32)
    pts = np.stack([x, np.full(10, 0.5, np.float32), np.arange(10, dtype=np.float32) / 16], axis=1)
    v, c, n = REF.point_to_voxel(pts, [1, 1, 1], [0, 0, 0, 4, 1, 1], 3, 2, 2)
    assert c.tolist() == [[0, 0, 2], [0, 0, 0]]                    # z, y, x
    assert n.tolist() == [2, 2]
    assert np.array_equal(v[0], pts[[0, 2]]) and np.array_equal(v[1], pts[[1, 4]])
    v, c, n = REF.point_to_voxel(pts, [1, 1, 1], [0, 0, 0, 4, 1, 1], 3, 4, 3)
    assert c.tolist() == [[0, 0, 2], [0, 0, 0], [0, 0, 3]] and n.tolist() == [3, 3, 2]
    assert np.array_equal(v[2], np.concatenate([pts[[3, 7]], np.zeros((2, 3), np.float32)]))   # zero-filled past its count
    assert np.array_equal(v[0, :3], pts[[0, 2, 5]]) and not v[0, 3].any()
    e = REF.point_to_voxel(pts[[6, 9]], [1, 1, 1], [0, 0, 0, 4, 1, 1], 3, 2, 2)              # the upper face (x = 4) is outside
    assert [a.shape for a in e] == [(0, 2, 3), (0, 3), (0,)]


def test_norm_points_rounding():
    """isotropic: float64 arithmetic rounded once; after the anisotropic branch when both are on; nothing when both are off"""
    pc = [0, -90, -20, 15.8, 90, 20]
    p = np.random.default_rng(0).uniform([0, -90, -20], [15.8, 90, 20], (64, 3)).astype(np.float32)
    off, sc = np.array([7.9, 0.0, 0.0]), np.array([7.9, 90.0, 20.0])
    t = torch.from_numpy(p.copy())
    REF.norm_points(t, None, pc, False, True)
    assert np.array_equal(t.numpy(), ((p.astype(np.float64) - off) / 90.0).astype(np.float32))
    a = (p - off.astype(np.float32)) / sc.astype(np.float32)
    t = torch.from_numpy(p.copy())
    REF.norm_points(t, None, pc, True, True)
    assert np.array_equal(t.numpy(), ((a.astype(np.float64) - off) / 90.0).astype(np.float32))
    t = torch.from_numpy(p.copy())
    REF.norm_points(t, None, pc, False, False)
    assert np.array_equal(t.numpy(), p)
