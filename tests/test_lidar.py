"""LiDAR front end on the device (rald_amd.lidar, rald_amd/csrc/lidar.hip) against the reference's crop (dataset_preprocessor/lidar.py)
and ColoRadarDataset.__getitem__ (tests/golden/make_golden_lidar.py -> g23_lidar.npz).  The raw scans are regenerated from the
generator's seed with rald_amd.synth.lidar_scan."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from lidar_ref import polar_f32 as _polar_correctly_rounded

SEED, FRAMES, NPTS = 2301, 2, 16384
SHIPPED = dict(pc_range=[0, -90, -20, 15.8, 90, 20], num_point_features=3, voxel_size=[0.05, 0.25, 0.5], max_points_per_voxel=10,
               max_number_of_voxels=50000, sampling=True, num_samples=10000, query_ratio=0.0625, norm_isotropy=False,
               norm_anisotropy=True, cache_voxel=False, view_cone_mode=True)
VARIANTS = {"ship": {}, "cap": dict(max_number_of_voxels=600, max_points_per_voxel=3)}
NUMPY_SIMD_ULP = 4     # numpy's float32 arctan2 / arcsin (SIMD kernels) are within 3 ulp of the correctly rounded value


@pytest.fixture(scope="module")
def g23():
    with np.load(os.path.join(GOLDEN, "g23_lidar.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _cfg(**over):
    from rald_amd.lidar import load_lidar_config
    return load_lidar_config({"dataset": {"lidar": dict(SHIPPED, **over)}})


def _sha(a) -> np.ndarray:
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def _ulp(a, b) -> int:
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def _keys(polar: np.ndarray, cfg) -> np.ndarray:
    lo = np.asarray(cfg.pc_range[:3], dtype=np.float32)
    v = np.asarray(cfg.voxel_size, dtype=np.float32)
    c = np.floor((polar - lo) / v)
    g = np.asarray(cfg.grid_size)
    inside = np.all((c >= 0) & (c < g.astype(np.float32)), axis=1)
    k = (c[:, 0].astype(np.int64) * g[1] + c[:, 1].astype(np.int64)) * g[2] + c[:, 2].astype(np.int64)
    return np.where(inside, k, -1)


# ---- CPU ----------------------------------------------------------------------------------------
def test_load_lidar_config_yaml_and_sections(tmp_path):
    from rald_amd.lidar import T_RADAR_TO_LIDAR, load_lidar_config
    y = tmp_path / "ae.yml"
    lines = ["dataset:", "  split_file: split.json", "  lidar:"]
    for k, v in SHIPPED.items():
        lines.append(f"    {k}: {v}")
    y.write_text("\n".join(lines) + "\n")
    pre = tmp_path / "pre.yaml"
    pre.write_text("single_chip_mode:\n  lidar:\n    FOV:\n      max_range: 12.5\n      az_range: [-60, 60]\n      el_range: [-15, 15]\n")
    a = load_lidar_config(y)
    b = load_lidar_config({"lidar": dict(SHIPPED)}, pre)
    for cfg in (a, b):
        assert list(cfg.pc_range) == SHIPPED["pc_range"] and list(cfg.voxel_size) == SHIPPED["voxel_size"]
        assert cfg.max_number_of_voxels == 50000 and cfg.max_points_per_voxel == 10 and cfg.num_samples == 10000
        assert cfg.view_cone_mode is True and cfg.norm_anisotropy is True and cfg.norm_isotropy is False
        assert cfg.grid_size.tolist() == [316, 720, 80]
        assert cfg.extrinsic is T_RADAR_TO_LIDAR
    assert a.fov == [[0, 15.863025538680999], [-90, 90], [-20, 20]]
    assert b.fov == [[0, 12.5], [-60, 60], [-15, 15]]
    with pytest.raises(KeyError):
        load_lidar_config({"lidar": {"pc_range": SHIPPED["pc_range"]}})


def test_extrinsic_matches_reference(g23):
    from rald_amd.lidar import T_RADAR_TO_LIDAR
    assert np.abs(T_RADAR_TO_LIDAR - g23["extrinsic"]).max() <= 1e-15


def test_grid_sizes_and_workspace_are_host_arithmetic():
    from rald_amd.lidar import LidarFrames, grid_size, workspace_bytes
    cone = _cfg()
    vox = _cfg(pc_range=[0, -15, -5, 15, 15, 5], voxel_size=[0.05, 0.05, 0.05], view_cone_mode=False)
    assert grid_size(cone).tolist() == [316, 720, 80] and grid_size(vox).tolist() == [300, 600, 200]
    h = LidarFrames(cone)                         # create allocates nothing on the device
    assert h.cells == 316 * 720 * 80
    w1, w8 = workspace_bytes(cone, 1, 65536), workspace_bytes(cone, 8, 8 * 65536)
    assert 0 < w1 < w8 and w8 >= 7 * 8 * 65536 * 4
    assert workspace_bytes(cone, 3, 0) > 0
    with pytest.raises(RuntimeError, match="voxel_size"):
        LidarFrames(_cfg(voxel_size=[0.05, 0.0, 0.5]))
    with pytest.raises(RuntimeError, match="voxel_size"):
        LidarFrames(_cfg(voxel_size=[-0.05, 0.25, 0.5]))
    with pytest.raises(RuntimeError, match="2\\^31"):
        LidarFrames(_cfg(voxel_size=[0.001, 0.01, 0.01]))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_empty_rank_rule_matches_nonzero(seed):
    """get_empty_voxel_centers (Coloradar_dataset.py:335-363) takes nonzero(~occupied)[perm]: the r-th empty cell is r + j for the
    smallest j with k_j - j > r over the sorted occupied cells k."""
    from rald_amd.lidar import empty_cell
    g = torch.Generator().manual_seed(seed)
    grid = tuple(int(v) for v in torch.randint(2, 9, (3,), generator=g))
    G = grid[0] * grid[1] * grid[2]
    occ = torch.rand(grid, generator=g) < [0.1, 0.5, 0.9, 0.0][seed]
    if seed == 2:
        occ.view(-1)[0] = True
        occ.view(-1)[-1] = True
    empty = torch.nonzero(~occ.flatten()).squeeze(1)
    keys = torch.nonzero(occ.flatten()).squeeze(1).numpy()
    r = np.arange(len(empty))
    assert np.array_equal(empty_cell(keys, r), empty.numpy())
    assert G - len(keys) == len(empty)


def test_unbuilt_options_raise():
    from rald_amd.lidar import LidarFrames
    for over in (dict(shuffle_pts=True), dict(DOUBLE_FLIP=True)):
        with pytest.raises(NotImplementedError):
            LidarFrames(_cfg(**over)).batch([np.zeros((10, 3), np.float32)])


# ---- GPU ----------------------------------------------------------------------------------------
def _pack(frames):
    from rald_amd.lidar import _pack
    flat, offs, _ = _pack(frames, 3)
    return torch.from_numpy(flat).cuda(), offs


@pytest.mark.gpu
def test_crop_matches_reference(g23):
    from rald_amd import synth
    from rald_amd.lidar import LidarFrames
    scans = synth.lidar_scan(FRAMES, SEED, NPTS)
    h = LidarFrames(_cfg())
    x, offs = _pack(scans)
    out, counts = h.crop(x, offs)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    for b in range(FRAMES):
        ref = g23[f"crop_b{b}"]
        keep = np.unpackbits(g23[f"crop_keep_b{b}"])[:NPTS].astype(bool)
        assert len(g23[f"near_b{b}"]) == 0          # no point within 1e-9 of a FOV bound: the kept sets must be equal
        assert counts[b] == keep.sum() == len(ref)
        got = out[offs[b]:offs[b] + counts[b]]
        assert _ulp(got, ref) <= 1, f"frame {b}: cropped points differ by more than 1 ulp"
        print(f"crop frame {b}: {counts[b]} kept, {int((got != ref).any(axis=1).sum())} rows differ by 1 ulp")


@pytest.mark.gpu
def test_polar_conversion(g23):
    from rald_amd.lidar import LidarFrames
    h = LidarFrames(_cfg())
    frames = [g23[f"crop_b{b}"] for b in range(FRAMES)]
    x, offs = _pack(frames)
    pol = h.voxelize(x, offs, to_polar=True, with_voxels=False)["polar"].cpu().numpy()
    for b in range(FRAMES):
        got = pol[offs[b]:offs[b + 1]]
        cr = _polar_correctly_rounded(frames[b])
        assert _ulp(got, cr) <= 1
        ref = g23[f"polar_b{b}"]
        d = _ulp(got, ref)
        assert d <= NUMPY_SIMD_ULP
        print(f"polar frame {b}: {int((got != ref).any(axis=1).sum())} of {len(got)} rows differ from numpy's float32 "
              f"(max {d} ulp), {int((got != cr).any(axis=1).sum())} from the correctly rounded value")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(VARIANTS))
def test_voxelize_bit_identical(g23, tag):
    from rald_amd.lidar import LidarFrames, VoxelGeneratorWrapper
    cfg = _cfg(**VARIANTS[tag])
    h = LidarFrames(cfg)
    frames = [g23[f"polar_b{b}"] for b in range(FRAMES)]
    x, offs = _pack(frames)
    res = h.voxelize(x, offs)
    for b in range(FRAMES):
        V = int(res["voxel_counts"][b])
        assert V == int(g23[f"vox_{tag}_b{b}_V"])
        got = [res["voxels"][b, :V], res["coords"][b, :V], res["num_points"][b, :V]]
        for name, t, want in zip(("voxels", "coords", "num_points"), got, g23[f"vox_{tag}_b{b}_sha"]):
            assert np.array_equal(_sha(t), want), f"{tag} frame {b}: {name} differ"
        if tag == "cap":
            assert V == cfg.max_number_of_voxels and int(res["num_points"][b, :V].max()) <= cfg.max_points_per_voxel
        keys = res["kept_keys"][b, :V].cpu().numpy().astype(np.int64)
        c = res["coords"][b, :V].cpu().numpy().astype(np.int64)
        g = cfg.grid_size
        assert np.array_equal(keys, np.sort((c[:, 2] * g[1] + c[:, 1]) * g[2] + c[:, 0]))
    w = VoxelGeneratorWrapper(cfg.voxel_size, cfg.pc_range, 3, cfg.max_points_per_voxel, cfg.max_number_of_voxels)
    v, c, n = w.generate(frames[0])
    assert v.dtype == np.float32 and c.dtype == np.int32 and n.dtype == np.int32
    assert [_sha(a).tolist() for a in (v, c, n)] == [s.tolist() for s in g23[f"vox_{tag}_b0_sha"]]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(VARIANTS))
@pytest.mark.parametrize("loader", ["train", "test"])
def test_batch_replays_reference_dicts(g23, tag, loader):
    """numpy's float32 polar rows in (polar=True): every value of the collated dict is bit-identical to the reference's."""
    from rald_amd.lidar import LidarFrames
    h = LidarFrames(_cfg(**VARIANTS[tag]))
    frames = [g23[f"polar_b{b}"] for b in range(FRAMES)]
    torch.manual_seed(int(g23["seeds"][1]))
    d = h.batch(frames, loader, rng=np.random.default_rng(int(g23["seeds"][0])), polar=True)
    assert d["raw_query_points"] is d["query_points"]
    assert ("raw_lidar_points" in d) == (loader != "train")
    for b in range(FRAMES):
        key = f"ds_{tag}_{loader}_b{b}"
        for name, want in zip(("lidar_points", "query_points", "query_labels"), g23[key + "_sha"]):
            assert np.array_equal(_sha(d[name][b]), want), f"{key}: {name} differ"
        assert int(d["in_voxel_num"][b]) == int(g23[key + "_in"])


@pytest.mark.gpu
def test_batch_from_cartesian_files(g23):
    """The lidar_sc files in: values not derived from a point whose device polar differs from numpy's are bit-identical."""
    from rald_amd.lidar import LidarFrames
    cfg = _cfg()
    h = LidarFrames(cfg)
    frames = [g23[f"crop_b{b}"] for b in range(FRAMES)]
    torch.manual_seed(int(g23["seeds"][1]))
    d = h.batch(frames, "train", rng=np.random.default_rng(int(g23["seeds"][0])))
    x, offs = _pack(frames[:1])
    dev_pol = h.voxelize(x, offs, to_polar=True, with_voxels=False)["polar"].cpu().numpy()
    ref_pol = g23["polar_b0"]
    same = (dev_pol == ref_pol).all(axis=1)
    idx = np.random.default_rng(int(g23["seeds"][0])).choice(len(ref_pol), cfg.num_samples, replace=False)
    lp, want = d["lidar_points"][0].cpu().numpy(), g23["ds_ship_train_b0_lidar_points"]
    assert np.array_equal(lp[same[idx]], want[same[idx]])
    assert _ulp(lp, want) <= NUMPY_SIMD_ULP + 1
    if np.array_equal(_keys(dev_pol, cfg), _keys(ref_pol, cfg)):     # the same cells: the same voxels, the same queries
        assert np.array_equal(d["query_points"][0].cpu().numpy(), g23["ds_ship_train_b0_query_points"])
    else:
        eq = (d["query_points"][0].cpu().numpy() == g23["ds_ship_train_b0_query_points"]).all(axis=1)
        assert eq.mean() > 0.99
    assert np.array_equal(d["query_labels"][0].cpu().numpy(), g23["ds_ship_train_b0_query_labels"])
    print(f"cartesian batch: {int((~same).sum())} of {len(same)} points with a polar differing from numpy's")


@pytest.mark.gpu
def test_frame_alone_equals_frame_in_mixed_batch():
    from rald_amd import synth
    from rald_amd.lidar import LidarFrames
    sizes = [16384, 9000, 30000, 17001, 4096]
    scans = [synth.lidar_scan(1, 40 + i, n)[0] for i, n in enumerate(sizes)]
    h = LidarFrames(_cfg())

    def run(frames):
        x, offs = _pack(frames)
        out, counts = h.crop(x, offs)
        v = h.voxelize(out[:, :3].contiguous(), offs, counts, to_polar=True)
        return offs, out, counts, v

    offs5, out5, c5, v5 = run(scans)
    for b in (0, 2, 4):
        offs1, out1, c1, v1 = run([scans[b]])
        n = int(c1[0])
        assert n == int(c5[b])
        assert torch.equal(out1[:n], out5[offs5[b]:offs5[b] + n])
        V = int(v1["voxel_counts"][0])
        assert V == int(v5["voxel_counts"][b])
        for k in ("voxels", "coords", "num_points", "kept_keys"):
            assert torch.equal(v1[k][0, :V], v5[k][b, :V]), k
        assert torch.equal(v1["polar"][:n], v5["polar"][offs5[b]:offs5[b] + n])


@pytest.mark.gpu
def test_device_generator_queries_land_in_the_right_cells():
    from rald_amd import synth
    from rald_amd.lidar import LidarFrames
    cfg = _cfg()
    h = LidarFrames(cfg)
    scans = synth.lidar_scan(3, 77, NPTS)
    g = torch.Generator("cuda").manual_seed(5)
    d = h.batch(scans, "train", rng=g, crop=True)
    x, offs = _pack(scans)
    out, counts = h.crop(x, offs)
    vox = h.voxelize(out, offs, counts, to_polar=True, with_voxels=False)
    lo, hi = np.array(cfg.pc_range[:3]), np.array(cfg.pc_range[3:])
    off, scale = (hi + lo) / 2, (hi - lo) / 2
    n_in = int(cfg.num_samples * cfg.query_ratio)
    for b in range(3):
        V = int(vox["voxel_counts"][b])
        kept = set(vox["kept_keys"][b, :V].cpu().numpy().tolist())
        q = d["query_points"][b].cpu().double().numpy() * scale + off                    # undo the anisotropic normalisation
        c = np.floor((q - lo) / np.array(cfg.voxel_size)).astype(np.int64)
        g3 = cfg.grid_size
        k = (c[:, 0] * g3[1] + c[:, 1]) * g3[2] + c[:, 2]
        inside = np.array([kk in kept for kk in k])
        lab = d["query_labels"][b].cpu().numpy()
        assert (lab[:n_in] == 1).all() and (lab[n_in:] == 0).all()
        assert inside[:n_in].mean() > 0.995 and (~inside[n_in:]).mean() > 0.995   # a query on a cell face may round across it
        assert np.isfinite(d["lidar_points"][b].cpu().numpy()).all()


@pytest.mark.gpu
def test_error_paths():
    from rald_amd.lidar import LidarFrames
    h = LidarFrames(_cfg())
    rng = np.random.default_rng(0)
    small = np.stack([rng.uniform(1, 10, 500), rng.uniform(-80, 80, 500), rng.uniform(-15, 15, 500)], axis=1).astype(np.float32)
    with pytest.raises(ValueError):                                  # N < num_samples
        h.batch([small], "train", polar=True)
    far = np.stack([np.full(12000, 15.85), rng.uniform(-80, 80, 12000), rng.uniform(-15, 15, 12000)], axis=1).astype(np.float32)
    with pytest.raises(ValueError):                                  # no voxel kept (r outside the grid, inside the crop)
        h.batch([far], "train", polar=True)
    with pytest.raises(ValueError):
        h.batch([far], "test", polar=True)
    d = h.batch([far], "train", polar=True, load_query=False)       # without queries the samples still come
    assert d["lidar_points"].shape == (1, 10000, 3) and "query_points" not in d


@pytest.mark.gpu
def test_process_lidar_files(g23, tmp_path):
    from rald_amd import synth
    from rald_amd.lidar import process_lidar_files
    scans = synth.lidar_scan(FRAMES, SEED, NPTS)
    files = []
    for b, s in enumerate(scans):
        p = tmp_path / f"lidar_pointcloud_{b}.bin"
        s.tofile(p)
        files.append(p)
    n = process_lidar_files(files, [1, 0], tmp_path / "lidar_sc", _cfg(), batch=1)
    assert n == 2
    for i, b in enumerate([1, 0]):
        got = np.fromfile(tmp_path / "lidar_sc" / f"{i:04d}.bin", dtype=np.float32).reshape(-1, 3)
        ref = g23[f"crop_b{b}"]
        assert got.shape == ref.shape and _ulp(got, ref) <= 1


@pytest.mark.gpu
def test_raw_scan_to_encode_chain_is_finite():
    from rald_amd import models_ae as A, synth, weights
    from rald_amd.lidar import LidarFrames
    h = LidarFrames(_cfg(num_samples=2048))
    d = h.batch(synth.lidar_scan(2, 91, NPTS), "test", crop=True, rng=torch.Generator("cuda").manual_seed(3))
    m = A.create_autoencoder(query_type="mix", N=2048)
    m.load_state_dict(weights.make_state_dict(weights.spec_of_state_dict(m.state_dict()), 0), strict=True)
    m = m.cuda()
    with torch.no_grad():
        kl, z = m.encode(d["lidar_points"])
    assert torch.isfinite(z).all() and torch.isfinite(kl).all()
    assert len(d["raw_lidar_points"]) == 2 and d["query_labels"].eq(1).all()
