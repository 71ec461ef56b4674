#!/usr/bin/env python3
"""Generate tests/golden/g23_lidar.npz: the reference's LiDAR path on seeded synthetic scans (rald_amd.synth.lidar_scan).

1. The crop of dataset_preprocessor/lidar.py:170-182, with the reference's own functions (remove_empty_points,
   transform_lidar_data, cartesian2polar, filter_points_polar, polar2cartesian, save_lidar_data's float32 cast).
2. A tiny dataset tree (split json, lidar_sc/{i:04d}.bin = the crop outputs, empty radarcube_raw/*.bin files) read by the
   reference's unmodified ColoRadarDataset(..., loader_type).__getitem__ for 'train' and 'test', with the shipped lidar config and a
   small-cap variant, cache_voxel False, np.random.default_rng patched to return one seeded generator, torch.manual_seed set and
   the radar cube loading switched off (set_load_radar(False)).

spconv and cumm.tensorview are not installed here, so they are stubbed in memory, as easydict and tqdm are.  The stub's
Point2VoxelCPU3d is a RESTATEMENT of spconv's CPU voxelizer rules, not spconv itself (tests/lidar_ref.py:point_to_voxel, the one
copy): cell c = floor((p - lo) / v) in float32, outside when c < 0 or c >= grid (grid = round((hi - lo) / v)); voxels numbered in
order of their first point; a new voxel beyond max_voxels is dropped while later points of kept voxels still count; each voxel
keeps its first max_points points; coordinates in z, y, x order; the voxel tensor zero-filled.

3. g25_lidar_configs.npz: the same loader away from the shipped flags, on scans of 4096 points (seed 2501) with num_samples 512,
   'train' and 'test', tags iso / both / none (the norm flags), cart / cart_iso (view_cone_mode False on a 64 x 64 x 32 grid).
   Stored: crop_b{b}, polar_b{b} as below; cfg_{tag}_pc_range / _voxel_size / _flags (view cone, anisotropic, isotropic);
   ds_{tag}_{loader}_b{b}_sha / _in as below; the full arrays of ds_{tag}_train_b0.

The scans are not stored (tests regenerate them from SEED).  Stored:
  fov, pc_range_*, voxel_size_*, caps     the configs used;  extrinsic  the reference's T_RADAR_TO_LIDAR (scipy-built)
  crop_keep_b{b}    packed bits over the scan's points: survivors of the reference's crop
  crop_b{b}         the reference's lidar_sc file contents, float32 [M, 3]
  near_b{b}         indices of scan points whose float64 polar lies within 1e-9 of a FOV bound (the crop may differ there)
  polar_b{b}        numpy's float32 cartesian2polar of crop_b{b} (the dataset's points; transcendentals may differ by ulps from a
                    correctly rounded float32 result depending on numpy's SIMD kernels)
  vox_{tag}_b{b}_V, _sha   kept voxels and sha256 of (voxels, coords, num_points) of the stub on polar_b{b}
  ds_{tag}_{loader}_b{b}_sha   sha256 of lidar_points, query_points, query_labels of __getitem__(b); _in  in_voxel_num
  ds_ship_train_b0_lidar_points / _query_points / _query_labels    the full arrays of one item
  seeds             (numpy seed, torch seed) of the replay

Usage:  python tests/golden/make_golden_lidar.py REFERENCE_ROOT
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lidar_ref  # noqa: E402
from rald_amd import synth  # noqa: E402

SEED, FRAMES, NPTS = 2301, 2, 16384
NP_SEED, TORCH_SEED = 99, 7
FOV = {"max_range": 15.863025538680999, "az_range": [-90, 90], "el_range": [-20, 20]}
SHIPPED = dict(pc_range=[0, -90, -20, 15.8, 90, 20], num_point_features=3, voxel_size=[0.05, 0.25, 0.5], max_points_per_voxel=10,
               max_number_of_voxels=50000, sampling=True, num_samples=10000, query_ratio=0.0625, norm_isotropy=False,
               norm_anisotropy=True, cache_voxel=False, view_cone_mode=True)
VARIANTS = {"ship": {}, "cap": dict(max_number_of_voxels=600, max_points_per_voxel=3)}
# g25_lidar_configs.npz: the shipped section with num_samples 512 on scans of 4096 points, and per tag the change from it
SEED25, NPTS25 = 2501, 4096
BASE25 = dict(num_samples=512)
CART = dict(view_cone_mode=False, pc_range=[0, -8, -2, 16, 8, 2], voxel_size=[0.25, 0.25, 0.125])      # 64 x 64 x 32 cells
CONFIGS = {"iso": dict(norm_anisotropy=False, norm_isotropy=True), "both": dict(norm_anisotropy=True, norm_isotropy=True),
           "none": dict(norm_anisotropy=False, norm_isotropy=False), "cart": dict(CART),
           "cart_iso": dict(CART, norm_anisotropy=False, norm_isotropy=True)}


def sha(a) -> np.ndarray:
    a = np.ascontiguousarray(a.numpy() if hasattr(a, "numpy") else a)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


class Point2VoxelCPU3d:
    """spconv's constructor and call shape around the restated rules of tests/lidar_ref.py:point_to_voxel; not spconv's source."""

    def __init__(self, vsize_xyz, coors_range_xyz, num_point_features, max_num_points_per_voxel, max_num_voxels):
        self.v, self.r = [float(v) for v in vsize_xyz], [float(v) for v in coors_range_xyz]
        self.F, self.maxp, self.maxv = int(num_point_features), int(max_num_points_per_voxel), int(max_num_voxels)

    def point_to_voxel(self, points):
        class T:
            def __init__(self, a):
                self.a = a

            def numpy(self):
                return self.a.copy()
        return tuple(T(a) for a in lidar_ref.point_to_voxel(points, self.v, self.r, self.F, self.maxp, self.maxv))


def install_stubs():
    class ED(dict):
        __getattr__ = dict.__getitem__

        def __setattr__(self, k, v):
            self[k] = v
    ed = types.ModuleType("easydict")
    ed.EasyDict = ED
    sys.modules["easydict"] = ed
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda x, *a, **k: x
    sys.modules["tqdm"] = tq
    sp = types.ModuleType("spconv")
    spu = types.ModuleType("spconv.utils")
    spu.Point2VoxelCPU3d = Point2VoxelCPU3d
    sp.utils = spu
    sys.modules["spconv"] = sp
    sys.modules["spconv.utils"] = spu
    cu = types.ModuleType("cumm")
    tv = types.ModuleType("cumm.tensorview")
    tv.from_numpy = lambda a: a
    cu.tensorview = tv
    sys.modules["cumm"] = cu
    sys.modules["cumm.tensorview"] = tv
    return ED


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(HERE, "g23_lidar.npz"))
    ap.add_argument("--out-configs", default=os.path.join(HERE, "g25_lidar_configs.npz"))
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    ED = install_stubs()
    sys.path.insert(0, ref)
    import torch
    from dataset_preprocessor import lidar as L
    from dataset_preprocessor.constants import T_RADAR_TO_LIDAR
    from datasets.aligned_coloradar.Coloradar_dataset import ColoRadarDataset

    out = {"fov": np.array([0, FOV["max_range"], *FOV["az_range"], *FOV["el_range"]], dtype=np.float64),
           "extrinsic": np.asarray(T_RADAR_TO_LIDAR, dtype=np.float64), "seeds": np.array([NP_SEED, TORCH_SEED]),
           "meta": np.array([SEED, FRAMES, NPTS])}
    limits = [[0, FOV["max_range"]], FOV["az_range"], FOV["el_range"]]
    scans = synth.lidar_scan(FRAMES, SEED, NPTS)
    crops = []
    for b, raw in enumerate(scans):
        xyz = raw[:, :3]
        pts = L.remove_empty_points(xyz)
        pol = L.cartesian2polar(L.transform_lidar_data(pts))
        kept = L.polar2cartesian(L.filter_points_polar(pol, limits)).astype(np.float32)
        # the same chain with the row indices kept
        nz = np.nonzero(np.linalg.norm(xyz, axis=1) > 0)[0]
        m = np.logical_and.reduce([pol[:, 0] >= limits[0][0], pol[:, 0] <= limits[0][1], pol[:, 1] >= limits[1][0],
                                   pol[:, 1] <= limits[1][1], pol[:, 2] >= limits[2][0], pol[:, 2] <= limits[2][1]])
        keep = np.zeros(len(xyz), bool)
        keep[nz[m]] = True
        assert keep.sum() == len(kept)
        dist = np.min(np.abs(np.stack([pol[:, 0] - limits[0][1], pol[:, 1] - limits[1][0], pol[:, 1] - limits[1][1],
                                        pol[:, 2] - limits[2][0], pol[:, 2] - limits[2][1]], axis=1)), axis=1)
        out[f"crop_keep_b{b}"] = np.packbits(keep)
        out[f"crop_b{b}"] = kept
        out[f"near_b{b}"] = nz[dist < 1e-9].astype(np.int64)
        out[f"polar_b{b}"] = L.cartesian2polar(kept)
        assert out[f"polar_b{b}"].dtype == np.float32
        crops.append(kept)
        print(f"frame {b}: {len(xyz)} points, {len(nz)} non-empty, {len(kept)} kept, {len(out[f'near_b{b}'])} near a bound")

    for tag, over in VARIANTS.items():
        lc = dict(SHIPPED, **over)
        out[f"caps_{tag}"] = np.array([lc["max_points_per_voxel"], lc["max_number_of_voxels"]])
        for b in range(FRAMES):
            gen = Point2VoxelCPU3d(lc["voxel_size"], lc["pc_range"], 3, lc["max_points_per_voxel"], lc["max_number_of_voxels"])
            v, c, n = (t.numpy() for t in gen.point_to_voxel(out[f"polar_b{b}"]))
            out[f"vox_{tag}_b{b}_V"] = np.array(len(v))
            out[f"vox_{tag}_b{b}_sha"] = np.stack([sha(v), sha(c), sha(n)])
            print(f"{tag} frame {b}: {len(v)} voxels")

    with tempfile.TemporaryDirectory() as root:
        seq = os.path.join(root, "seq0")
        os.makedirs(os.path.join(seq, "lidar_sc"))
        os.makedirs(os.path.join(seq, "single_chip", "radarcube_raw"))
        for b, kept in enumerate(crops):
            L.save_lidar_data(kept, os.path.join(seq, "lidar_sc", f"{b:04d}.bin"))
            open(os.path.join(seq, "single_chip", "radarcube_raw", f"{b:04d}.bin"), "wb").close()
        with open(os.path.join(root, "split.json"), "w") as f:
            json.dump({"train": ["seq0"], "val": ["seq0"], "test": ["seq0"]}, f)
        orig = np.random.default_rng
        for tag, over in VARIANTS.items():
            cfg = ED(split_file="split.json", lidar=ED(dict(SHIPPED, **over)), radar=ED())
            for loader in ("train", "test"):
                ds = ColoRadarDataset(root, cfg, "scRadar", loader)
                ds.set_load_radar(False)
                g = orig(NP_SEED)
                np.random.default_rng = lambda *a, **k: g
                torch.manual_seed(TORCH_SEED)
                try:
                    for b in range(FRAMES):
                        d = ds[b]
                        key = f"ds_{tag}_{loader}_b{b}"
                        out[key + "_sha"] = np.stack([sha(d["lidar_points"]), sha(d["query_points"]), sha(d["query_labels"])])
                        out[key + "_in"] = np.array(d["in_voxel_num"])
                        assert d["query_points"] is d["raw_query_points"]
                        if loader == "test":
                            assert np.array_equal(d["raw_lidar_points"], crops[b])
                        if tag == "ship" and loader == "train" and b == 0:
                            out[key + "_lidar_points"] = d["lidar_points"].numpy()
                            out[key + "_query_points"] = d["query_points"].numpy()
                            out[key + "_query_labels"] = d["query_labels"].numpy()
                finally:
                    np.random.default_rng = orig
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out) / 1e3:.0f} KB")
    configs_fixture(ED, L, torch, ColoRadarDataset, limits, args.out_configs)


def configs_fixture(ED, L, torch, ColoRadarDataset, limits, path):
    """g25_lidar_configs.npz: the unmodified loader away from the shipped flags (CONFIGS), on two scans of NPTS25 points."""
    out = {"seeds": np.array([NP_SEED, TORCH_SEED]), "meta": np.array([SEED25, FRAMES, NPTS25]), "tags": np.array(list(CONFIGS))}
    crops = []
    for b, raw in enumerate(synth.lidar_scan(FRAMES, SEED25, NPTS25)):
        pol = L.cartesian2polar(L.transform_lidar_data(L.remove_empty_points(raw[:, :3])))
        kept = L.polar2cartesian(L.filter_points_polar(pol, limits)).astype(np.float32)
        out[f"crop_b{b}"] = kept
        out[f"polar_b{b}"] = L.cartesian2polar(kept)
        assert out[f"polar_b{b}"].dtype == np.float32
        crops.append(kept)
        print(f"configs frame {b}: {len(raw)} points, {len(kept)} kept")
    with tempfile.TemporaryDirectory() as root:
        seq = os.path.join(root, "seq0")
        os.makedirs(os.path.join(seq, "lidar_sc"))
        os.makedirs(os.path.join(seq, "single_chip", "radarcube_raw"))
        for b, kept in enumerate(crops):
            L.save_lidar_data(kept, os.path.join(seq, "lidar_sc", f"{b:04d}.bin"))
            open(os.path.join(seq, "single_chip", "radarcube_raw", f"{b:04d}.bin"), "wb").close()
        with open(os.path.join(root, "split.json"), "w") as f:
            json.dump({"train": ["seq0"], "val": ["seq0"], "test": ["seq0"]}, f)
        orig = np.random.default_rng
        for tag, over in CONFIGS.items():
            lc = dict(SHIPPED, **BASE25, **over)
            out[f"cfg_{tag}_pc_range"] = np.array(lc["pc_range"], dtype=np.float64)
            out[f"cfg_{tag}_voxel_size"] = np.array(lc["voxel_size"], dtype=np.float64)
            out[f"cfg_{tag}_flags"] = np.array([lc["view_cone_mode"], lc["norm_anisotropy"], lc["norm_isotropy"]], dtype=np.int64)
            cfg = ED(split_file="split.json", lidar=ED(lc), radar=ED())
            for loader in ("train", "test"):
                ds = ColoRadarDataset(root, cfg, "scRadar", loader)
                ds.set_load_radar(False)
                g = orig(NP_SEED)
                np.random.default_rng = lambda *a, **k: g
                torch.manual_seed(TORCH_SEED)
                try:
                    for b in range(FRAMES):
                        d = ds[b]
                        key = f"ds_{tag}_{loader}_b{b}"
                        out[key + "_sha"] = np.stack([sha(d["lidar_points"]), sha(d["query_points"]), sha(d["query_labels"])])
                        out[key + "_in"] = np.array(d["in_voxel_num"])
                        if b == 0 and loader == "train":
                            out[key + "_lidar_points"] = d["lidar_points"].numpy()
                            out[key + "_query_points"] = d["query_points"].numpy()
                            out[key + "_query_labels"] = d["query_labels"].numpy()
                finally:
                    np.random.default_rng = orig
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    main()
