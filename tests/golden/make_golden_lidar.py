#!/usr/bin/env python3
"""Generate tests/golden/g23_lidar.npz: the reference's LiDAR path on seeded synthetic scans (rald_amd.synth.lidar_scan).

1. The crop of dataset_preprocessor/lidar.py:170-182, with the reference's own functions (remove_empty_points,
   transform_lidar_data, cartesian2polar, filter_points_polar, polar2cartesian, save_lidar_data's float32 cast).
2. A tiny dataset tree (split json, lidar_sc/{i:04d}.bin = the crop outputs, empty radarcube_raw/*.bin files) read by the
   reference's unmodified ColoRadarDataset(..., loader_type).__getitem__ for 'train' and 'test', with the shipped lidar config and a
   small-cap variant, cache_voxel False, np.random.default_rng patched to return one seeded generator, torch.manual_seed set and
   the radar cube loading switched off (set_load_radar(False)).

spconv and cumm.tensorview are not installed here, so they are stubbed in memory, as easydict and tqdm are.  The stub's
Point2VoxelCPU3d is a RESTATEMENT of spconv's CPU voxelizer rules, not spconv itself: cell c = floor((p - lo) / v) in float32,
outside when c < 0 or c >= grid (grid = round((hi - lo) / v)); voxels numbered in order of their first point; a new voxel beyond
max_voxels is dropped while later points of kept voxels still count; each voxel keeps its first max_points points; coordinates in
z, y, x order; the voxel tensor zero-filled.

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
from rald_amd import synth  # noqa: E402

SEED, FRAMES, NPTS = 2301, 2, 16384
NP_SEED, TORCH_SEED = 99, 7
FOV = {"max_range": 15.863025538680999, "az_range": [-90, 90], "el_range": [-20, 20]}
SHIPPED = dict(pc_range=[0, -90, -20, 15.8, 90, 20], num_point_features=3, voxel_size=[0.05, 0.25, 0.5], max_points_per_voxel=10,
               max_number_of_voxels=50000, sampling=True, num_samples=10000, query_ratio=0.0625, norm_isotropy=False,
               norm_anisotropy=True, cache_voxel=False, view_cone_mode=True)
VARIANTS = {"ship": {}, "cap": dict(max_number_of_voxels=600, max_points_per_voxel=3)}


def sha(a) -> np.ndarray:
    a = np.ascontiguousarray(a.numpy() if hasattr(a, "numpy") else a)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


class Point2VoxelCPU3d:
    """Restatement of spconv's Point2VoxelCPU3d.point_to_voxel rules (see the module docstring); not spconv's source."""

    def __init__(self, vsize_xyz, coors_range_xyz, num_point_features, max_num_points_per_voxel, max_num_voxels):
        self.v = np.asarray(vsize_xyz, dtype=np.float32)
        self.lo = np.asarray(coors_range_xyz[:3], dtype=np.float32)
        r = np.asarray(coors_range_xyz, dtype=np.float64)
        self.grid = np.round((r[3:] - r[:3]) / np.asarray(vsize_xyz, dtype=np.float64)).astype(np.int64)
        self.F, self.maxp, self.maxv = int(num_point_features), int(max_num_points_per_voxel), int(max_num_voxels)

    def point_to_voxel(self, points):
        pts = np.asarray(points, dtype=np.float32)
        c = np.floor((pts[:, :3] - self.lo) / self.v)                          # float32 throughout
        inside = np.all((c >= 0) & (c < self.grid.astype(np.float32)), axis=1)
        voxels = np.zeros((self.maxv, self.maxp, self.F), dtype=np.float32)
        coords = np.zeros((self.maxv, 3), dtype=np.int32)
        num = np.zeros((self.maxv,), dtype=np.int32)
        ids = {}
        for i in np.nonzero(inside)[0]:
            key = (int(c[i, 2]), int(c[i, 1]), int(c[i, 0]))                  # z, y, x
            v = ids.get(key)
            if v is None:
                if len(ids) >= self.maxv:
                    continue
                v = ids[key] = len(ids)
                coords[v] = key
            if num[v] < self.maxp:
                voxels[v, num[v]] = pts[i]
                num[v] += 1
        V = len(ids)

        class T:
            def __init__(self, a):
                self.a = a

            def numpy(self):
                return self.a.copy()
        return T(voxels[:V]), T(coords[:V]), T(num[:V])


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


if __name__ == "__main__":
    main()
