"""Plain reference of each stage of the LiDAR front end (rald_amd/csrc/lidar.hip, rald_amd/lidar.py): numpy, and CPU torch where the
reference project's loader itself computes with torch.  The rules are those of dataset_preprocessor/lidar.py (the offline crop) and
of ColoRadarDataset.__getitem__ with spconv's Point2VoxelCPU3d behind it, restated; nothing here takes a shortcut the device takes
(no sort, no prefix sums, no binary search: a dictionary in point order, a dense occupancy grid).

    crop             remove_empty_points, extrinsic, cartesian2polar, filter_points_polar, polar2cartesian (float64), float32 cast
    polar_f32        numpy's float32 cartesian2polar with the transcendentals correctly rounded
    grid_of, passes  the grid of a config and the radix passes its keys need (8 bits per pass, the outside key = cells)
    point_to_voxel   the ordered-dictionary loop of spconv's CPU voxelizer
    empty_cells      nonzero(~occupied)[ranks] on a dense grid
    queries          voxel centres + offsets, empty-cell centres + offsets, labels, norm_points (CPU torch)
    norm_points      the anisotropic and the isotropic branch as the loader writes them
    replay_item      one __getitem__ from float32 points, the draws in the loader's order
"""
import warnings

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------- crop
def cartesian2polar(p: np.ndarray) -> np.ndarray:
    """r, -degrees(atan2(y, x)), degrees(asin(z / r)) in the dtype of `p`, as numpy evaluates it"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        r = np.sqrt(x ** 2 + y ** 2 + z ** 2)
        az = -np.rad2deg(np.arctan2(y, x))
        el = np.rad2deg(np.arcsin(z / r))
    return np.stack([r, az, el], axis=1)


def polar2cartesian(p: np.ndarray) -> np.ndarray:
    r, az, el = p[:, 0], -np.deg2rad(p[:, 1]), np.deg2rad(p[:, 2])
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1)


def in_fov(pol: np.ndarray, fov) -> np.ndarray:
    """inclusive bounds; fov = [[r_lo, r_hi], [az_lo, az_hi], [el_lo, el_hi]].  NaN fails every comparison."""
    with np.errstate(invalid="ignore"):
        return np.logical_and.reduce([pol[:, 0] >= fov[0][0], pol[:, 0] <= fov[0][1], pol[:, 1] >= fov[1][0],
                                      pol[:, 1] <= fov[1][1], pol[:, 2] >= fov[2][0], pol[:, 2] <= fov[2][1]])


def crop(xyz: np.ndarray, T: np.ndarray, fov):
    """The offline crop of one scan (float32 [N, >= 3]; x, y, z first).  -> (keep [N] bool, rows float32 [M, 3] in input order,
    polar float64 [N, 3]: the polar coordinates in the radar frame the filter saw, NaN rows for the points dropped as empty)."""
    f = np.asarray(xyz, dtype=np.float32)[:, :3]
    with np.errstate(all="ignore"):
        nonempty = np.sqrt(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2]) > 0      # float32; NaN > 0 is False
    nz = np.nonzero(nonempty)[0]
    h = np.hstack([f[nz], np.ones((len(nz), 1))])                                            # float64
    with np.errstate(all="ignore"):
        pol = cartesian2polar((h @ np.asarray(T, dtype=np.float64).T)[:, :3])
        m = in_fov(pol, fov)
        rows = polar2cartesian(pol[m]).astype(np.float32)
    keep = np.zeros(len(f), dtype=bool)
    keep[nz[m]] = True
    polar = np.full((len(f), 3), np.nan)
    polar[nz] = pol
    return keep, rows, polar


def bound_distance(polar: np.ndarray, fov) -> np.ndarray:
    """distance of each polar row to the nearest of the five FOV bounds a point can cross (NaN rows: inf)"""
    d = np.stack([polar[:, 0] - fov[0][1], polar[:, 1] - fov[1][0], polar[:, 1] - fov[1][1], polar[:, 2] - fov[2][0],
                  polar[:, 2] - fov[2][1]], axis=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.where(np.isnan(d).all(axis=1), np.inf, np.nanmin(np.abs(np.where(np.isnan(d), np.inf, d)), axis=1))


def polar_f32(p: np.ndarray) -> np.ndarray:
    """numpy's float32 cartesian2polar with the transcendentals correctly rounded (double, rounded once)"""
    p = np.asarray(p, dtype=np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = np.float32(180.0) / np.float32(np.pi)
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y + z * z)
        az = -(np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32) * c)
        el = np.arcsin((z / r).astype(np.float64)).astype(np.float32) * c
    return np.stack([r, az, el], axis=1)


# ---------------------------------------------------------------------------------------------------- voxels
def grid_of(pc_range, voxel_size) -> np.ndarray:
    r = np.asarray(pc_range, dtype=np.float64)
    return np.round((r[3:] - r[:3]) / np.asarray(voxel_size, dtype=np.float64)).astype(np.int64)


def passes(cells: int) -> int:
    """8-bit digits that hold every key 0 .. cells (cells itself is the key of a point outside the grid)"""
    n = 0
    while cells > 0:
        cells >>= 8
        n += 1
    return n


def cell_index(points: np.ndarray, voxel_size, pc_range):
    """float32 floor((p - lo) / v) per axis and the inside mask (0 <= c < grid; NaN is outside)"""
    pts = np.asarray(points, dtype=np.float32)
    lo = np.asarray(pc_range[:3], dtype=np.float32)
    v = np.asarray(voxel_size, dtype=np.float32)
    grid = grid_of(pc_range, voxel_size)
    with np.errstate(all="ignore"):
        c = np.floor((pts[:, :3] - lo) / v)                                    # float32 throughout
        inside = np.all((c >= 0) & (c < grid.astype(np.float32)), axis=1)
    return c, inside


def point_to_voxel(points, voxel_size, pc_range, F, max_points, max_voxels):
    """spconv's Point2VoxelCPU3d.point_to_voxel rules: voxels numbered in order of their first point; a new voxel beyond max_voxels
    is dropped while later points of kept voxels still count; each voxel keeps its first max_points points; coordinates z, y, x;
    the voxel tensor zero-filled.  -> (voxels [V, max_points, F] float32, coords [V, 3] int32, num_points [V] int32)."""
    pts = np.asarray(points, dtype=np.float32)
    F, maxp, maxv = int(F), int(max_points), int(max_voxels)
    assert pts.ndim == 2 and pts.shape[1] == F
    c, inside = cell_index(pts, voxel_size, pc_range)
    voxels, coords, num, ids = [], [], [], {}
    for i in np.nonzero(inside)[0]:
        key = (int(c[i, 2]), int(c[i, 1]), int(c[i, 0]))                      # z, y, x
        v = ids.get(key)
        if v is None:
            if len(ids) >= maxv:
                continue
            v = ids[key] = len(ids)
            coords.append(key)
            num.append(0)
            voxels.append(np.zeros((maxp, F), dtype=np.float32))
        if num[v] < maxp:
            voxels[v][num[v]] = pts[i]
            num[v] += 1
    V = len(ids)
    return (np.stack(voxels) if V else np.zeros((0, maxp, F), np.float32),
            np.array(coords, dtype=np.int32).reshape(V, 3), np.array(num, dtype=np.int32))


def linear_keys(coords_zyx: np.ndarray, grid) -> np.ndarray:
    c = np.asarray(coords_zyx, dtype=np.int64)
    return (c[:, 2] * int(grid[1]) + c[:, 1]) * int(grid[2]) + c[:, 0]


# ---------------------------------------------------------------------------------------------------- queries
def empty_cells(coords_xyz: np.ndarray, grid, ranks) -> np.ndarray:
    """x, y, z of nonzero(~occupied)[ranks] (row-major), from a dense boolean grid: get_empty_voxel_centers' rule.  The grid is
    allocated, so this is for grids of some 10^7 cells at the most."""
    g = tuple(int(v) for v in grid)
    occupied = np.zeros(g, dtype=bool)
    c = np.asarray(coords_xyz, dtype=np.int64).reshape(-1, 3)
    occupied[c[:, 0], c[:, 1], c[:, 2]] = True
    empty = np.nonzero(~occupied.reshape(-1))[0]
    sel = empty[np.asarray(ranks, dtype=np.int64)]
    return np.stack(np.unravel_index(sel, g), axis=1).astype(np.int64).reshape(-1, 3)


def norm_points(points: torch.Tensor, query_points, pc_range, aniso: bool, iso: bool) -> None:
    """The loader's norm_points, in place on float32 CPU tensors [N, 3]: Python scalars against the tensor columns (anisotropic), a
    float64 numpy offset array against the tensor slice (isotropic: float64 arithmetic, rounded on assignment)."""
    r = np.array(pc_range)
    x_offset, y_offset, z_offset = (r[3] + r[0]) / 2, (r[4] + r[1]) / 2, (r[5] + r[2]) / 2
    x_scale, y_scale, z_scale = (r[3] - r[0]) / 2, (r[4] - r[1]) / 2, (r[5] - r[2]) / 2
    both = [t for t in (points, query_points) if t is not None]
    if aniso:
        for t in both:
            t[:, 0] = (t[:, 0] - x_offset) / x_scale
            t[:, 1] = (t[:, 1] - y_offset) / y_scale
            t[:, 2] = (t[:, 2] - z_offset) / z_scale
    if iso:
        max_scale = max(x_scale, y_scale, z_scale)
        offset = np.array([x_offset, y_offset, z_offset])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)                # torch's __array_wrap__ under numpy 2
            for t in both:
                d = t[:, :3] - offset
                assert d.dtype == torch.float64                                # the promotion this restatement relies on
                t[:, :3] = d / max_scale


def queries(points, sample_idx, coords_zyx, voxel_idx, u_in, empty_xyz, u_out, voxel_size, pc_range, aniso, iso):
    """transform_voxels_to_query_points + norm_points for one frame.  points float32 [N, 3]; sample_idx [S]; coords_zyx [V, 3];
    voxel_idx [in_num] with u_in float64 [in_num, 3]; empty_xyz int [out_num, 3] (empty_cells) with u_out float64 [out_num, 3], or
    None.  -> (lidar_points [S, 3], query_points [S, 3], query_labels [S]) float32 numpy."""
    r = np.array(pc_range)
    vx, vy, vz = (float(v) for v in voxel_size)
    x_off, y_off, z_off = vx / 2 + r[0], vy / 2 + r[1], vz / 2 + r[2]
    lidar_points = torch.from_numpy(np.asarray(points, dtype=np.float32)[np.asarray(sample_idx, dtype=np.int64)][:, :3].copy())
    coords = torch.from_numpy(np.asarray(coords_zyx, dtype=np.int32).reshape(-1, 3).copy())[:, [2, 1, 0]]
    centre = torch.zeros((coords.shape[0], 3), dtype=torch.float32)
    centre[:, 0] = coords[:, 0].to(torch.float32) * vx + x_off
    centre[:, 1] = coords[:, 1].to(torch.float32) * vy + y_off
    centre[:, 2] = coords[:, 2].to(torch.float32) * vz + z_off
    vi = torch.from_numpy(np.asarray(voxel_idx, dtype=np.int64).reshape(-1).copy())
    q = centre[vi] + torch.from_numpy(np.asarray(u_in, dtype=np.float64).reshape(-1, 3).copy()).to(torch.float32)
    lab = torch.ones(q.shape[0])
    if empty_xyz is not None and len(empty_xyz):
        e = torch.from_numpy(np.asarray(empty_xyz, dtype=np.int64).reshape(-1, 3).copy())
        ec = torch.zeros((e.shape[0], 3), dtype=torch.float32)
        ec[:, 0] = e[:, 0] * vx + x_off
        ec[:, 1] = e[:, 1] * vy + y_off
        ec[:, 2] = e[:, 2] * vz + z_off
        q = torch.cat([q, ec + torch.from_numpy(np.asarray(u_out, dtype=np.float64).reshape(-1, 3).copy()).to(torch.float32)], dim=0)
        lab = torch.cat([lab, torch.zeros(e.shape[0])], dim=0)
    norm_points(lidar_points, q, pc_range, aniso, iso)
    return lidar_points.numpy(), q.numpy(), lab.numpy()


def replay_item(points, cfg: dict, loader: str, rng: np.random.Generator):
    """One __getitem__ on float32 points [N, F] (polar rows in view-cone mode) with the draws of the loader in its order: numpy's from
    `rng`, the empty-cell ranks from torch's global CPU generator.  -> (lidar_points, query_points, query_labels, in_num)."""
    pts = np.asarray(points, dtype=np.float32)
    S = int(cfg["num_samples"])
    vsize = np.array(cfg["voxel_size"])
    grid = grid_of(cfg["pc_range"], cfg["voxel_size"])
    _, coords, _ = point_to_voxel(pts, cfg["voxel_size"], cfg["pc_range"], cfg["num_point_features"], cfg["max_points_per_voxel"],
                                  cfg["max_number_of_voxels"])
    V = len(coords)
    sidx = rng.choice(len(pts), S, replace=False)
    in_ratio = int(S * cfg["query_ratio"])
    if loader == "train":
        in_num, out_num = in_ratio, S - in_ratio
        u_in = rng.uniform(low=-vsize / 2, high=vsize / 2, size=(in_num, 3))
        u_out = rng.uniform(low=-vsize / 2, high=vsize / 2, size=(out_num, 3))
        vidx = rng.choice(V, in_num, replace=True)
        ranks = torch.randint(0, int(np.prod(grid)) - V, (out_num,)).numpy()
        empty = empty_cells(coords[:, ::-1], grid, ranks)
    else:
        u_in = rng.uniform(low=-vsize / 2, high=vsize / 2, size=(S, 3))
        vidx = rng.choice(V, S, replace=True)
        empty = u_out = None
    lp, qp, lab = queries(pts, sidx, coords, vidx, u_in, empty, u_out, cfg["voxel_size"], cfg["pc_range"],
                          bool(cfg.get("norm_anisotropy", False)), bool(cfg.get("norm_isotropy", False)))
    return lp, qp, lab, in_ratio
