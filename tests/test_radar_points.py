"""Helper points on the device (rald_amd.radar_points, rald_amd/csrc/radar_points.hip) against the reference's
cache_test_cfar.py chain (tests/golden/make_golden_radar_points.py -> g22_radar_points.npz).  The ADC frames behind the stored
cubes are regenerated from the generator's seed with rald_amd.synth.radar_adc."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

SEED, FRAMES = 2201, 2
NEAR_INT = 1e-2        # a slice whose reference pre-floor value lies this close to an integer may get one point more or less
TIE_REL = 1e-6         # a voxel this close (relative) to its slice's k-th value may be swapped for another one


@pytest.fixture(scope="module")
def g22():
    with np.load(os.path.join(GOLDEN, "g22_radar_points.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _cfg(g22, dims=None, num=None):
    from rald_amd.radar_dsp import RadarConfig
    d = [int(v) for v in g22["dims"]]
    cfg = RadarConfig(max_range=float(g22["max_range"]), angles_DOA_az=g22["fov_az"].tolist(), angles_DOA_ele=g22["fov_el"].tolist(),
                      input_r_size=d[0], input_a_size=d[1], input_e_size=d[2], target_r_size=d[3], target_a_size=d[4], target_e_size=d[5],
                      cfar_num_point=int(float(str(g22["num_point_str"]))))
    if dims is not None:
        cfg.target_r_size, cfg.target_a_size, cfg.target_e_size = (int(v) for v in dims)
    if num is not None:
        cfg.cfar_num_point = int(num)
    cfg.fov = [[0, cfg.max_range], cfg.angles_DOA_az, cfg.angles_DOA_ele]
    return cfg


def _write_yamls(g22, tmp_path):
    with open(tmp_path / "radar.yml", "w") as f:
        for k, v in zip(g22["radar_keys"], g22["radar_cfg"]):
            f.write(f"{k}: {int(v)}\n" if float(v).is_integer() and abs(v) < 1e6 else f"{k}: {float(v):.17e}\n")
        f.write(f"angles_DOA_az: [{', '.join(str(int(v)) for v in g22['fov_az'])}]\n")
        f.write(f"angles_DOA_ele: [{', '.join(str(int(v)) for v in g22['fov_el'])}]\n")
    d = [int(v) for v in g22["dims"]]
    with open(tmp_path / "dataset.yaml", "w") as f:
        f.write("single_chip_mode:\n  radar:\n    cfar:\n")
        for k, v in zip(["input_r_dim", "input_a_dim", "input_e_dim", "tgt_r_dim", "tgt_a_dim", "tgt_e_dim"], d):
            f.write(f"      {k}: {v}\n")
        f.write(f"      cfar_num_point: {str(g22['num_point_str'])}\n")
    return tmp_path / "dataset.yaml", tmp_path / "radar.yml"


# ---- CPU ----------------------------------------------------------------------------------------
def test_load_cfar_config_matches_fixture(g22, tmp_path):
    from rald_amd import radar_points as RP
    ds, radar = _write_yamls(g22, tmp_path)
    cfg = RP.load_cfar_config(ds, radar)
    want = _cfg(g22)
    assert cfg.max_range == want.max_range
    assert isinstance(cfg.cfar_num_point, int) and cfg.cfar_num_point == 800000
    for k in ("input_r_size", "input_a_size", "input_e_size", "target_r_size", "target_a_size", "target_e_size"):
        assert cfg[k] == want[k], k
    assert cfg.fov == [[0, want.max_range], want.angles_DOA_az, want.angles_DOA_ele]


def test_coordinate_axes_and_keep_masks_match_reference_bit_for_bit(g22):
    from rald_amd import radar_points as RP
    cfg = _cfg(g22)
    axes, masks = RP.coordinate_axes(cfg), RP.keep_masks(cfg)
    for name, t, m in zip("rae", axes, masks):
        assert t.dtype == np.float64
        np.testing.assert_array_equal(t.astype(np.float32), g22[f"axis_{name}"])
        np.testing.assert_array_equal(m, g22[f"keep_{name}"])
        assert all(np.diff(t.astype(np.float32)) > 0)          # strictly increasing: a coordinate maps back to one index
    assert masks[2].sum() == 44 and masks[0].all() and masks[1].all()


@pytest.mark.parametrize("change, msg", [
    ({"input_a_size": 0}, "must be positive"),
    ({"target_e_size": -1}, "must be positive"),
    ({"target_a_size": 512}, "exceeds 32768"),
    ({"cfar_num_point": 0}, "num_points = 0"),
    ({"cfar_num_point": 256 * 256 * 128 + 1}, "must be in [1, 8388608]"),
])
def test_unsupported_configs_raise_at_creation(g22, change, msg):
    from rald_amd import radar_points as RP
    cfg = _cfg(g22)
    cfg.update(change)
    axes = [np.zeros(1024)] * 3
    masks = [np.ones(1024, bool)] * 3
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        RP.RadarPoints(cfg, 1, axes=axes, masks=masks)
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        RP.workspace_bytes(cfg, 1)


def test_null_tables_and_short_tables_are_rejected(g22):
    from rald_amd import radar_points as RP
    cfg = _cfg(g22)
    h = C.c_void_p()
    rc = RP.lib().rald_radar_points_create(C.byref(RP.points_config(cfg)), None, None, None, None, None, None, C.byref(h))
    assert rc != 0 and "axis tables and keep masks" in RP.lib().rald_last_error().decode()
    with pytest.raises(ValueError, match="tgt_e"):
        RP.RadarPoints(cfg, 1, axes=[np.zeros(256), np.zeros(256), np.zeros(127)])


def test_workspace_query_is_host_arithmetic(g22):
    from rald_amd import radar_points as RP
    cfg = _cfg(g22)
    r256 = lambda v: (v + 255) // 256 * 256
    for B in (1, 8, 64):
        # sums (double), counts, offsets, kept counts, buffer choice per slice; a status per frame; two 16-bit index buffers
        assert RP.workspace_bytes(cfg, B) == r256(B * 256 * 8) + 4 * r256(B * 256 * 4) + r256(B * 4) + 2 * r256(B * 800000 * 2)
    assert RP.lib().rald_radar_points_workspace_bytes(C.byref(RP.points_config(cfg)), 0) == -1


# ---- GPU ----------------------------------------------------------------------------------------
def _upsample(cube, dims):
    return F.interpolate(torch.from_numpy(np.ascontiguousarray(cube))[:, None], size=tuple(int(v) for v in dims), mode="trilinear",
                         align_corners=False)[:, 0].numpy()


def _check_frame(up, peaks, inten, points, count, cfg, ref_counts, ref_pre, ref_sel=None):
    """One frame's device output against the CPU-upsampled cube `up` [R, A, E] and the reference's allocation / selection.
    Returns (selection mismatches, mismatches that are not near-ties) for the caller to print and bound."""
    from rald_amd import radar_points as RP
    R, A, E = up.shape
    num = int(cfg.cfar_num_point)
    assert peaks.shape == (num, 3) and inten.shape == (num,)
    r, a, e = peaks[:, 0], peaks[:, 1], peaks[:, 2]
    assert (np.diff(r) >= 0).all() and r.min() >= 0 and r.max() < R and a.min() >= 0 and a.max() < A and e.min() >= 0 and e.max() < E
    # counts: the reference's, except by one where its fp32 pre-floor value is near an integer
    counts = np.bincount(r, minlength=R)
    assert counts.sum() == num
    near = np.abs(ref_pre - np.round(ref_pre)) < NEAR_INT
    diff = counts - ref_counts
    assert (diff[~near] == 0).all(), np.nonzero(diff[~near])
    assert (np.abs(diff) <= 1).all()
    # intensities: the interpolated value at each peak
    want = up[r, a, e]
    rel = np.abs(inten - want) / np.maximum(np.abs(want), 1e-30)
    assert rel.max() <= 1e-6, rel.max()
    # order: value descending within a slice, equal values by flat index ascending
    flat = a.astype(np.int64) * E + e
    same = r[1:] == r[:-1]
    assert (inten[1:][same] <= inten[:-1][same]).all()
    eq = same & (inten[1:] == inten[:-1])
    assert (flat[1:][eq] > flat[:-1][eq]).all()
    # selection: within each slice with the reference's count, the same voxels except near the k-th value
    got = np.zeros((R, A * E), bool)
    got[r, flat] = True
    mism = robust = 0
    if ref_sel is not None:
        upf = up.reshape(R, A * E)
        for s in np.nonzero((diff == 0) & (counts > 0))[0]:
            d = np.nonzero(got[s] != ref_sel[s])[0]
            if len(d):
                vk = np.sort(upf[s])[::-1][counts[s] - 1]
                mism += len(d)
                robust += int((np.abs(upf[s, d] - vk) > TIE_REL * abs(vk)).sum())
    # points: the float32 table lookup of the kept peaks, compacted in order
    ax = [t.astype(np.float32) for t in RP.coordinate_axes(cfg)]
    km = RP.keep_masks(cfg)
    keep = km[0][r] & km[1][a] & km[2][e]
    assert count == keep.sum()
    np.testing.assert_array_equal(points[:count], np.stack([ax[0][r], ax[1][a], ax[2][e]], 1)[keep])
    return mism, robust


def _ref_peaks(g22, tag):
    """the reference's peaks [N, 3] (r, a, e) in its order, from the stored flat indices and slice counts"""
    E = int(g22[f"{tag}_dims"][2])
    flat = g22[f"{tag}_flat"].astype(np.int64)
    r = np.repeat(np.arange(len(g22[f"{tag}_counts"])), g22[f"{tag}_counts"])
    return np.stack([r, flat // E, flat % E], 1)


def _unpack(g22, b, dims):
    return np.unpackbits(g22["selected"][b])[:int(np.prod(dims))].astype(bool).reshape(int(dims[0]), -1)


@pytest.mark.gpu
def test_shipped_config_matches_reference(g22):
    """Shipped config (256 x 256 x 128, 8e5 points) on the reference's cubes."""
    from rald_amd import radar_points as RP
    cfg = _cfg(g22)
    h = RP.RadarPoints(cfg, 1)
    points, counts, peaks, inten = h.points_padded(torch.from_numpy(g22["cube"]).cuda(), with_peaks=True)
    points, counts, peaks, inten = points.cpu().numpy(), counts.cpu().numpy(), peaks.cpu().numpy(), inten.cpu().numpy()
    up = _upsample(g22["cube"], g22["dims"][3:])
    for b in range(FRAMES):
        mism, robust = _check_frame(up[b], peaks[b], inten[b], points[b], int(counts[b]), cfg, g22["counts"][b], g22["prefloor"][b],
                                    _unpack(g22, b, g22["dims"][3:]))
        print(f"frame {b}: kept {counts[b]} (reference {g22['kept'][b]}), selection mismatches {mism} ({robust} not near a tie)")
        assert robust == 0


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["p2", "nd"])
def test_reduced_configs_match_reference(g22, tag):
    """Reduced configs on frame 0 against the reference's full peaks, intensities (its F.interpolate values at its peaks) and
    filtered points."""
    from rald_amd import radar_points as RP
    dims, num = g22[f"{tag}_dims"], int(g22[f"{tag}_num"])
    cfg = _cfg(g22, dims, num)
    h = RP.RadarPoints(cfg, 1)
    points, counts, peaks, inten = (t.cpu().numpy() for t in h.points_padded(torch.from_numpy(g22["cube"][:1]).cuda(), with_peaks=True))
    up = _upsample(g22["cube"][:1], dims)[0]
    rp = _ref_peaks(g22, tag)
    ref_sel = np.zeros((int(dims[0]), int(dims[1] * dims[2])), bool)
    ref_sel[rp[:, 0], rp[:, 1] * int(dims[2]) + rp[:, 2]] = True
    mism, robust = _check_frame(up, peaks[0], inten[0], points[0], int(counts[0]), cfg, g22[f"{tag}_counts"], g22[f"{tag}_prefloor"], ref_sel)
    print(f"{tag}: kept {counts[0]} (reference {len(g22[f'{tag}_points'])}), selection mismatches {mism} ({robust} not near a tie)")
    assert robust == 0
    if mism == 0 and (np.bincount(peaks[0][:, 0], minlength=int(dims[0])) == g22[f"{tag}_counts"]).all():
        # same voxels: the reference's intensities in its order equal ours up to the order inside tie runs, and its points too
        ri = up[rp[:, 0], rp[:, 1], rp[:, 2]]
        rel = np.abs(np.sort(inten[0]) - np.sort(ri)) / np.maximum(np.abs(np.sort(ri)), 1e-30)
        assert rel.max() <= 1e-6
        assert (rp[:, 0] == peaks[0][:, 0]).all()
        n = int(counts[0])
        assert n == len(g22[f"{tag}_points"])
        key = lambda p: p[np.lexsort(p.T[::-1])]
        np.testing.assert_array_equal(key(points[0][:n]), key(g22[f"{tag}_points"]))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["p2", "nd"])
def test_dropin_ra2d_detector_tensor(g22, tag):
    """RA2DDetectorTensor(up, num) with the reference's signature on the reference's upsampled cube: scale 1, so the intensities
    are input values and, with the same voxels chosen, equal the reference's exactly in its order."""
    from rald_amd import radar_points as RP
    dims, num = g22[f"{tag}_dims"], int(g22[f"{tag}_num"])
    up = torch.from_numpy(_upsample(g22["cube"][:1], dims))
    peaks, inten = RP.RA2DDetectorTensor(up, num=num)
    assert peaks.dtype == torch.int32 and peaks.shape == (num, 3) and inten.shape == (num,) and not peaks.is_cuda
    pk, iv = peaks.numpy().astype(np.int64), inten.numpy()
    np.testing.assert_array_equal(iv, up[0].numpy()[pk[:, 0], pk[:, 1], pk[:, 2]])
    counts = np.bincount(pk[:, 0], minlength=int(dims[0]))
    pre = g22[f"{tag}_prefloor"]
    near = np.abs(pre - np.round(pre)) < NEAR_INT
    assert (counts[~near] == g22[f"{tag}_counts"][~near]).all()
    if (counts == g22[f"{tag}_counts"]).all():
        rp = _ref_peaks(g22, tag)
        np.testing.assert_array_equal(iv, up[0].numpy()[rp[:, 0], rp[:, 1], rp[:, 2]])
    two = RP.RA2DDetectorTensor(torch.cat([up, up]), num=num)
    assert two[0].shape == (2, num, 3) and torch.equal(two[0][1], peaks) and torch.equal(two[1][0], inten)


def _valid(points, counts, peaks, inten, b):
    n = int(counts[b])
    return points[b, :n], peaks[b], inten[b]


@pytest.mark.gpu
def test_batch_invariance_and_determinism(g22):
    from rald_amd import radar_points as RP
    h = RP.RadarPoints(_cfg(g22), 1)
    cube = torch.from_numpy(g22["cube"])
    batch = torch.cat([cube, cube.flip(2) * 0.5, cube[:1] * 2.0]).cuda()
    out1 = [t.cpu() for t in h.points_padded(batch, with_peaks=True)]
    out2 = [t.cpu() for t in h.points_padded(batch, with_peaks=True)]
    assert torch.equal(out1[1], out2[1])
    for b in range(5):
        for x, y in zip(_valid(*out1, b), _valid(*out2, b)):
            assert torch.equal(x, y)
        alone = [t.cpu() for t in h.points_padded(batch[b], with_peaks=True)]
        assert int(alone[1][0]) == int(out1[1][b])
        for x, y in zip(_valid(*alone, 0), _valid(*out1, b)):
            assert torch.equal(x, y)


@pytest.mark.gpu
def test_rejected_frames_raise_and_the_others_are_written(g22):
    from rald_amd import radar_points as RP
    cfg = _cfg(g22)
    h = RP.RadarPoints(cfg, 1)
    cube = torch.from_numpy(g22["cube"]).cuda()
    batch = torch.stack([cube[0], torch.zeros_like(cube[0]), cube[1]])
    with pytest.raises(ValueError, match="frame 1"):                    # the reference: 0/0 weights, then np.argpartition raises
        h.points(batch)
    points, counts, _, _ = h.run(batch, check_frames=False)
    ref = h.points_padded(cube[:2])
    assert counts.cpu().tolist() == [int(ref[1][0]), -1, int(ref[1][1])]
    assert torch.equal(points[0, :counts[0]], ref[0][0, :ref[1][0]]) and torch.equal(points[2, :counts[2]], ref[0][1, :ref[1][1]])
    # passes create, but the largest slice (2.4 % of 3e4 = ~725 points) has only 16 * 8 = 128 voxels: the reference's assert
    small = RP.RadarPoints(_cfg(g22, (256, 16, 8), 30000), 1)
    with pytest.raises(AssertionError, match="frame 0"):
        small.points(cube[:1])
    _, counts, _, _ = small.run(torch.stack([cube[0], torch.zeros_like(cube[0])]), check_frames=False)
    assert counts.cpu().tolist() == [-2, -1]


def _ref_tie_rule(x, num):
    """this project's contract on an identity-scale cube x [R, A, E]: allocation in double, the k largest per slice, ties by lowest
    flat index, output by value descending then flat index ascending"""
    R, A, E = x.shape
    xf = np.where(x == 0, 0.0, x).reshape(R, -1).astype(np.float64)
    s = xf.sum(1)
    c = np.floor(s / s.sum() * num).astype(np.int64)
    c[int(np.argmax(s))] += num - c.sum()
    peaks, vals = [], []
    for r in range(R):
        order = np.lexsort((np.arange(A * E), -xf[r]))[:c[r]]
        peaks.append(np.stack([np.full(c[r], r), order // E, order % E], 1))
        vals.append(x.reshape(R, -1)[r, order])
    return np.concatenate(peaks), np.concatenate(vals)


@pytest.mark.gpu
def test_tie_rule_on_planted_equal_values():
    from rald_amd import radar_points as RP
    from rald_amd.radar_dsp import RadarConfig
    rng = np.random.default_rng(2202)
    R, A, E, num = 6, 48, 20, 2000
    x = rng.choice(np.array([-0.0, 0.0, 1.0, 2.0, 2.5, 3.0], np.float32), size=(R, A, E)).astype(np.float32)
    x[2] = 1.0                                           # a slice of one value: every pick is a tie
    x[4, :, ::2] = -0.0
    peaks, inten = RP.RA2DDetectorTensor(torch.from_numpy(x)[None], num=num)
    want_p, want_v = _ref_tie_rule(x, num)
    np.testing.assert_array_equal(peaks.numpy(), want_p)
    np.testing.assert_array_equal(np.abs(inten.numpy()), np.abs(want_v))
    # the same cube through the handle (float32 tables, no filter): the points are the peaks' coordinates in the same order
    cfg = RadarConfig(input_r_size=R, input_a_size=A, input_e_size=E, target_r_size=R, target_a_size=A, target_e_size=E, cfar_num_point=num)
    axes = [np.arange(R) * 1.0, np.arange(A) * 10.0, np.arange(E) * 100.0]
    h = RP.RadarPoints(cfg, 1, axes=axes, masks=[np.ones(R, bool), np.arange(A) % 3 > 0, np.ones(E, bool)])
    pts = h.points(torch.from_numpy(x).cuda())[0].cpu().numpy()
    keep = want_p[:, 1] % 3 > 0
    np.testing.assert_array_equal(pts, (want_p * np.array([1.0, 10.0, 100.0]))[keep].astype(np.float32))


def _dsp_32x16():
    from rald_amd import radar_dsp as RD
    with np.load(os.path.join(GOLDEN, "g21_radar_dsp.npz"), allow_pickle=False) as f:
        g21 = {k: f[k] for k in ("cfg_keys", "c32x16_cfg", "tx", "rx")}
    cfg = RD.RadarConfig({k: (int(v) if float(v).is_integer() and k.startswith(("num", "range", "doppler", "ANGLE", "ELEVATION"))
                              else float(v)) for k, v in zip(g21["cfg_keys"], g21["c32x16_cfg"])})
    return RD.RadarDSP(cfg, g21["tx"], g21["rx"])


@pytest.mark.gpu
def test_adc_to_helper_points_chain(g22):
    """ADC (regenerated) -> RadarDSP (32 x 16) -> RadarPoints against the reference's chain.  The device cube differs from the
    reference's by up to ~1e-4 dB, so slice counts may move by one and near-equal voxels may swap.  Measured on an MI355X: counts
    equal, selection Jaccard 0.99997, kept points equal but one on frame 0."""
    from rald_amd import radar_points as RP, synth
    cfg = _cfg(g22)
    dsp, pts = _dsp_32x16(), RP.RadarPoints(cfg, 3)
    frames = synth.radar_adc(FRAMES, SEED).cuda()
    out = RP.helper_points_from_adc(frames, dsp, pts)
    assert len(out) == FRAMES and all(p.is_cuda and p.dtype == torch.float32 for p in out)
    points, counts, peaks, _ = pts.points_padded(dsp.cubes(frames), with_peaks=True)
    dims = g22["dims"][3:]
    for b in range(FRAMES):
        assert torch.equal(out[b], points[b, :counts[b]])
        pk = peaks[b].cpu().numpy().astype(np.int64)
        c = np.bincount(pk[:, 0], minlength=int(dims[0]))
        assert np.abs(c - g22["counts"][b]).max() <= 1
        got = np.zeros((int(dims[0]), int(dims[1] * dims[2])), bool)
        got[pk[:, 0], pk[:, 1] * int(dims[2]) + pk[:, 2]] = True
        ref = _unpack(g22, b, dims)
        jac = (got & ref).sum() / (got | ref).sum()
        print(f"chain frame {b}: selection Jaccard {jac:.5f}, kept {int(counts[b])} (reference {g22['kept'][b]})")
        assert jac >= 0.9999           # measured on an MI355X: 0.99997


@pytest.mark.gpu
def test_process_cube_files_writes_save_lidar_data_bytes(g22, tmp_path):
    """RAEIVV cube files named like the reference's (stem ..._<frame>) -> {i:04d}.bin in the reference's sorted order, each the
    float32 bytes of that frame's valid rows."""
    from rald_amd import radar_points as RP
    cfg = _cfg(g22)
    rng = np.random.default_rng(5)
    cube = np.ascontiguousarray(np.concatenate([g22["cube"], g22["cube"][:1, :, ::-1] * 0.5]))     # three frames
    names = ["radar_10.bin", "radar_2.bin", "radar_1.bin"]            # frames 2, 1, 0 once sorted by the trailing integer
    for name, b in zip(names, (2, 1, 0)):
        raeivv = np.stack([cube[b], rng.normal(size=cube[b].shape).astype(np.float32), np.ones_like(cube[b])], -1)
        raeivv.astype(np.float32).tofile(tmp_path / name)
    paths = RP.sorted_cube_files(tmp_path / n for n in names)
    assert [p.name for p in paths] == ["radar_1.bin", "radar_2.bin", "radar_10.bin"]
    assert RP.process_cube_files(paths, tmp_path / "out", cfg, batch=2) == 3
    points, counts = RP.RadarPoints(cfg, 1).points_padded(torch.from_numpy(cube).cuda())
    for i, b in enumerate((0, 1, 2)):
        got = (tmp_path / "out" / f"{i:04d}.bin").read_bytes()
        assert got == points[b, :counts[b]].cpu().numpy().tobytes()
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["0000.bin", "0001.bin", "0002.bin"]
