"""Voxel-grid down-sampling on the GPU (rald_amd/csrc/voxel_reduce.hip) against tests/voxel_ref.py, by equality: integers as integers,
floats by bit pattern.  Every call goes through _run: the outputs are pre-filled with poison and followed by guard rows, the input
rows the kernels must not read (behind counts, behind the bound, behind offsets[B]) are NaN, and _check asserts that everything the
definition does not write still holds its poison."""
import ctypes as C

import numpy as np
import pytest
import torch

import voxel_ref as REF

gpu = pytest.mark.gpu
F32 = np.float32
GUARD = 64
POISON_F = np.array([0x7FC12345], np.uint32).view(F32)[0]          # a NaN with a payload: compared by bits
POISON_I = -777


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _grid(lo, hi, voxel):
    from rald_amd.postprocess import voxel_grid
    return voxel_grid(lo, hi, voxel)


def _run(points, offsets, grid, bound, counts=None, chunk=0, post=False):
    """The C entry on poisoned, guarded buffers -> dict of numpy arrays, whole buffers (guards included)."""
    from rald_amd._handles import _stream
    from rald_amd._lib import check, lib
    p = np.array(points, F32).reshape(-1, 3)
    T, B = len(p), len(offsets) - 1
    hidden = np.ones(T + GUARD, bool)
    for b in range(B):
        n = offsets[b + 1] - offsets[b]
        if counts is not None:
            n = min(n, max(int(counts[b]), 0))
        hidden[offsets[b]:offsets[b] + max(min(n, bound), 0)] = False
    dev_p = np.concatenate([p, np.zeros((GUARD, 3), F32)])
    dev_p[hidden] = np.nan
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = dict(points=cu(dev_p), offsets=cu(np.array(offsets, np.int64)), counts=None if counts is None else cu(np.array(counts, np.int32)),
             out=cu(np.full((T + GUARD, 3), POISON_F, F32)), out_offsets=cu(np.full(B + 1 + GUARD, POISON_I, np.int64)),
             count=cu(np.full(T + GUARD, POISON_I, np.int32)), first=cu(np.full(T + GUARD, POISON_I, np.int64)),
             cells=cu(np.full((T + GUARD, 3), POISON_I, np.int32)), inverse=cu(np.full(T + GUARD, POISON_I, np.int64)))
    L = lib()
    nbytes = L.rald_post_voxel_scratch_bytes(B, T, bound) if post else L.rald_op_voxel_scratch_bytes(B, T, bound, chunk)
    assert nbytes > 0
    scratch = torch.empty(nbytes + 16 * GUARD, dtype=torch.uint8, device="cuda")
    scratch[nbytes:] = 0xA5
    lo3, v3, dims3 = (C.c_float * 3)(*grid[0]), (C.c_float * 3)(*grid[1]), (C.c_int32 * 3)(*grid[2])
    ptr = lambda k: None if t[k] is None else t[k].data_ptr()
    head = (ptr("points"), ptr("offsets"), ptr("counts"), B, 0, T, bound, lo3, v3, dims3, ptr("out"), ptr("out_offsets"), ptr("count"),
            ptr("first"), ptr("cells"), ptr("inverse"), scratch.data_ptr(), nbytes)
    if post:
        check(L.rald_post_voxel_downsample_ragged(*head, _stream()))
    else:
        check(L.rald_op_voxel_downsample_ragged(*head, chunk, _stream()))
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "the scratch's guard was written"
    return {k: t[k].cpu().numpy() for k in ("out", "out_offsets", "count", "first", "cells", "inverse")}


def _check(got, ref, B):
    """Everything the definition writes equals the reference; everything else still holds its poison."""
    M = int(ref["offsets"][-1])
    assert got["out_offsets"][:B + 1].tolist() == ref["offsets"].tolist()
    assert (got["out_offsets"][B + 1:] == POISON_I).all()
    assert np.array_equal(got["count"][:M], ref["count"]) and (got["count"][M:] == POISON_I).all()
    assert np.array_equal(got["first"][:M], ref["first"]) and (got["first"][M:] == POISON_I).all()
    assert np.array_equal(got["cells"][:M], ref["cells"]) and (got["cells"][M:] == POISON_I).all()
    T = len(ref["inverse"])
    want_inv = np.where(ref["untouched"], POISON_I, ref["inverse"])
    assert np.array_equal(got["inverse"][:T], want_inv) and (got["inverse"][T:] == POISON_I).all()
    diff = np.nonzero((_bits(got["out"][:M]) != _bits(ref["points"])).any(axis=1))[0]
    assert diff.size == 0, (diff[:5], got["out"][diff[:5]], ref["points"][diff[:5]])
    assert (_bits(got["out"][M:]) == _bits(POISON_F)).all()


def _offsets(lengths):
    return [0] + np.cumsum(lengths).tolist()


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == F32 else a[k], b[k].view(np.uint32) if b[k].dtype == F32 else b[k]) for k in a)


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4099, 70000]
_SIZES = {}


def _sizes():
    """The ragged batch of test 1 (rows uniform in [-10.6, 10.6)^3, so a few per cent lie outside the grid of 21^3 cells of edge 1),
    its grid and its reference; built once."""
    if not _SIZES:
        off = _offsets(LENGTHS)
        p = np.random.RandomState(5).uniform(-10.6, 10.6, size=(off[-1], 3)).astype(F32)
        grid = _grid((-10,) * 3, (10,) * 3, 1.0)
        _SIZES.update(p=p, off=off, grid=grid, ref=REF.voxel_ragged(p, off, *grid, max(LENGTHS)))
    return _SIZES


@gpu
@pytest.mark.parametrize("chunk", [0, 1024, 2048, 4096])
def test_sizes_in_one_ragged_batch(chunk):
    """Clouds of 0 .. 70 000 rows around the wave (64), the key block (256), the segment block and smallest chunk (1024) and the
    largest automatic chunk (4096, what chunk 0 picks for this batch) in one batch; the 70 000-row cloud spans 69 / 35 / 18 chunks."""
    s = _sizes()
    assert s["grid"][2] == (21, 21, 21) and 0 < (s["ref"]["inverse"] == -1).sum() < 0.3 * len(s["p"])
    assert [-(-70000 // c) for c in (1024, 2048, 4096)] == [69, 35, 18]
    _check(_run(s["p"], s["off"], s["grid"], max(LENGTHS), chunk=chunk), s["ref"], len(LENGTHS))


@gpu
def test_sizes_each_cloud_alone():
    """Every cloud of the batch alone, its length as the bound (the one-workgroup sort up to 4099 rows, chunks of 4096 for the 70 000):
    the batch's result, cloud for cloud, and through the rald_post_ entry as well."""
    s = _sizes()
    ref, off = s["ref"], s["off"]
    for b, n in enumerate(LENGTHS):
        lo, hi = int(ref["offsets"][b]), int(ref["offsets"][b + 1])
        one = dict(points=ref["points"][lo:hi], offsets=np.array([0, hi - lo]), count=ref["count"][lo:hi], first=ref["first"][lo:hi],
                   cells=ref["cells"][lo:hi], inverse=ref["inverse"][off[b]:off[b + 1]], untouched=ref["untouched"][off[b]:off[b + 1]])
        _check(_run(s["p"][off[b]:off[b + 1]], [0, n], s["grid"], max(n, 1), post=(b % 2 == 0)), one, 1)


@gpu
def test_automatic_rule_boundaries():
    """The bounds at which chunk 0 changes its route (one workgroup up to 8192 rows; up to 16384 from 64 clouds; up to 65536 from 256
    clouds; chunks of 2048 up to 8 clouds and 65536 rows, of 4096 beyond): the bound picks the route, so short clouds reach every one;
    the 8193-row cloud is cut by the bound 8192 and spans five chunks of 2048 at 8193."""
    s = _sizes()
    p = s["p"][-8193:]
    for bound in (8192, 8193):
        _check(_run(p, [0, 8193], s["grid"], bound), REF.voxel_ragged(p, [0, 8193], *s["grid"], bound), 1)
    for B, bounds in ((8, (65536, 65537)), (9, (65536,)), (64, (16384, 16385)), (256, (65536, 65537))):
        lengths = [(37 * b) % 301 for b in range(B)]
        lengths[B // 2] = 2500
        off = _offsets(lengths)
        q = s["p"][-off[-1]:]
        ref = REF.voxel_ragged(q, off, *s["grid"], 2500)
        for bound in bounds:
            _check(_run(q, off, s["grid"], bound), ref, B)


# ---- 2. grids and pass counts ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims,want_passes", [((3, 5, 17), 1), ((4, 8, 8), 2), ((15, 17, 257), 2), ((16, 64, 64), 3), ((255, 273, 241), 3),
                                              ((256, 256, 256), 4), ((1290, 1290, 1290), 4)])
def test_grids_and_pass_counts(dims, want_passes):
    """cells = 255, 256, 65 535, 65 536, 2^24 - 1, 2^24 and 1290^3: 1, 2, 2, 3, 3, 4, 4 radix passes.  Cell 0 and the last cell are
    occupied (and keys above 2^30 in the largest grid); the 100 outside rows carry the key `cells`, alone in the top digit where cells
    is a power of 256.  3000 rows: three chunks of 1024, and the one-workgroup route."""
    from rald_amd._lib import lib
    cells = dims[0] * dims[1] * dims[2]
    assert cells in (255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 1290 ** 3)
    assert lib().rald_op_voxel_passes(cells) == want_passes == REF.passes(cells)
    rs = np.random.RandomState(cells % 1000)
    c = np.stack([rs.randint(0, d, size=1500) for d in dims], axis=1)
    c[0], c[1] = 0, np.array(dims) - 1
    c[2:40, 0] = dims[0] - 1 - rs.randint(0, max(dims[0] // 3, 1), size=38)           # the top third of the keys
    p = np.concatenate([c + 0.5, c[rs.randint(0, 1500, size=1400)] + 0.25, np.full((100, 3), -1.0)]).astype(F32)
    p = p[rs.permutation(len(p))]
    grid = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims)
    ref = REF.voxel_ragged(p, [0, 3000], *grid, 3000)
    keys = (ref["cells"][:, 0].astype(np.int64) * dims[1] + ref["cells"][:, 1]) * dims[2] + ref["cells"][:, 2]
    assert keys[0] == 0 and keys[-1] == cells - 1 and (ref["inverse"] == -1).sum() == 100
    if cells == 1290 ** 3:
        assert (keys > 2 ** 30).sum() > 30
    for chunk in (1024, 4096):
        _check(_run(p, [0, 3000], grid, 3000, chunk=chunk), ref, 1)


# ---- 3. contents -----------------------------------------------------------------------------------------------------------------------------
def _content(name):
    rs = np.random.RandomState(11)
    if name == "one_cell":                                            # 3000 rows in one cell: one lane walks them all
        return rs.uniform(2.0, 3.0, size=(3000, 3)).astype(F32)
    if name == "distinct":                                            # 3000 distinct cells, rows in descending key order
        k = rs.permutation(21 ** 3)[:3000]
        k = np.sort(k)[::-1]
        return (np.stack([k // 441, k // 21 % 21, k % 21], axis=1) - 10 + 0.5).astype(F32)
    if name == "every_second_outside":
        p = rs.uniform(-10, 10, size=(3000, 3)).astype(F32)
        p[::2, rs.randint(0, 3)] = 50.0
        return p
    if name == "all_outside":
        return rs.uniform(20, 30, size=(3000, 3)).astype(F32)
    if name == "duplicates":                                          # 10 distinct rows, 300 copies each
        return np.tile(rs.uniform(-10, 10, size=(10, 3)).astype(F32), (300, 1))
    assert name == "order"                                            # a cell next to 0 with 1e-30, 0.04 and 0.049 in both orders
    return np.array([[1e-30, 0.5, 0.5], [0.04, 0.5, 0.5], [0.049, 0.5, 0.5], [1.049, 0.5, 0.5], [1.04, 0.5, 0.5], [1 + 1e-7, 0.5, 0.5]], F32)


@gpu
@pytest.mark.parametrize("name", ["one_cell", "distinct", "every_second_outside", "all_outside", "duplicates", "order"])
def test_contents(name):
    p = _content(name)
    grid = _grid((-10,) * 3, (10,) * 3, 1.0)
    n = len(p)
    ref = REF.voxel_ragged(p, [0, n], *grid, n)
    m = int(ref["offsets"][-1])
    assert m == {"one_cell": 1, "distinct": 3000, "every_second_outside": m, "all_outside": 0, "duplicates": 10, "order": 2}[name]
    if name == "every_second_outside":
        assert (ref["inverse"][::2] == -1).all() and (ref["inverse"][1::2] >= 0).all()
    if name == "order":
        assert ref["points"][0, 0] == F32(((np.float64(F32(1e-30)) + np.float64(F32(0.04))) + np.float64(F32(0.049))) / 3.0)
    for chunk in ((0,) if n < 1024 else (0, 1024)):
        _check(_run(p, [0, n], grid, n, chunk=chunk), ref, 1)
    # between two other clouds: offsets flat for an empty result, the neighbours untouched by it
    other = _sizes()["p"][:700]
    off = [0, 700, 700 + n, 1400 + n]
    batch = np.concatenate([other, p, other])
    _check(_run(batch, off, grid, max(n, 700), chunk=1024 if n > 1024 else 0), REF.voxel_ragged(batch, off, *grid, max(n, 700)), 3)


# ---- 4. faces --------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("v", [0.5, 0.25, 0.05, 0.1])
def test_faces(v):
    """Every face of the grid along each axis - the float32 nearest lo + k v, the float32 below it and the one above - with the other
    two coordinates inside a cell; the grid's upper face and what lies above it are outside.  For the binary edges the faces are exact;
    for 0.05 and 0.1 the cell is whatever fl(fl(p - lo) / v) says, rounded division included.  Then -0.0, NaN and +-inf rows."""
    lo, dims = -1.0, 40
    grid = ((lo,) * 3, (float(F32(v)),) * 3, (dims,) * 3)
    rows = []
    for axis in range(3):
        for k in range(dims + 1):
            f = F32(F32(lo) + F32(k) * F32(v))
            for x in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
                r = [F32(lo + 0.3 * v), F32(lo + 1.6 * v), F32(lo + 2.4 * v)]
                r[axis] = x
                rows.append(r)
    grid0 = ((0.0,) * 3, grid[1], grid[2])
    special = [[-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 0], [0, 0, np.inf],
               [-np.inf, -np.inf, -np.inf], [np.nan, np.nan, np.nan], [3e38, 0, 0], [-3e38, 0, 0], [1e-45, 1e-45, 1e-45], [-1e-45, 0, 0]]
    p = np.array(rows, F32)
    ref = REF.voxel_ragged(p, [0, len(p)], *grid, len(p))
    inside = ref["inverse"].reshape(3, dims + 1, 3) >= 0
    assert not inside[:, 0, 0].any() and inside[:, 0, 1:].all() and inside[:, 1:dims, :].all() and not inside[:, dims, 1:].any()
    if v in (0.5, 0.25):                                              # exact faces: the face itself opens cell k; the float below it
        c = REF.cells_of(p, *grid)[1].reshape(3, dims + 1, 3, 3)      # is in cell k - 1 unless fl(p - lo) rounds it onto the face
        for axis in range(3):
            assert (c[axis, 1:dims, 1, axis] == np.arange(1, dims)).all() and (c[axis, 1:dims, 2, axis] == np.arange(1, dims)).all()
            below = c[axis, 1:dims, 0, axis]
            assert ((below == np.arange(dims - 1)) | (below == np.arange(1, dims))).all() and (below == np.arange(dims - 1)).sum() > dims // 4
    _check(_run(p, [0, len(p)], grid, len(p)), ref, 1)
    s = np.array(special, F32)
    sref = REF.voxel_ragged(s, [0, len(s)], *grid0, len(s))
    assert sref["inverse"].tolist() == [0, 0] + [-1] * 10 + [0, -1] and sref["count"].tolist() == [3]
    _check(_run(s, [0, len(s)], grid0, len(s)), sref, 1)


# ---- 5. the integer lattice ------------------------------------------------------------------------------------------------------------------
def _lattice(seed=21, n=5000):
    return np.random.RandomState(seed).randint(-40, 41, size=(n, 3)).astype(F32)


@gpu
def test_integer_lattice_pins_every_output():
    """Integer coordinates in [-40, 40], cells of edge 2 from -40 (41^3 cells, three passes): sums of integers are exact in float64 in
    any order, so the centroids are pinned by an independent route (np.unique and np.add.at) as well as by the reference; count,
    first, cells and inverse likewise."""
    p = _lattice()
    grid = _grid((-40,) * 3, (40,) * 3, 2.0)
    assert grid[2] == (41, 41, 41) and REF.passes(41 ** 3) == 3
    ref = REF.voxel_ragged(p, [0, len(p)], *grid, len(p))
    cells, cnt, cen, inv = REF.voxel_brute_float64(p, *grid)
    assert np.array_equal(ref["cells"], cells) and np.array_equal(ref["count"], cnt) and np.array_equal(ref["inverse"], inv)
    assert np.array_equal(_bits(ref["points"]), _bits(cen.astype(F32))) and 1000 < len(cnt) < 5000 and cnt.max() > 1
    for chunk in (0, 1024, 2048):
        got = _run(p, [0, len(p)], grid, len(p), chunk=chunk)
        _check(got, ref, 1)
        m = len(cnt)
        assert np.array_equal(_bits(got["out"][:m]), _bits(cen.astype(F32))) and np.array_equal(got["cells"][:m], cells)
        assert np.array_equal(got["first"][:m], [np.nonzero(inv == k)[0][0] for k in range(m)])


# ---- 6. determinism and invariance -----------------------------------------------------------------------------------------------------------
@gpu
def test_determinism_batch_invariance_and_permutation():
    p = _lattice(22, 6000)
    perm = np.random.RandomState(23).permutation(len(p))
    grid = _grid((-40,) * 3, (40,) * 3, 2.0)
    a, b = REF.voxel_one(p, *grid), REF.voxel_one(p[perm], *grid)
    # on the reference first: the lattice's sums are exact, so the centroids do not depend on the row order
    assert np.array_equal(a["cells"], b["cells"]) and np.array_equal(a["count"], b["count"]) and np.array_equal(_bits(a["points"]), _bits(b["points"]))
    assert not np.array_equal(a["first"], b["first"])
    noisy = _sizes()["p"][-9000:] * F32(3.9)                          # a cloud whose sums do depend on the order
    batch = np.concatenate([p, noisy, p[perm]])
    off = _offsets([len(p), len(noisy), len(p)])
    ref = REF.voxel_ragged(batch, off, *grid, 9000)
    runs = [_run(batch, off, grid, 9000, chunk=c) for c in (0, 0, 1024, 2048, 4096, 9216)]
    _check(runs[0], ref, 3)
    assert all(_same(runs[0], r) for r in runs[1:])                   # two calls, every chunk length, the one-workgroup route
    m = [int(x) for x in ref["offsets"]]
    got = runs[0]
    assert m[1] - m[0] == m[3] - m[2] == len(a["count"])
    for k in ("out", "count", "cells"):                               # the permuted cloud: the same voxels, counts and centroids
        assert np.array_equal(got[k][m[0]:m[1]].view(np.int32), got[k][m[2]:m[3]].view(np.int32)), k
    assert np.array_equal(got["inverse"][:len(p)][perm], got["inverse"][off[2]:off[3]])
    for i in range(3):                                                # each cloud alone
        alone = _run(batch[off[i]:off[i + 1]], [0, off[i + 1] - off[i]], grid, off[i + 1] - off[i])
        for k in ("out", "count", "first", "cells"):
            assert np.array_equal(alone[k][:m[i + 1] - m[i]].view(np.int32) if k == "out" else alone[k][:m[i + 1] - m[i]],
                                  got[k][m[i]:m[i + 1]].view(np.int32) if k == "out" else got[k][m[i]:m[i + 1]]), (i, k)
        assert np.array_equal(alone["inverse"][:off[i + 1] - off[i]], got["inverse"][off[i]:off[i + 1]])


# ---- 7. bounds -------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_bounds_and_counts():
    s = _sizes()
    lengths = [300, 5000, 0, 2500, 1100]
    off = _offsets(lengths)
    p = s["p"][-off[-1]:]
    grid = s["grid"]
    exact = _run(p, off, grid, 5000)
    _check(exact, REF.voxel_ragged(p, off, *grid, 5000), 5)
    assert _same(exact, _run(p, off, grid, 10 ** 6))                  # a loose host bound changes the grids, not the result
    for bound in (1, 64, 1000, 1024, 2499):                           # a bound below a segment: its first rows only
        _check(_run(p, off, grid, bound), REF.voxel_ragged(p, off, *grid, bound), 5)
    for counts in ([300, 5000, 0, 2500, 1100], [10, 0, 0, 2499, 5000], [0, 0, 0, 0, 0], [-5, 1 << 30, 7, 1, 1025]):
        ref = REF.voxel_ragged(p, off, *grid, 5000, counts=counts)
        _check(_run(p, off, grid, 5000, counts=counts), ref, 5)
        _check(_run(p, off, grid, 5000, counts=counts, chunk=1024), ref, 5)
    _check(_run(p, off, grid, 1200, counts=[300, 1300, 0, 1150, 5]), REF.voxel_ragged(p, off, *grid, 1200, counts=[300, 1300, 0, 1150, 5]), 5)


# ---- 8. past the scans' 256 lanes --------------------------------------------------------------------------------------------------------------
@gpu
def test_one_cloud_of_257_segment_blocks():
    """262 145 rows are 257 blocks of 1024 sorted positions, one more than the 256 lanes of the per-cloud scan of the block counts:
    its second turn starts from the first one's carry.  Rows uniform in a box of 45^3 cells, about three per occupied cell; the
    automatic chunk."""
    n = 256 * 1024 + 1
    p = np.random.RandomState(21).uniform(0.0, 44.0, size=(n, 3)).astype(F32)
    grid = _grid((0,) * 3, (44,) * 3, 1.0)
    ref = REF.voxel_ragged(p, [0, n], *grid, n)
    assert -(-n // 1024) == 257 and 2.5 < ref["count"].mean() < 4 and ref["offsets"][1] > 256 * 256
    _check(_run(p, [0, n], grid, n), ref, 1)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_python_layer():
    from rald_amd import postprocess as PP
    s = _sizes()
    off = _offsets([700, 0, 4099])
    p = s["p"][-off[-1]:]
    ref = REF.voxel_ragged(p, off, *s["grid"], 4099)
    M = int(ref["offsets"][-1])
    dp, doff = torch.from_numpy(p).cuda(), torch.tensor(off, device="cuda")
    out = PP.voxel_downsample_ragged(dp, doff, s["grid"], 4099, return_count=True, return_first=True, return_cells=True, return_inverse=True)
    assert len(out) == 6 and out[1].tolist() == ref["offsets"].tolist()
    assert np.array_equal(_bits(out[0][:M].cpu().numpy()), _bits(ref["points"]))
    for t, k in zip(out[2:5], ("count", "first", "cells")):
        assert np.array_equal(t[:M].cpu().numpy(), ref[k]) and t.dtype == torch.from_numpy(ref[k]).dtype
    assert np.array_equal(out[5].cpu().numpy(), ref["inverse"])
    assert len(PP.voxel_downsample_ragged(dp, doff, s["grid"], 4099)) == 2
    assert [t.dtype for t in PP.voxel_downsample_ragged(dp, doff, s["grid"], 4099, return_first=True, return_inverse=True)[2:]] == [torch.int64] * 2
    # one cloud, with bounds and with its own extent
    one = PP.voxel_downsample(dp[:700], 1.0, lo=(-10,) * 3, hi=(10,) * 3)
    assert np.array_equal(_bits(one.cpu().numpy()), _bits(ref["points"][:int(ref["offsets"][1])]))
    q = p[:700]
    own = PP.voxel_downsample(dp[:700], (1.0, 2.0, 0.5))
    want = REF.voxel_one(q, *PP.voxel_grid(q.min(axis=0).tolist(), q.max(axis=0).tolist(), (1.0, 2.0, 0.5)))
    assert np.array_equal(_bits(own.cpu().numpy()), _bits(want["points"])) and (want["inverse"] >= 0).all()
    with pytest.raises(RuntimeError):
        PP.voxel_downsample_ragged(torch.from_numpy(p), doff, s["grid"], 4099)


# ---- 9. the tail -----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_infer_point_clouds_thin():
    """infer_point_clouds(..., thin=0.5) on the 4-frame setup of tests/test_gpu_infer_batch.py (view cone: the cube of +-15.8 m), alone,
    with normals and with resample: the new keys equal the references on the returned 'pred', every other key equals the call without
    the argument."""
    import fps_ref
    from rald_amd import engine_generation as E, postprocess as PP, query_points as QP, synth
    from test_gpu_infer_batch import _small_vae, _tail_args
    vae, z9 = _small_vae()
    z = z9[:4].contiguous()
    n, aug, k = 3000, 2048, 300
    args = _tail_args(n, aug)
    helpers = [synth.queries(1, max(h, 1), seed=100 + h)[0][:h].cuda() for h in (0, 1, 500, 1100)]
    surfaces = synth.point_cloud(4, 1000, seed=62).cuda()
    draws = QP.draw_tail_randoms(4, n, aug, 10, torch.Generator("cuda").manual_seed(23))
    kw = dict(helper_points=helpers, surfaces=surfaces, draws=draws)
    grid = PP.voxel_grid([-15.8] * 3, [15.8] * 3, 0.5)
    base = E.infer_point_clouds(vae, z, args, **kw)
    res = E.infer_point_clouds(vae, z, args, thin=0.5, **kw)
    assert set(res) == set(base) | {"thinned", "thin_count", "thin_first"} and res["n_queries"] == base["n_queries"]
    assert all(torch.equal(a, b) for a, b in zip(res["pred"], base["pred"]))
    assert all(a == b or abs(a - b) <= 1e-9 * abs(b) for a, b in zip(res["cd"], base["cd"]))      # cal_metrics_ragged's double atomics

    def check_thin(r):
        refs = []
        for b in range(4):
            ref = REF.voxel_one(r["pred"][b].cpu().numpy(), *grid)
            assert np.array_equal(_bits(r["thinned"][b].cpu().numpy()), _bits(ref["points"])), b
            assert np.array_equal(r["thin_count"][b].cpu().numpy(), ref["count"]) and np.array_equal(r["thin_first"][b].cpu().numpy(), ref["first"])
            assert r["thin_count"][b].dtype == torch.int32 and r["thin_first"][b].dtype == torch.int64
            refs.append(ref)
        return refs
    refs = check_thin(res)
    sizes = [(p.shape[0], len(r["count"])) for p, r in zip(res["pred"], refs)]
    print("final clouds and their voxels:", sizes)
    assert any(0 < m < n_ for n_, m in sizes)
    with_n = E.infer_point_clouds(vae, z, args, thin=0.5, normals=True, **kw)
    check_thin(with_n)
    for b in range(4):
        assert torch.equal(with_n["thinned_normals"][b], with_n["normals"][b][with_n["thin_first"][b]])
    both = E.infer_point_clouds(vae, z, args, thin=0.5, resample=k, **kw)
    assert set(both) == set(res) | {"resampled", "resample_index"}
    refs = check_thin(both)
    flat = np.concatenate([r["points"] for r in refs])
    lengths = [len(r["count"]) for r in refs]
    want_pts, want_idx = fps_ref.resample_ref(flat, _offsets(lengths), k, max(max(lengths), 1))
    assert np.array_equal(both["resample_index"].cpu().numpy(), want_idx)
    assert np.array_equal(_bits(both["resampled"].cpu().numpy()), _bits(want_pts))
    dev = E.infer_point_clouds_device(vae, z, args, thin=0.5, resample=k, **kw)
    assert len(dev) == 9 and torch.equal(dev[-1], both["resample_index"]) and dev[4].tolist() == _offsets(lengths)
    with pytest.raises(ValueError):
        E.infer_point_clouds(vae, z, args, thin=0.01, **kw)


@gpu
def test_thin_then_resample_on_a_frame_longer_than_the_sampler_takes():
    """The tail's chain (engine_generation._thin, _thin_bound, _resample) on a 70 000-row frame in [-10, 10)^3 with a 1.0 cell: at most
    8000 voxels, inside the sampler's resident form, and 'resampled' equals the farthest-point reference run on the voxel reference's
    output.  Without thinning the same frame is sampled from its first 65 536 rows - today's behaviour, unchanged."""
    import fps_ref
    from rald_amd import engine_generation as E, postprocess as PP
    k = 48
    p = np.random.RandomState(31).uniform(-10, 10, size=(70000, 3)).astype(F32)
    p = np.minimum(p, np.nextafter(F32(10), F32(0)))
    grid = PP.voxel_grid((-10,) * 3, (10,) * 3, 1.0)
    dp, off = torch.from_numpy(p).cuda(), torch.tensor([0, 70000], device="cuda")
    thinned = E._thin(dp, off, grid, 70000)
    ref = REF.voxel_one(p, *grid)
    m = len(ref["count"])
    assert m <= 8000 and thinned[1].tolist() == [0, m] and np.array_equal(_bits(thinned[0][:m].cpu().numpy()), _bits(ref["points"]))
    bound = E._thin_bound(70000, grid)
    assert bound == 21 ** 3 <= 16384
    pts, idx = E._resample(thinned[0], thinned[1], k, bound)
    want_pts, want_idx = fps_ref.resample_ref(ref["points"], [0, m], k, bound)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(_bits(pts.cpu().numpy()), _bits(want_pts))
    pts, idx = E._resample(dp, off, k, 70000)
    want_pts, want_idx = fps_ref.resample_ref(p[:65536], [0, 65536], k, 65536)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(_bits(pts.cpu().numpy()), _bits(want_pts))
