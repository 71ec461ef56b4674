"""Surface-nets meshing on the GPU (rald_amd/csrc/surface_nets.hip) against tests/surface_ref.py, by equality:
integers as integers, floats by bit pattern - no tolerance anywhere.  Every call of the C entry goes through _run: the outputs are
pre-filled with poison (NaNs with a payload, -7) and followed by guard rows, the volume is followed by NaNs, the scratch is filled with
0xFF and followed by a guard, and _check asserts that everything the definition does not write still holds its poison.
tests/test_surface_host.py holds the reference against an independent route and shows what each construction is for.  Below the entry:
the node grid, decode_volume, mesh_to_metric and extract_meshes against the existing entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import surface_ref as REF
from test_gpu_radius_filter import F32, GUARD, POISON_F, POISON_I, _bits

gpu = pytest.mark.gpu
CONE = [2.0, -60.0, -30.0, 50.0, 60.0, 30.0]            # r > 0 and |el| < 90 on the whole normalised cube
BOX = [-40.0, -30.0, -2.0, 60.0, 30.0, 6.0]


def _call(L, vol_ptr, B, dims, lo, h, iso, t_, max_v, max_f, scratch_ptr, nbytes):
    from rald_amd._handles import _stream
    ptr = lambda k: None if t_.get(k) is None else t_[k].data_ptr()
    return L.rald_post_surface_nets(vol_ptr, B, None if dims is None else (C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*h),
                                    float(iso), ptr("vertices"), ptr("v_offsets"), max_v, ptr("faces"), ptr("f_offsets"), max_f, ptr("cells"),
                                    scratch_ptr, nbytes, _stream())


def _buffers(B, max_v, max_f, outputs=True, cells=True):
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_ = dict(v_offsets=cu(np.full(B + 1 + GUARD, POISON_I, np.int64)), f_offsets=cu(np.full(B + 1 + GUARD, POISON_I, np.int64)))
    if outputs:
        t_.update(vertices=cu(np.full((max_v + GUARD, 3), POISON_F, F32)), faces=cu(np.full((max_f + GUARD, 3), POISON_I, np.int32)))
        if cells:
            t_.update(cells=cu(np.full(max_v + GUARD, POISON_I, np.int32)))
    return t_


def _run(vols, iso=0.0, lo=(0, 0, 0), h=(1, 1, 1), max_v=0, max_f=0, outputs=True, cells=True):
    """The C entry on poisoned, guarded buffers -> dict of numpy arrays, whole buffers (guards included)."""
    from rald_amd._lib import check, lib
    vols = np.ascontiguousarray(vols, F32)
    B, dims = vols.shape[0], vols.shape[1:]
    dev_v = torch.from_numpy(np.concatenate([vols.reshape(-1), np.full(4 * GUARD, np.nan, F32)])).cuda()
    t_ = _buffers(B, max_v, max_f, outputs, cells)
    L = lib()
    nbytes = L.rald_post_surface_scratch_bytes(B, *dims)
    assert nbytes > 0
    scratch = torch.empty(nbytes + 16 * GUARD, dtype=torch.uint8, device="cuda")
    scratch[:nbytes] = 0xFF                                            # -1 / NaN everywhere: nothing may rest on a zeroed scratch
    scratch[nbytes:] = 0xA5
    check(_call(L, dev_v.data_ptr(), B, dims, lo, h, iso, t_, max_v, max_f, scratch.data_ptr(), nbytes))
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "the scratch's guard was written"
    return {k: v.cpu().numpy() for k, v in t_.items()}


def _check(got, ref, max_v, max_f):
    """Everything the call writes equals the reference; everything else still holds its poison."""
    B = len(ref["v_offsets"]) - 1
    for k in ("v_offsets", "f_offsets"):                               # the TRUE counts, whatever the capacity
        assert got[k][:B + 1].tolist() == ref[k].tolist() and (got[k][B + 1:] == POISON_I).all(), (k, got[k][:B + 1], ref[k])
    if "vertices" not in got:
        return
    V, F = min(int(ref["v_offsets"][-1]), max_v), min(int(ref["f_offsets"][-1]), max_f)
    bad = np.nonzero((_bits(got["vertices"][:V]) != _bits(ref["vertices"][:V])).any(1))[0]
    assert bad.size == 0, (bad[:5], got["vertices"][bad[:5]], ref["vertices"][bad[:5]])
    assert (_bits(got["vertices"][V:]) == _bits(POISON_F)).all(), "a vertex row behind the capacity or the last volume was written"
    bad = np.nonzero((got["faces"][:F] != ref["faces"][:F]).any(1))[0]
    assert bad.size == 0, (bad[:5], got["faces"][bad[:5]], ref["faces"][bad[:5]])
    assert (got["faces"][F:] == POISON_I).all(), "a face row behind the capacity or the last volume was written"
    if "cells" in got:
        assert np.array_equal(got["cells"][:V], ref["cells"][:V]) and (got["cells"][V:] == POISON_I).all()


def _exact(vols, iso=0.0, lo=(0, 0, 0), h=(1, 1, 1), ref=None, **kw):
    """The call with exactly the capacity the reference needs -> the reference."""
    vols = np.ascontiguousarray(vols, F32)
    ref = REF.extract_batch(vols, iso, lo, h) if ref is None else ref
    V, F = int(ref["v_offsets"][-1]), int(ref["f_offsets"][-1])
    _check(_run(vols, iso, lo, h, V, F, **kw), ref, V, F)
    return ref


_SPHERE = {}


def _sphere24():
    """The sphere at 24^3 and its reference, once."""
    if not _SPHERE:
        vol, lo, h = REF.sphere(24)
        _SPHERE.update(vol=vol, lo=lo, h=h, ref=REF.extract_batch(vol[None], 0.0, lo, h))
    return _SPHERE


# ---- the entry against the reference ---------------------------------------------------------------------------------------------------
@gpu
def test_tiny():
    """2 x 2 x 2 and 2 x 2 x 3 (one and two cells, no face), and 3^3 with one inside node: 8 vertices at lo + (5/6 or 7/6) x spacing, 12
    faces."""
    for dims in ((2, 2, 2), (2, 2, 3)):
        ref = _exact(REF.noise((2,) + dims, 3))
        assert ref["v_offsets"][-1] >= 1 and ref["f_offsets"][-1] == 0
    lo, h = (1.0, 2.0, 3.0), (0.5, 1.0, 2.0)
    ref = _exact(REF.one_inside()[None], 0.0, lo, h)
    assert ref["v_offsets"].tolist() == [0, 8] and ref["f_offsets"].tolist() == [0, 12]
    for a in range(3):
        want = {float(F32(lo[a]) + (F32(c) + F32(s) / F32(3)) * F32(h[a])) for c, s in ((0, 2.5), (1, 0.5))}
        assert set(ref["vertices"][:, a].astype(float).tolist()) == want


@gpu
@pytest.mark.parametrize("ny", [2, 3])
@pytest.mark.parametrize("nz", [63, 64, 65, 129])
def test_word_boundary(nz, ny):
    """nz around the 64-node word of the sign bits: the last word's tail, the bit shifted in from the next word, the cell and the face
    that straddle two words; ny = 2 has no y-interior (only the y-edges make faces), ny = 3 has one row of it (all three axes do).
    B = 2."""
    ref = _exact(REF.noise((2, 4, ny, nz), nz + ny), 0.1)
    assert ref["v_offsets"][-1] > nz and ref["f_offsets"][-1] > nz


@gpu
def test_dims_that_divide_nothing():
    """37 x 21 x 70 noise at iso = 0.3, anisotropic spacing and a non-zero lo: no dimension a multiple of a tile, a word or a block."""
    _exact(REF.noise((1, 37, 21, 70), 4), 0.3, (0.5, -1.25, 2.0), (0.1, 0.25, 0.3))


@gpu
def test_sphere_102():
    """One volume of 102^3 (21 blocks of 1024 words): 17258 vertices, 34512 faces, as the host reference measured."""
    vol, lo, h = REF.sphere(102)
    ref = _exact(vol[None], 0.0, lo, h)
    assert (int(ref["v_offsets"][-1]), int(ref["f_offsets"][-1])) == (17258, 34512)


@gpu
def test_more_than_256_blocks_of_words():
    """600 x 450 x 3: one word per (i, j) row, 270000 words = 264 blocks of 1024, so the scan over a volume's blocks takes a second pass;
    sparse noise (iso = 1.5)."""
    ref = _exact(REF.noise((1, 600, 450, 3), 6), 1.5)
    assert ref["v_offsets"][-1] > 100000 and ref["f_offsets"][-1] > 10000


@gpu
def test_batch_positions():
    """An all-outside and an all-inside volume around the sphere (no vertex, no face, the offsets repeat), and the same sphere at batch
    positions 0 and 2 around noise: equal bits at both positions."""
    s = _sphere24()
    vols = np.stack([np.full_like(s["vol"], -1), s["vol"], np.full_like(s["vol"], 1)])
    ref = _exact(vols, 0.0, s["lo"], s["h"])
    V, F = int(s["ref"]["v_offsets"][-1]), int(s["ref"]["f_offsets"][-1])
    assert ref["v_offsets"].tolist() == [0, 0, V, V] and ref["f_offsets"].tolist() == [0, 0, F, F]
    vols = np.stack([s["vol"], REF.noise(s["vol"].shape, 8), s["vol"]])
    ref = REF.extract_batch(vols, 0.0, s["lo"], s["h"])
    cap = int(ref["v_offsets"][-1]), int(ref["f_offsets"][-1])
    got = _run(vols, 0.0, s["lo"], s["h"], *cap)
    _check(got, ref, *cap)
    vo, fo = ref["v_offsets"], ref["f_offsets"]
    assert np.array_equal(_bits(got["vertices"][:vo[1]]), _bits(got["vertices"][vo[2]:vo[3]]))
    assert np.array_equal(got["faces"][:fo[1]], got["faces"][fo[2]:fo[3]])


@gpu
def test_values_at_iso_and_hostile_values():
    """Nodes exactly at iso = 1 (outside under `>`), and NaN / +inf / -inf nodes at iso = 0.25 (a NaN t becomes 0, a NaN node is outside)."""
    vol, iso = REF.ties()
    _exact(vol[None], iso)
    _exact(np.stack([REF.hostile(), REF.hostile()[::-1].copy()]), 0.25, (-1, 0, 1), (0.5, 0.5, 2))
    _exact(REF.noise((1, 5, 6, 7), 9), float("inf"))                  # nothing is inside: no vertex


@gpu
def test_counting_call_and_short_capacities():
    """NULL outputs: the offsets alone.  Capacities one short in vertices, in faces and in both: the offsets stay true and the rows
    behind the capacity keep their poison.  out_cells NULL: the rest is unchanged.  Capacity 0 with outputs given."""
    s = _sphere24()
    vol, ref = s["vol"][None], s["ref"]
    V, F = int(ref["v_offsets"][-1]), int(ref["f_offsets"][-1])
    _check(_run(vol, 0.0, s["lo"], s["h"], outputs=False), ref, 0, 0)
    for mv, mf in ((V - 1, F), (V, F - 1), (V - 1, F - 1), (V // 2, 7), (0, 0), (V + 5, F + 5)):
        _check(_run(vol, 0.0, s["lo"], s["h"], mv, mf), ref, mv, mf)
    _check(_run(vol, 0.0, s["lo"], s["h"], V, F, cells=False), ref, V, F)


@gpu
def test_refused_arguments_write_nothing():
    """Every refused call returns a status (and a message) before any GPU work: the poisoned outputs are untouched."""
    from rald_amd._lib import lib
    L = lib()
    vol = torch.zeros(4 * 4 * 4 * 2, device="cuda")
    good = dict(vol=vol.data_ptr(), B=2, dims=(4, 4, 4), lo=(0, 0, 0), h=(1, 1, 1), iso=0.0)
    nbytes = L.rald_post_surface_scratch_bytes(2, 4, 4, 4)
    scratch = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    bad = [dict(vol=None), dict(B=0), dict(B=65536), dict(dims=(1, 4, 4)), dict(dims=(4, 4, 1025)), dict(dims=None), dict(h=(1, 0, 1)),
           dict(h=(1, 1, float("nan"))), dict(h=(float("inf"), 1, 1)), dict(lo=(0, float("nan"), 0)), dict(iso=float("nan")), dict(nbytes=nbytes - 16),
           dict(scratch=None), dict(scratch=scratch.data_ptr() + 4), dict(max_v=-1), dict(max_f=-1), dict(B=8, dims=(512, 512, 512)),
           dict(drop="v_offsets"), dict(drop="f_offsets")]
    for kw in bad:
        t_ = _buffers(2, 8, 8)
        t_.pop(kw.pop("drop", None), None)
        a = {**good, "nbytes": nbytes, "scratch": scratch.data_ptr(), "max_v": 8, "max_f": 8, **kw}
        rc = _call(L, a["vol"], a["B"], a["dims"], a["lo"], a["h"], a["iso"], t_, a["max_v"], a["max_f"], a["scratch"], a["nbytes"])
        torch.cuda.synchronize()
        assert rc != 0 and L.rald_last_error(), kw
        for k, v in t_.items():
            v = v.cpu().numpy()
            assert (_bits(v) == _bits(POISON_F)).all() if v.dtype == F32 else (v == POISON_I).all(), (kw, k)
    assert bool((scratch == 0xFF).all())
    assert L.rald_post_surface_scratch_bytes(8, 256, 256, 256) > 0    # a batch of 8 volumes of 256^3 is accepted
    for sizes in ((1, 1024, 1024, 1024), (0, 4, 4, 4), (1, 4, 4, 1), (65536, 2, 2, 2)):
        assert L.rald_post_surface_scratch_bytes(*sizes) == -1


# ---- the Python entries ------------------------------------------------------------------------------------------------------------------
@gpu
def test_extract_surface_python():
    """capacity=None (count, read, exact) and a given capacity give the reference; extract_surface trims one volume."""
    from rald_amd import postprocess as PP
    s = _sphere24()
    vols = np.stack([s["vol"], REF.noise(s["vol"].shape, 8)])
    ref = REF.extract_batch(vols, 0.0, s["lo"], s["h"])
    V, F = int(ref["v_offsets"][-1]), int(ref["f_offsets"][-1])
    dv = torch.from_numpy(vols).cuda()
    for cap in (None, (V + 3, F + 3)):
        v, vo, f, fo, c = PP.extract_surface_batch(dv, 0.0, s["lo"], s["h"], capacity=cap, return_cells=True)
        assert v.shape[0] == (V if cap is None else V + 3) and f.shape[0] == (F if cap is None else F + 3)
        assert vo.cpu().tolist() == ref["v_offsets"].tolist() and fo.cpu().tolist() == ref["f_offsets"].tolist()
        assert np.array_equal(_bits(v[:V].cpu().numpy()), _bits(ref["vertices"])) and np.array_equal(f[:F].cpu().numpy(), ref["faces"])
        assert np.array_equal(c[:V].cpu().numpy(), ref["cells"])
    v, f = PP.extract_surface(dv[0], 0.0, s["lo"], s["h"])
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(s["ref"]["vertices"])) and np.array_equal(f.cpu().numpy(), s["ref"]["faces"])
    v, vo, f, fo = PP.extract_surface_batch(torch.full((2, 3, 3, 3), -1.0, device="cuda"))
    assert v.shape == (0, 3) and f.shape == (0, 3) and vo.cpu().tolist() == [0, 0, 0] and fo.cpu().tolist() == [0, 0, 0]


@gpu
def test_grid_queries_against_the_node_formula():
    """Every node of 5 x 7 x 9 with an anisotropic spacing, all planes and planes 2 .. 3, bit for bit."""
    from rald_amd import query_points as QP
    lo, h, dims = (0.5, -1.25, 2.0), (0.1, 0.3, 0.7), (5, 7, 9)
    want = REF.nodes(lo, h, dims)
    got = QP.grid_queries(lo, h, dims).cpu().numpy()
    assert got.shape == (5 * 7 * 9, 3) and np.array_equal(_bits(got), _bits(want.reshape(-1, 3)))
    part = QP.grid_queries(lo, h, dims, 2, 2).cpu().numpy()
    assert np.array_equal(_bits(part), _bits(want[2:4].reshape(-1, 3)))
    glo, gh, gd = QP.field_grid(24)
    assert np.array_equal(_bits(QP.grid_queries(glo, gh, gd).cpu().numpy()), _bits(REF.nodes(*REF.box_grid(24), (24,) * 3).reshape(-1, 3)))


def _vae(dim, M):
    from test_gpu_oriented_points import _vae as centred
    return centred(dim, M, centre=True)


@gpu
@pytest.mark.parametrize("dim,M", [(256, 64), (512, 512)])
def test_decode_volume_equals_decode(dim, M):
    """The decoder shapes of tests/test_gpu_ae_rays.py (256 / 64 and 512 / 512), B = 3: torch.equal to decode on grid_queries' positions.
    9 x 5 x 7: planes of 35 nodes, a slab needs 64 of them, so the grid is one slab whatever max_queries says.  70 x 3 x 2: planes of 6,
    slabs of 32 planes at max_queries = 200 (32, 32, 6).  6 x 4 x 8: planes of 32, slabs of 2 at max_queries = 64, one slab by default."""
    from rald_amd import query_points as QP
    m, _, z = _vae(dim, M)
    for dims, max_queries in (((9, 5, 7), 100), ((70, 3, 2), 200), ((6, 4, 8), 64), ((6, 4, 8), 1 << 22)):
        lo, h = (-1.0, -0.9, -0.8), (1.9 / (dims[0] - 1), 0.4, 0.2)
        q = QP.grid_queries(lo, h, dims)
        want = m.decode(z, q[None].expand(3, -1, -1).contiguous()).reshape(3, *dims)
        got = m.decode_volume(z, lo, h, dims, max_queries=max_queries)
        assert got.shape == (3,) + dims and torch.equal(got, want), (dims, max_queries)


def _sphere_mesh():
    from rald_amd import postprocess as PP
    s = _sphere24()
    return PP.extract_surface(torch.from_numpy(s["vol"]).cuda(), 0.0, s["lo"], s["h"])


@gpu
@pytest.mark.parametrize("view_cone", [True, False])
def test_mesh_to_metric_keeps_the_normals_outward(view_cone):
    """The sphere's mesh through the view-cone transform (which reverses orientation: the winding is swapped) and through the plain one
    (which does not): the signed volume, in float64 on the host from what comes back, is positive both times, and the vertices are the
    existing transform's."""
    from rald_amd import postprocess as PP
    v, f = _sphere_mesh()
    rng = CONE if view_cone else BOX
    pts, faces = PP.mesh_to_metric(v, f, rng, True, False, view_cone)
    assert torch.equal(pts, PP._transform(v, rng, True, False, view_cone))
    vol = REF.signed_volume(pts.cpu().numpy(), faces.cpu().numpy())
    unswapped = REF.signed_volume(pts.cpu().numpy(), f.cpu().numpy())
    print(f"mesh_to_metric view_cone={view_cone}: signed volume {vol:.6g} (faces as extracted: {unswapped:.6g})")
    assert vol > 0 and (unswapped < 0) == view_cone
    assert REF.signed_volume(v.cpu().numpy(), f.cpu().numpy()) > 0


@gpu
@pytest.mark.parametrize("normals,surface_steps", [(False, 0), (True, 0), (False, 2), (True, 2)])
def test_extract_meshes_equals_the_chain_by_hand(normals, surface_steps):
    """extract_meshes at 20^3 on the centred depth-1 autoencoder (B = 3) equals field_grid -> decode_volume -> extract_surface_batch ->
    project_to_surface_ragged -> mesh_to_metric / oriented_points_ragged composed here, bit for bit, with and without a given capacity;
    the Chamfer distance of cal_metrics_ragged on the same vertices to 1e-9 relative (its float64 sums have no fixed order)."""
    from rald_amd import engine_generation as E, postprocess as PP, query_points as QP
    from test_gpu_infer_batch import PC_RANGE, _tail_args
    m, _, z = _vae(256, 128)
    args = _tail_args(1000, 100)
    surfaces = torch.rand(3, 50, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1
    lo, h, dims = QP.field_grid(20)
    v, vo, f, fo = PP.extract_surface_batch(m.decode_volume(z, lo, h, dims), 0.0, lo, h)
    V, F = v.shape[0], f.shape[0]
    assert V > 100 and F > 100
    longest = max(1, min(V, 19 ** 3))
    grad = None
    if normals or surface_steps:
        v, _, grad = QP.project_to_surface_ragged(m, z, v, vo, longest, surface_steps, 0.05)
    pts, faces = PP.mesh_to_metric(v, f, PC_RANGE, True, False, True)
    nrm = PP.oriented_points_ragged(v, grad, vo, PC_RANGE, True, False, True)[1] if normals else None
    gt = PP.polar2cartesian(PP.inverse_norm_points(surfaces.cuda().reshape(-1, 3), PC_RANGE, True, False))
    cd = PP.cal_metrics_ragged(pts, vo, gt, torch.arange(4, dtype=torch.int64, device="cuda") * 50, longest, 50).cpu().tolist()
    vo, fo = vo.cpu().tolist(), fo.cpu().tolist()
    for cap in (None, (V, F)):
        out = E.extract_meshes(m, z, args, 20, normals=normals, surface_steps=surface_steps, capacity=cap, surfaces=surfaces)
        assert len(out) == 3
        for b, mesh in enumerate(out):
            assert torch.equal(mesh["vertices"], pts[vo[b]:vo[b + 1]]) and torch.equal(mesh["faces"], faces[fo[b]:fo[b + 1]])
            assert ("normals" in mesh) == normals and (not normals or torch.equal(mesh["normals"], nrm[vo[b]:vo[b + 1]]))
            assert abs(mesh["cd"] - cd[b]) <= 1e-9 * cd[b], (b, mesh["cd"], cd[b])   # float64 sums in no fixed order, as test_gpu_infer_batch.py
    with pytest.raises(RuntimeError):
        E.extract_meshes(m, z, args, 20, capacity=(V - 1, F))
