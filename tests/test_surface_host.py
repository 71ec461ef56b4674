"""The definition of the surface-nets meshing (tests/surface_ref.py, include/rald_hip.h) against its independent
route by bit pattern, what each construction of the tests is for shown on the reference alone, the named mutations of the definition,
and the argument rules of the new Python entries (ValueError before any device use).  No GPU, no library."""
import types

import numpy as np
import pytest
import torch

import surface_ref as REF

F32 = np.float32
R_SPHERE = 0.6
V_SPHERE = 4.0 / 3.0 * np.pi * R_SPHERE ** 3
# the sphere R = 0.6 on [-1, 1]^3: (vertices, faces, relative error of the signed volume as measured with the committed reference)
SPHERE = {12: (194, 384, -0.101708), 24: (890, 1776, -0.023767), 33: (1760, 3516, -0.012300)}
_ns = lambda **kw: types.SimpleNamespace(**kw)


def _mesh(vol, lo, h, iso=0.0):
    m = REF.extract(vol, iso, lo, h)
    assert REF.same(m, REF.extract_alt(vol, iso, lo, h)), "the two routes differ"
    return m


def _closed_and_oriented(m):
    cu, cd = REF.edge_counts(m["faces"])
    return bool((cu == 2).all()) and bool((cd == 1).all())


# ---- (a) analytic shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(SPHERE))
def test_sphere(n):
    """value = 0.6 - |p| at 12^3, 24^3, 33^3: a closed, consistently oriented 2-manifold of Euler characteristic 2 with outward normals.
    Measured with the committed reference: V = 194 / 890 / 1760, F = 384 / 1776 / 3516, signed volume -10.17 %, -2.38 %, -1.23 % off 4/3
    pi R^3 (and -0.12 % at 102^3, 17258 vertices, 34512 faces: tests/test_gpu_surface.py); asserted within 1.5 x the measured error."""
    vol, lo, h = REF.sphere(n)
    m = _mesh(vol, lo, h)
    V, F, err = SPHERE[n]
    assert (len(m["vertices"]), len(m["faces"])) == (V, F)
    assert _closed_and_oriented(m) and REF.euler(V, m["faces"]) == 2
    vol_mesh = REF.signed_volume(m["vertices"], m["faces"])
    rel = (vol_mesh - V_SPHERE) / V_SPHERE
    print(f"sphere {n}: V {V} F {F} signed volume {vol_mesh:.6f} ({100 * rel:+.3f} %)")
    assert vol_mesh > 0 and abs(rel) <= 1.5 * abs(err)


@pytest.mark.parametrize("name,chi", [("two_spheres", 4), ("torus", 0)])
def test_two_spheres_and_torus(name, chi):
    """Two disjoint spheres (two components: V - E + F = 4) and a torus (genus 1: 0) at 24^3: closed, oriented, positive volume.
    Measured: 428 / 848 and 1136 / 2272 vertices / faces; the torus' signed volume 0.7083 against 2 pi^2 R r^2 = 0.7402."""
    vol, lo, h = getattr(REF, name)()
    m = _mesh(vol, lo, h)
    assert _closed_and_oriented(m) and REF.euler(len(m["vertices"]), m["faces"]) == chi
    assert REF.signed_volume(m["vertices"], m["faces"]) > 0
    assert (len(m["vertices"]), len(m["faces"])) == {"two_spheres": (428, 848), "torus": (1136, 2272)}[name]


def test_sphere_clipped_by_the_box():
    """R = 1.2 at 16^3 leaves the box: the mesh is open, its boundary edges lie in exactly one triangle, every other edge in two, no
    directed edge twice, and no vertex lies outside the box (an edge on the grid's border makes no face: its four cells do not exist)."""
    vol, lo, h = REF.clipped_sphere()
    m = _mesh(vol, lo, h)
    cu, cd = REF.edge_counts(m["faces"])
    assert set(cu.tolist()) == {1, 2} and (cd == 1).all()
    assert (np.abs(m["vertices"]) <= 1).all() and m["faces"].min() >= 0 and m["faces"].max() < len(m["vertices"])


def test_one_inside_node():
    """One inside node at the centre of 3^3: the 8 cells around it, each with three crossing edges at t = 1/2 -> u = (1/2 + 1 + 1) / 3 or
    (1/2 + 0 + 0) / 3 per axis, so the vertices sit at lo + (5/6 or 7/6) * spacing, and the 6 edges at the node give 12 triangles."""
    lo, h = (1.0, 2.0, 3.0), (0.5, 1.0, 2.0)
    m = _mesh(REF.one_inside(), lo, h)
    assert len(m["vertices"]) == 8 and len(m["faces"]) == 12 and m["cells"].tolist() == list(range(8))
    for a in range(3):
        want = {float(F32(lo[a]) + (F32(c) + F32(s) / F32(3)) * F32(h[a])) for c, s in ((0, 2.5), (1, 0.5))}
        assert set(m["vertices"][:, a].astype(float).tolist()) == want
    assert _closed_and_oriented(m) and REF.signed_volume(m["vertices"], m["faces"]) > 0


@pytest.mark.parametrize("dims", [(2, 2, 2), (2, 2, 3), (2, 5, 2)])
def test_no_interior_edge_no_face(dims):
    """Grids with an axis of two nodes have vertices but no edge with four cells around it."""
    m = _mesh(REF.noise(dims, 3), (0, 0, 0), (1, 1, 1))
    assert len(m["vertices"]) >= 1 and len(m["faces"]) == 0


# ---- (b) the vertex lies in its cell -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise", "hostile", "ties", "sphere"])
def test_vertex_in_its_cell(name):
    """Every vertex lies in the closed box of its cell (the box's corners by the node formula), also with NaN and inf nodes."""
    lo, h, iso = (0.5, -1.0, 2.0), (0.1, 0.25, 0.3), 0.0
    if name == "sphere":
        vol, lo, h = REF.sphere(12)
    elif name == "ties":
        vol, iso = REF.ties()
    else:
        vol = REF.noise((7, 6, 9), 1) if name == "noise" else REF.hostile()
    m = _mesh(vol, lo, h, iso)
    nx, ny, nz = vol.shape
    c = m["cells"].astype(np.int64)
    ijk = np.stack([c // ((ny - 1) * (nz - 1)), c // (nz - 1) % (ny - 1), c % (nz - 1)], 1)
    assert len(c) > 20 and np.isfinite(m["vertices"]).all()
    for a in range(3):
        lo_a = F32(lo[a]) + ijk[:, a].astype(F32) * F32(h[a])
        hi_a = F32(lo[a]) + (ijk[:, a] + 1).astype(F32) * F32(h[a])
        assert (m["vertices"][:, a] >= lo_a).all() and (m["vertices"][:, a] <= hi_a).all()


# ---- (c) mutations -------------------------------------------------------------------------------------------------------------------------
def _mutated(vol, iso, mutation):
    a, b = REF.extract(vol, iso), REF.extract(vol, iso, mutate=mutation)
    assert REF.same(b, REF.extract_alt(vol, iso, mutate=mutation)), "the two routes differ under the mutation"
    return a, b


def test_mutation_ge():
    """`>=` for `>` moves the nodes exactly at iso inside: other counts on the volume of small integers."""
    vol, iso = REF.ties()
    assert int((vol == iso).sum()) > 20
    a, b = _mutated(vol, iso, "ge")
    assert (len(a["vertices"]), len(a["faces"])) != (len(b["vertices"]), len(b["faces"]))


def test_mutation_diagonal_and_winding():
    """The other diagonal gives other triangles over the same vertices and the same volume sign; the swapped winding flips the sign."""
    vol, lo, h = REF.sphere(12)
    a = REF.extract(vol, 0.0, lo, h)
    d, w = REF.extract(vol, 0.0, lo, h, mutate="diagonal"), REF.extract(vol, 0.0, lo, h, mutate="winding")
    assert REF.same(d, REF.extract_alt(vol, 0.0, lo, h, mutate="diagonal")) and REF.same(w, REF.extract_alt(vol, 0.0, lo, h, mutate="winding"))
    assert not np.array_equal(a["faces"], d["faces"]) and np.array_equal(a["vertices"], d["vertices"])
    assert REF.signed_volume(d["vertices"], d["faces"]) > 0
    assert REF.signed_volume(w["vertices"], w["faces"]) == -REF.signed_volume(a["vertices"], a["faces"]) < 0


def test_mutation_edge_order():
    """Summing the crossings in descending e changes the bits of some vertices (and moves none by more than a few ulps)."""
    a, b = _mutated(REF.noise((7, 6, 9), 1), 0.0, "edge_order")
    differ = (a["vertices"].view(np.uint32) != b["vertices"].view(np.uint32)).any(1)
    assert differ.sum() > 10 and np.allclose(a["vertices"], b["vertices"], rtol=0, atol=1e-5) and np.array_equal(a["faces"], b["faces"])


def test_mutation_nan_rule():
    """Without NaN -> 0 an edge between +inf and -inf (or from an inf to anything: inf / inf) leaves a NaN coordinate."""
    vol = REF.hostile()
    assert np.isnan(vol).sum() > 10 and np.isposinf(vol).sum() > 10 and np.isneginf(vol).sum() > 10
    a, b = _mutated(vol, 0.25, "no_nan_rule")
    assert np.isfinite(a["vertices"]).all() and np.isnan(b["vertices"]).any()


def test_nan_is_outside():
    """A NaN node is outside under `>`, whatever iso: replacing every NaN by -inf changes no face and no vertex count."""
    vol = REF.hostile()
    m, n = REF.extract(vol, 0.25), REF.extract(np.where(np.isnan(vol), -np.inf, vol).astype(F32), 0.25)
    assert np.array_equal(m["faces"], n["faces"]) and np.array_equal(m["cells"], n["cells"])


def test_batch_layout():
    vols = np.stack([np.full((5, 4, 6), -1, F32), REF.noise((5, 4, 6), 2), np.full((5, 4, 6), 1, F32), REF.noise((5, 4, 6), 2)])
    r = REF.extract_batch(vols, 0.0)
    one = REF.extract(vols[1], 0.0)
    assert r["v_offsets"].tolist() == [0, 0, len(one["vertices"]), len(one["vertices"]), 2 * len(one["vertices"])]
    assert r["f_offsets"].tolist() == [0, 0, len(one["faces"]), len(one["faces"]), 2 * len(one["faces"])]
    assert np.array_equal(r["faces"][:len(one["faces"])], r["faces"][len(one["faces"]):])


# ---- (d) argument rules ------------------------------------------------------------------------------------------------------------------
def test_extract_surface_argument_errors():
    from rald_amd import postprocess as PP
    vol = torch.zeros(2, 4, 4, 4)
    bad = [dict(volume=torch.zeros(4, 4, 4)), dict(volume=torch.zeros(2, 4, 4, 4, dtype=torch.int32)), dict(volume=torch.zeros(2, 1, 4, 4)),
           dict(volume=torch.zeros(1, 2, 2, 1025)), dict(iso=float("nan")), dict(iso="0"), dict(iso=True), dict(lo=(0, 0)),
           dict(lo=(0, 0, float("inf"))), dict(spacing=(1, 1, 0)), dict(spacing=(1, -1, 1)), dict(spacing=(1, 1, float("nan"))),
           dict(spacing=(1e-60, 1, 1)), dict(spacing=1.0), dict(capacity=(1,)), dict(capacity=(1, -1)), dict(capacity=(1.5, 2)), dict(capacity=5)]
    for kw in bad:
        with pytest.raises(ValueError):
            PP.extract_surface_batch(**{"volume": vol, **kw})
    for kw in (dict(volume=vol), dict(volume=torch.zeros(4, 4, 1)), dict(volume=torch.zeros(4, 4, 4), iso=None)):
        with pytest.raises(ValueError):
            PP.extract_surface(**kw)
    with pytest.raises(ValueError):                          # 8 x 512^3 nodes: more than the counters hold
        PP.extract_surface_batch(torch.zeros(1, 1, 1, 1).expand(8, 512, 512, 512))
    with pytest.raises(RuntimeError):                        # every rule passed: now the volume must live on the GPU
        PP.extract_surface_batch(vol)


def test_mesh_to_metric_argument_errors():
    from rald_amd import postprocess as PP
    v, f, rng = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), [0, -90, -20, 15.8, 90, 20]
    for args in ((torch.zeros(4, 2), f, rng, True, False), (v, torch.zeros(2, 3), rng, True, False), (v, torch.zeros(2, 4, dtype=torch.int32), rng, True, False),
                 (v, f, rng[:5], True, False), (v, f, rng, False, False)):
        with pytest.raises(ValueError):
            PP.mesh_to_metric(*args)
    with pytest.raises(RuntimeError):
        PP.mesh_to_metric(v, f, rng, True, False)


def test_grid_argument_errors():
    from rald_amd import query_points as QP
    assert QP.field_grid(3) == ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (3, 3, 3))
    lo, h, dims = QP.field_grid((2, 5, 1024))
    assert dims == (2, 5, 1024) and h == (2.0, 0.5, float(F32(2.0 / 1023)))
    for res in (1, 1025, 2.0, True, (4, 4), (4, 4, 1), "4", None):
        with pytest.raises(ValueError):
            QP.field_grid(res)
    for kw in (dict(dims=(4, 4)), dict(dims=(4, 4, 1)), dict(dims=(4, 4, 2.5)), dict(spacing=(1, 1, 0)), dict(lo=(0, float("nan"), 0)),
               dict(i0=-1), dict(i0=4), dict(i0=2, ni=3), dict(ni=0)):
        with pytest.raises(ValueError):
            QP.grid_queries(**{"lo": (0, 0, 0), "spacing": (1, 1, 1), "dims": (4, 4, 4), **kw})
    with pytest.raises(RuntimeError):
        QP.grid_queries((0, 0, 0), (1, 1, 1), (4, 4, 4), device="cpu")


def test_decode_volume_argument_errors():
    from rald_amd import models_ae as A
    m = A.KLAutoEncoder(depth=1, dim=256, queries_dim=256, num_latents=64, latent_dim=32, num_inputs=1000, query_type="mix")
    x = torch.zeros(1, 64, 32)
    for kw in (dict(dims=(4, 4, 1)), dict(spacing=(0, 1, 1)), dict(max_queries=0), dict(max_queries=2.5), dict(x=torch.zeros(64, 32))):
        with pytest.raises(ValueError):
            m.decode_volume(**{"x": x, "lo": (-1, -1, -1), "spacing": (1, 1, 1), "dims": (3, 3, 3), **kw})


class _StubVae:
    """Fails the test if extract_meshes touches the autoencoder before its argument checks are through."""
    def __getattr__(self, name):
        raise AssertionError(f"the autoencoder was used ({name}) before the arguments were checked")


def _args(aniso=True, iso=False):
    return _ns(eval=_ns(skip_eval_metric=False),
               dataset=_ns(lidar=_ns(pc_range=[0, -90, -20, 15.8, 90, 20], norm_anisotropy=aniso, norm_isotropy=iso, view_cone_mode=True)))


def test_extract_meshes_argument_errors():
    from rald_amd import engine_generation as E
    z = torch.zeros(2, 8, 4)
    bad = [dict(resolution=1), dict(resolution=(8, 8)), dict(threshold=float("nan")), dict(threshold="0"), dict(surface_steps=-1),
           dict(surface_steps=1.5), dict(surface_max_step=0.0), dict(surface_max_step=float("inf")), dict(capacity=(10,)), dict(capacity=(-1, 5)),
           dict(capacity=7), dict(capacity=(1, 2, 3)), dict(surfaces=torch.zeros(3, 5, 3)), dict(surfaces=torch.zeros(2, 5, 2)), dict(metric_thresholds=(-1.0,)),
           dict(sampled_tokens=torch.zeros(8, 4)), dict(args=_args(False, False)), dict(resolution=1024)]
    for kw in bad:
        with pytest.raises(ValueError):
            E.extract_meshes(**{"vae": _StubVae(), "sampled_tokens": z, "args": _args(), "resolution": 8, **kw})
    with pytest.raises(AssertionError):                      # every rule passed: the first use of the autoencoder
        E.extract_meshes(_StubVae(), z, _args(), 8, capacity=(10, 20), metric_thresholds=(0.1,))
