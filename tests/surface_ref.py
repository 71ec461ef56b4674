"""The definition of the surface-nets meshing of a dense volume (include/rald_hip.h) in numpy, for the tests to
compare with by equality: fp32 one numpy operation at a time, so every operation is rounded once and nothing is contracted.

extract is the reference: whole-array operations over all cells and all grid edges, the faces sorted by their key.  extract_alt is an
independent route for tests/test_surface_host.py: a Python loop over the cells and over the nodes in their order, numpy float32 scalars,
a dictionary from cell to vertex.  Both take a `mutate` name (MUTATIONS) that breaks one rule of the definition on purpose.  Below them
the constructions both test files use, and the mesh checks (edge incidence, Euler characteristic, signed volume)."""
import numpy as np

F32 = np.float32
MUTATIONS = ("ge", "diagonal", "winding", "edge_order", "no_nan_rule")
CYCLIC = ((1, 2), (2, 0), (0, 1))                          # the (u, w) axes of an edge along x, y, z


def _edge(e):
    """e -> (axis, the two other axes ascending, p, q)."""
    axis, p, q = e >> 2, (e >> 1) & 1, e & 1
    o1, o2 = [x for x in range(3) if x != axis]
    return axis, o1, o2, p, q


def _inside(vol, iso, mutate):
    with np.errstate(invalid="ignore"):
        return vol >= iso if mutate == "ge" else vol > iso


def _clamp(t, mutate):
    if mutate != "no_nan_rule":
        t = np.where(np.isnan(t), F32(0), t)
    return np.where(t < 0, F32(0), np.where(t > 1, F32(1), t)).astype(F32)


def _triangles(c0, c1, c2, c3, inside, mutate):
    """The two triangles of a quad, [..., 2, 3]."""
    if mutate == "diagonal":
        a, b = (c0, c1, c3), (c1, c2, c3)
    else:
        a, b = (c0, c1, c2), (c0, c2, c3)
    keep = (inside if mutate != "winding" else ~inside)[:, None]
    a = np.where(keep, np.stack(a, 1), np.stack((a[0], a[2], a[1]), 1))
    b = np.where(keep, np.stack(b, 1), np.stack((b[0], b[2], b[1]), 1))
    return np.stack((a, b), 1)                             # [n, 2, 3]


def extract(volume, iso=0.0, lo=(0, 0, 0), spacing=(1, 1, 1), mutate=None):
    """volume f32 [nx, ny, nz] -> dict(vertices f32 [V, 3], faces int32 [F, 3], cells int32 [V])."""
    assert mutate is None or mutate in MUTATIONS
    vol = np.ascontiguousarray(volume, F32)
    nx, ny, nz = vol.shape
    iso = F32(iso)
    lo, h = np.array(lo, F32), np.array(spacing, F32)
    ins = _inside(vol, iso, mutate)
    corner = lambda a, d: a[d[0]:nx - 1 + d[0], d[1]:ny - 1 + d[1], d[2]:nz - 1 + d[2]]
    corners = [(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    n_in = sum(corner(ins, d).astype(np.int32) for d in corners)
    active = (n_in > 0) & (n_in < 8)
    shape = active.shape
    s = [np.zeros(shape, F32) for _ in range(3)]
    count = np.zeros(shape, np.int32)
    order = range(12) if mutate != "edge_order" else range(11, -1, -1)
    with np.errstate(all="ignore"):
        for e in order:
            axis, o1, o2, p, q = _edge(e)
            d0, d1 = [0, 0, 0], [0, 0, 0]
            d1[axis] = 1
            d0[o1] = d1[o1] = p
            d0[o2] = d1[o2] = q
            va, vb = corner(vol, d0), corner(vol, d1)
            cross = corner(ins, d0) != corner(ins, d1)
            t = _clamp((iso - va) / (vb - va), mutate)
            s[axis] = np.where(cross, s[axis] + t, s[axis])
            s[o1] = np.where(cross, s[o1] + F32(p), s[o1])
            s[o2] = np.where(cross, s[o2] + F32(q), s[o2])
            count += cross
    at = np.nonzero(active)                                # C order: ascending linear cell index
    n = count[at].astype(F32)
    vertices = np.empty((len(at[0]), 3), F32)
    for a in range(3):
        u = s[a][at] / n
        vertices[:, a] = lo[a] + (at[a].astype(F32) + u) * h[a]
    assert vertices.dtype == F32
    cells = ((at[0] * (ny - 1) + at[1]) * (nz - 1) + at[2]).astype(np.int32)
    vid = np.full(shape, -1, np.int64)
    vid[at] = np.arange(len(at[0]))
    dims = (nx, ny, nz)
    keys, tris = [], []
    for a in range(3):
        u, w = CYCLIC[a]
        sl = [slice(None)] * 3
        sl[a] = slice(0, dims[a] - 1)
        sl[u] = slice(1, dims[u] - 1)
        sl[w] = slice(1, dims[w] - 1)
        up = list(sl)
        up[a] = slice(1, dims[a])
        cross = ins[tuple(sl)] != ins[tuple(up)]
        idx = np.nonzero(cross)
        node = [idx[0] + sl[0].start, idx[1] + sl[1].start, idx[2] + sl[2].start]
        cell = []
        for du, dw in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            c = [x.copy() for x in node]
            c[u] += du
            c[w] += dw
            cell.append(vid[tuple(c)])
        assert all((c >= 0).all() for c in cell)           # the four cells are active by construction
        keys.append(((node[0] * ny + node[1]) * nz + node[2]) * 3 + a)
        tris.append(_triangles(*cell, ins[tuple(node)], mutate))
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    faces = tris[np.argsort(keys, kind="stable")].reshape(-1, 3).astype(np.int32)
    return dict(vertices=vertices, faces=faces, cells=cells)


def extract_alt(volume, iso=0.0, lo=(0, 0, 0), spacing=(1, 1, 1), mutate=None):
    """The same result by a loop over the cells, then over the nodes and axes in the faces' order."""
    vol = np.ascontiguousarray(volume, F32)
    nx, ny, nz = vol.shape
    iso = F32(iso)
    lo, h = [F32(x) for x in lo], [F32(x) for x in spacing]
    inside = (lambda v: bool(v >= iso)) if mutate == "ge" else (lambda v: bool(v > iso))
    vid, vertices, cells = {}, [], []
    with np.errstate(all="ignore"):
        for i in range(nx - 1):
            for j in range(ny - 1):
                for k in range(nz - 1):
                    block = vol[i:i + 2, j:j + 2, k:k + 2]
                    flags = [inside(v) for v in block.reshape(-1)]
                    if all(flags) or not any(flags):
                        continue
                    total, count = [F32(0), F32(0), F32(0)], 0
                    for e in (range(12) if mutate != "edge_order" else range(11, -1, -1)):
                        axis, o1, o2, p, q = _edge(e)
                        a_at, b_at = [0, 0, 0], [0, 0, 0]
                        b_at[axis] = 1
                        a_at[o1] = b_at[o1] = p
                        a_at[o2] = b_at[o2] = q
                        va, vb = block[tuple(a_at)], block[tuple(b_at)]
                        if inside(va) == inside(vb):
                            continue
                        t = F32(F32(iso - va) / F32(vb - va))
                        if np.isnan(t) and mutate != "no_nan_rule":
                            t = F32(0)
                        t = F32(0) if t < 0 else (F32(1) if t > 1 else t)
                        point = [None] * 3
                        point[axis], point[o1], point[o2] = t, F32(p), F32(q)
                        total = [F32(total[x] + point[x]) for x in range(3)]
                        count += 1
                    u = [F32(total[x] / F32(count)) for x in range(3)]
                    vid[(i, j, k)] = len(vertices)
                    vertices.append([F32(lo[x] + F32(F32(F32((i, j, k)[x]) + u[x]) * h[x])) for x in range(3)])
                    cells.append((i * (ny - 1) + j) * (nz - 1) + k)
    dims = (nx, ny, nz)
    faces = []
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                n = (i, j, k)
                for a in range(3):
                    u, w = CYCLIC[a]
                    if n[a] + 1 >= dims[a] or not (1 <= n[u] <= dims[u] - 2 and 1 <= n[w] <= dims[w] - 2):
                        continue
                    m = list(n)
                    m[a] += 1
                    if inside(vol[n]) == inside(vol[tuple(m)]):
                        continue
                    c = []
                    for du, dw in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
                        x = list(n)
                        x[u] += du
                        x[w] += dw
                        c.append(vid[tuple(x)])
                    quad = [(c[0], c[1], c[3]), (c[1], c[2], c[3])] if mutate == "diagonal" else [(c[0], c[1], c[2]), (c[0], c[2], c[3])]
                    if inside(vol[n]) == (mutate == "winding"):
                        quad = [(t[0], t[2], t[1]) for t in quad]
                    faces += quad
    return dict(vertices=np.array(vertices, F32).reshape(-1, 3), faces=np.array(faces, np.int32).reshape(-1, 3),
                cells=np.array(cells, np.int32))


def extract_batch(volumes, iso=0.0, lo=(0, 0, 0), spacing=(1, 1, 1)):
    """[B, nx, ny, nz] -> the ragged result: vertices, v_offsets int64 [B + 1], faces, f_offsets, cells."""
    parts = [extract(v, iso, lo, spacing) for v in volumes]
    cat = lambda k, d, w: np.concatenate([p[k] for p in parts]) if parts else np.zeros((0,) + w, d)
    off = lambda k: np.array([0] + np.cumsum([len(p[k]) for p in parts]).tolist(), np.int64)
    return dict(vertices=cat("vertices", F32, (3,)), v_offsets=off("vertices"), faces=cat("faces", np.int32, (3,)), f_offsets=off("faces"),
                cells=cat("cells", np.int32, ()))


def same(a, b):
    """Two results equal: the floats by bit pattern."""
    return np.array_equal(a["vertices"].view(np.uint32), b["vertices"].view(np.uint32)) and np.array_equal(a["faces"], b["faces"]) and \
        np.array_equal(a["cells"], b["cells"])


# ---- the grid and the constructions ----------------------------------------------------------------------------------------------------
def box_grid(dims):
    """The grid over [-1, 1]^3 with these node counts -> (lo, spacing) as float32 numbers."""
    dims = (dims,) * 3 if np.isscalar(dims) else tuple(dims)
    return (F32(-1),) * 3, tuple(F32(2.0 / (n - 1)) for n in dims)


def nodes(lo, spacing, dims):
    """The node positions f32 [nx, ny, nz, 3] by the node formula."""
    ax = [F32(lo[a]) + np.arange(dims[a]).astype(F32) * F32(spacing[a]) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).astype(F32)


def _field(dims, fn):
    dims = (dims,) * 3 if np.isscalar(dims) else tuple(dims)
    lo, h = box_grid(dims)
    p = nodes(lo, h, dims).astype(np.float64)
    return fn(p[..., 0], p[..., 1], p[..., 2]).astype(F32), lo, h


def sphere(dims, R=0.6, centre=(0.0, 0.0, 0.0)):
    """value = R - |p - centre| on the box grid -> (volume, lo, spacing)."""
    return _field(dims, lambda x, y, z: R - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2))


def two_spheres(dims=24):
    return _field(dims, lambda x, y, z: np.maximum(0.3 - np.sqrt((x + 0.5) ** 2 + y ** 2 + z ** 2),
                                                   0.3 - np.sqrt((x - 0.5) ** 2 + (y - 0.1) ** 2 + z ** 2)))


def torus(dims=24, R=0.6, r=0.25):
    return _field(dims, lambda x, y, z: r - np.sqrt((np.sqrt(x ** 2 + y ** 2) - R) ** 2 + z ** 2))


def clipped_sphere(dims=16):
    return sphere(dims, R=1.2)


def ties(dims=(5, 6, 7)):
    """Small integers around iso = 1 with many nodes exactly at iso: `>=` for `>` moves them inside."""
    rng = np.random.default_rng(5)
    return rng.integers(-1, 4, dims).astype(F32), F32(1.0)


def hostile(dims=(6, 5, 9)):
    """Random values with NaN, +inf and -inf nodes: edges whose t is a NaN (inf - inf, inf / inf), and NaN nodes, which are outside."""
    rng = np.random.default_rng(9)
    v = rng.standard_normal(dims).astype(F32)
    r = rng.random(dims)
    v[r < 0.10] = np.nan
    v[(r >= 0.10) & (r < 0.20)] = np.inf
    v[(r >= 0.20) & (r < 0.30)] = -np.inf
    return v


def noise(dims, seed=0):
    return np.random.default_rng(seed).standard_normal(dims).astype(F32)


def one_inside(dims=(3, 3, 3)):
    """+1 at the centre node of a 3^3 volume of -1: 8 vertices, 12 faces."""
    v = np.full(dims, -1, F32)
    v[1, 1, 1] = 1
    return v


# ---- mesh checks ------------------------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_counts(faces):
    """-> (the number of triangles at every undirected edge, the number of times every directed edge occurs)."""
    d = directed_edges(faces)
    und = np.sort(d, 1)
    _, cu = np.unique(und, axis=0, return_counts=True)
    _, cd = np.unique(d, axis=0, return_counts=True)
    return cu, cd


def euler(n_vertices, faces):
    cu, _ = edge_counts(faces)
    return n_vertices - len(cu) + len(faces)


def signed_volume(vertices, faces):
    """float64: sum of det(a, b, c) / 6 over the triangles; positive for outward normals."""
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
