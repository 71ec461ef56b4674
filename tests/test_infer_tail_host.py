"""The batched inference tail across its options, host side (no GPU, no library): with every device function stubbed (the stub chain of
tests/test_normals_host.py, plus the cluster filter as tests/test_cluster_host.py stubs it), every key of infer_point_clouds' dict is the
per-frame slice or the host copy of the matching element of infer_point_clouds_device's tuple, for every combination of
{no filter, denoise, denoise_statistical, denoise_cluster} x {Chamfer, metric_thresholds} x {no normals, normals, normals and
normal_consistency} x thin x resample x {surfaces, none}, and each call makes exactly one host read (the device form none).  And the
helper that packs that one read."""
import itertools
import math

import pytest
import torch

FILTERS = {"none": {}, "radius": dict(denoise=(0.5, 2)), "statistical": dict(denoise_statistical=(8, 2.0, 0.5, 1.25)),
           "cluster": dict(denoise_cluster=(0.5, 2, 30, True))}


def _stub_all(monkeypatch):
    from rald_amd import postprocess as real
    from test_normals_host import _stub_normals, _with_index
    E, calls, reads, pos, kw, seen = _stub_normals(monkeypatch)
    _with_index(E, calls)

    def cluster(pts, off, eps, min_points, min_cluster_size, grid, max_per_sample, largest_only=False, return_index=False, return_labels=False):
        calls.append("remove_small_clusters_ragged")
        return (torch.full((pts.shape[0], 3), 3.0), torch.tensor([0, 4, 6]), torch.arange(pts.shape[0]) * 2,
                torch.arange(pts.shape[0], dtype=torch.int32) % 3, torch.tensor([5, 9], dtype=torch.int32))

    # the chain's voxel stub names rows 0 .. T-1 as the cells' first rows, which only the first frame has; here every cell's first row
    # is row 0 or 1 of its frame, so that the normals gathered through thin_first (and through denoise_index) exist in every frame
    def thin(pts, off, grid, max_per_sample, return_count=False, return_first=False):
        calls.append("voxel_downsample_ragged")
        T = pts.shape[0]
        return (torch.arange(T * 3, dtype=torch.float32).reshape(T, 3), torch.tensor([0, 3, 5]), torch.arange(T, dtype=torch.int32) + 1,
                (torch.arange(T) + 1) % 2)

    def oriented(kept, grad, off, *a, **k):                                   # normals that tell their rows apart
        calls.append("oriented_points_ragged")
        return kept, torch.arange(kept.shape[0] * 3, dtype=torch.float32).reshape(-1, 3)
    E.PP.remove_small_clusters_ragged, E.PP._cluster_size = cluster, real._cluster_size
    E.PP.voxel_downsample_ragged, E.PP.oriented_points_ragged = thin, oriented
    return E, calls, reads, pos, kw


def _same(host, dev):
    """A host value of the dict against the device tensor it was read from, NaN equal to NaN."""
    want = dev.tolist()
    if isinstance(host, tuple):
        host = list(host)
    flat = lambda v: [x for y in v for x in flat(y)] if isinstance(v, list) else [v]
    a, b = flat(host), flat(want)
    return len(a) == len(b) and all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(a, b))


def _metrics_match(frames, metrics, B):
    return all(set(frames[b]) == set(metrics) and all(_same(frames[b][k], metrics[k][b]) for k in metrics) for b in range(B))


@pytest.mark.parametrize("which", sorted(FILTERS))
def test_every_key_of_the_dict_is_the_slice_or_host_copy_of_the_device_tuple(monkeypatch, which):
    E, calls, reads, pos, kw = _stub_all(monkeypatch)
    B, P = 2, 20
    combos = 0
    for taus, oriented, thin, resample, surf in itertools.product((None, (0.1, 0.2)), ("no", "normals", "consistency"), (None, 4.0), (None, 5),
                                                                  (True, False)):
        if oriented == "consistency" and not surf:
            continue                                                            # normal_consistency without surfaces is refused
        opts = dict(FILTERS[which], metric_thresholds=taus, thin=thin, resample=resample)
        if oriented != "no":
            opts["normals"] = True
        if oriented == "consistency":
            opts["normal_consistency"] = (8, 0.5)
        k = {**kw, **opts, **({} if surf else {"surfaces": None})}
        del reads[:]
        dev = list(E.infer_point_clouds_device(*pos, **k))
        assert not reads, opts
        out = E.infer_point_clouds(*pos, **k)
        assert len(reads) == 1, opts
        keys = {"pred", "cd", "n_queries"}
        pts, off, cd = dev[:3]
        at = 3
        o = off.tolist()
        per_frame = lambda t, oo: [t[oo[b]:oo[b + 1]] for b in range(B)]
        equal = lambda got, want: len(got) == len(want) and all(torch.equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
        assert equal(out["pred"], per_frame(pts, o)) and out["n_queries"] == [150, 150], opts
        assert (out["cd"] is None and cd is None and not surf) or _same(out["cd"], cd), opts
        if taus is not None:
            keys.add("metrics")
            metrics = dev[at]
            at += 1
            assert (out["metrics"] is None and metrics is None and not surf) or _metrics_match(out["metrics"], metrics, B), opts
            assert metrics is None or cd is metrics["cd"]
        nrm = None
        if oriented != "no":
            keys.add("normals")
            nrm = dev[at]
            at += 1
            assert equal(out["normals"], per_frame(nrm, o)), opts
        if oriented == "consistency":
            keys |= {"normal_consistency", "surface_normals"}
            nc, gt_nrm = dev[at:at + 2]
            at += 2
            assert all(_same(out["normal_consistency"][b], nc[b]) for b in range(B)), opts
            assert equal(out["surface_normals"], [gt_nrm[b * P:(b + 1) * P] for b in range(B)]), opts
        d_idx = None
        if which != "none":
            keys |= {"denoised", "denoise_index"}
            d_pts, d_off, d_idx, d_cd = dev[at:at + 4]
            at += 4
            do = d_off.tolist()
            assert equal(out["denoised"], per_frame(d_pts, do)) and equal(out["denoise_index"], per_frame(d_idx, do)), opts
            d_idx = per_frame(d_idx, do)
            if surf:
                keys.add("cd_denoised")
                assert _same(out["cd_denoised"], d_cd), opts
            else:
                assert d_cd is None
            if taus is not None:
                keys.add("metrics_denoised")
                d_metrics = dev[at]
                at += 1
                assert (out["metrics_denoised"] is None and d_metrics is None and not surf) or _metrics_match(out["metrics_denoised"], d_metrics, B)
            if nrm is not None:
                keys.add("denoised_normals")
                assert equal(out["denoised_normals"], [nrm[o[b] + d_idx[b]] for b in range(B)]), opts
            if which == "statistical":
                keys.add("denoise_stats")
                assert all(_same(out["denoise_stats"][b], dev[at][b]) for b in range(B)) and len(out["denoise_stats"]) == B, opts
                at += 1
            if which == "cluster":
                keys |= {"denoise_labels", "n_clusters"}
                assert equal(out["denoise_labels"], per_frame(dev[at], do)) and out["n_clusters"] == dev[at + 1].tolist(), opts
                assert all(isinstance(v, int) for v in out["n_clusters"])
                at += 2
        if thin is not None:
            keys |= {"thinned", "thin_count", "thin_first"}
            t_pts, t_off, t_count, t_first = dev[at:at + 4]
            at += 4
            to = t_off.tolist()
            for key, t in (("thinned", t_pts), ("thin_count", t_count), ("thin_first", t_first)):
                assert equal(out[key], per_frame(t, to)), (key, opts)
            if nrm is not None:
                keys.add("thinned_normals")
                first = per_frame(t_first, to)
                rows = first if d_idx is None else [d_idx[b][first[b]] for b in range(B)]
                assert equal(out["thinned_normals"], [nrm[o[b] + rows[b]] for b in range(B)]), opts
        if resample is not None:
            keys |= {"resampled", "resample_index"}
            assert torch.equal(out["resampled"], dev[at]) and torch.equal(out["resample_index"], dev[at + 1]), opts
            at += 2
        assert at == len(dev) and set(out) == keys, opts
        assert all(isinstance(v, int) for v in out["n_queries"])
        combos += 1
    assert combos == 40


def test_the_host_pack_returns_every_group_from_one_read(monkeypatch):
    from rald_amd import engine_generation as E
    reads = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(1), real_cpu(self, *a, **k))[1])
    inf, nan = float("inf"), float("nan")
    groups = {"offsets": torch.tensor([0, 7, 1 << 40, (1 << 53) - 1, -3], dtype=torch.int64),
              "counts": torch.tensor([5, -9, (1 << 31) - 1, -(1 << 31)], dtype=torch.int32),
              "cd": torch.tensor([1.5, inf, -inf, nan, 0.1, 5e-324, 1.7976931348623157e308], dtype=torch.float64),
              "empty": torch.zeros(0, dtype=torch.float64),
              "stats": torch.tensor([[0.5, 0.25, 1.0], [nan, nan, nan]], dtype=torch.float64)}
    pack = E._HostPack()
    for name, t in groups.items():
        pack.add(name, t)
    metrics = {k: torch.tensor([[i, 0.5], [nan, -i]], dtype=torch.float64) for i, k in enumerate(reversed(E.PP.METRIC_KEYS))}
    pack.add("metrics", metrics)
    pack.add("not computed", None)
    assert not reads
    host = pack.read()
    assert len(reads) == 1 and list(host) == list(groups) + ["metrics"]
    for name, t in groups.items():
        assert _same(host[name], t.reshape(-1)) and len(host[name]) == t.numel(), name
    assert [int(v) for v in host["offsets"]] == groups["offsets"].tolist() and [int(v) for v in host["counts"]] == groups["counts"].tolist()
    assert _same(host["metrics"], torch.cat([metrics[k].reshape(-1) for k in E.PP.METRIC_KEYS]))   # a metrics dict: METRIC_KEYS' order, flattened
