"""First-return scans above the kernel: KLAutoEncoder.cast_rays against the replay of tests/test_gpu_ae_rays.py run
through vae.decode, and engine_generation.scan_point_clouds against the existing transforms and metrics applied to cast_rays' outputs.

Fixture: a depth-1 KLAutoEncoder (256 wide, 128 latents) on seeded weights, B = 2 seeded latents, 16 x 8 beams over the whole field of
view, S = 32, n_refine = 6.  Random weights give one-signed logits, so the output bias is moved (as test_gpu_oriented_points.py moves it)
by the median over the beams of the largest logit along the beam: about half of the beams then return."""
import math

import pytest
import torch

from test_gpu_ae_rays import _assert_equal, _march_logits, _replay, _same
from test_gpu_infer_batch import PC_RANGE, _tail_args

gpu = pytest.mark.gpu
S, N_REFINE, N_AZ, N_EL = 32, 6, 16, 8
_FX = {}


def _fixture():
    if not _FX:
        from rald_amd import models_ae as A, query_points as QP, synth, weights
        args = _tail_args(1000, 256)
        az, el = QP.beam_grid(-80.0, 80.0, N_AZ, -18.0, 18.0, N_EL)
        o, d = QP.beam_segments(args, az, el)
        z = synth.latents(range(2))[:, :128].contiguous().cuda()

        def build(shift):
            m = A.KLAutoEncoder(depth=1, dim=256, queries_dim=256, num_latents=128, latent_dim=32, num_inputs=1000, query_type="mix")
            sd = weights.make_state_dict(weights.spec_of_state_dict(m.state_dict()), 0)
            sd["to_outputs.bias"] = sd["to_outputs.bias"] - shift
            m.load_state_dict(sd, strict=True)
            return m.cuda().eval()
        plain = build(0.0)
        lg = _march_logits(_dc(plain, z), o.cpu(), d.cpu(), S)                               # [S+1,B,R]
        top = lg.max(0).values
        _FX.update(args=args, az=az, el=el, o=o, d=d, z=z, vae=build(float(top.median())), empty=build(float(lg.max()) + 1.0))
    return _FX


def _dc(vae, z):
    return dict(x=z, decode=lambda pts: vae.decode(z, pts).squeeze(-1))


@gpu
def test_cast_rays_equals_the_replay_through_decode():
    """t, logit, step and points torch.equal to the replay whose logits come from vae.decode on the same latents (the memoised context),
    for the shared beam table and for the same table given per sample; without `points` the first three are the same.  Hit share asserted
    in [10 %, 90 %]."""
    fx = _fixture()
    vae, z, o, d = fx["vae"], fx["z"], fx["o"], fx["d"]
    want = _replay(_dc(vae, z), o.cpu(), d.cpu(), S, N_REFINE)
    got = vae.cast_rays(z, o, d, S, N_REFINE)
    assert got[0].shape == (2, N_AZ * N_EL) and got[2].dtype == torch.int32 and got[3].shape == (2, N_AZ * N_EL, 3)
    _assert_equal([g.cpu() for g in got], want, "shared")
    per = vae.cast_rays(z, o[None].expand(2, -1, -1).contiguous(), d[None].expand(2, -1, -1).contiguous(), S, N_REFINE)
    _assert_equal([g.cpu() for g in per], want, "per sample")
    three = vae.cast_rays(z, o, d, S, N_REFINE, points=False)
    assert len(three) == 3
    _assert_equal([g.cpu() for g in three], want[:3], "no points")
    share = float((want[2] >= 0).float().mean())
    print(f"hit share {share:.3f}, crossing share {float((want[2] >= 1).float().mean()):.3f}")
    assert 0.10 <= share <= 0.90
    with pytest.raises(ValueError):
        vae.cast_rays(z, o, d[:-1], S, N_REFINE)
    with pytest.raises(ValueError):
        vae.cast_rays(z, o[None].expand(3, -1, -1).contiguous(), d[None].expand(3, -1, -1).contiguous(), S, N_REFINE)


@gpu
def test_scan_point_clouds_is_the_existing_tail_on_the_returns():
    """'pred' equals the existing compaction + un-normalisation + polar2cartesian of cast_rays' points, frame by frame and bit for bit;
    'range' is the r column of inverse_norm_points on them (NaN without a return) and lies within 2e-5 relative of r_min + t (r_max -
    r_min); 'beam_index', the counts and 'n_queries' are consistent; 'cd' is cal_metrics of the frame (1e-6 relative; the ragged and the
    single-frame sums differ in order); with metric_thresholds the per-frame dicts carry the same cd; hit share in [10 %, 90 %]."""
    from rald_amd import engine_generation as E, postprocess as PP
    fx = _fixture()
    vae, z, args = fx["vae"], fx["z"], fx["args"]
    R = N_AZ * N_EL
    surf = (torch.rand(2, 500, 3, generator=torch.Generator().manual_seed(9)) * 2 - 1).cuda()
    out = E.scan_point_clouds(vae, z, args, fx["az"], fx["el"], S, N_REFINE, surfaces=surf)
    t, lg, st, pts = vae.cast_rays(z, fx["o"], fx["d"], S, N_REFINE)
    assert set(out) == {"pred", "range", "beam_index", "cd", "n_queries"} and out["n_queries"] == [R * (S + 1 + N_REFINE)] * 2
    assert out["range"].shape == (2, R) and len(out["pred"]) == len(out["beam_index"]) == len(out["cd"]) == 2
    polar = PP.inverse_norm_points(pts.reshape(-1, 3), PC_RANGE, True, False).view(2, R, 3)
    gt = PP.polar2cartesian(PP.inverse_norm_points(surf.reshape(-1, 3), PC_RANGE, True, False)).view(2, 500, 3)
    total = 0
    for b in range(2):
        hit = st[b] >= 0
        n = int(hit.sum())
        total += n
        want = PP.polar2cartesian(PP.occupied_points(lg[b], pts[b], PC_RANGE, True, False, view_cone_mode=False))
        assert out["pred"][b].shape == (n, 3) and torch.equal(out["pred"][b], want), b
        assert torch.equal(out["beam_index"][b], torch.nonzero(hit)[:, 0])
        assert _same(out["range"][b].cpu(), torch.where(hit, polar[b, :, 0], torch.full_like(polar[b, :, 0], float("nan"))).cpu())
        r_lin = PC_RANGE[0] + t[b][hit].double() * (PC_RANGE[3] - PC_RANGE[0])
        assert float((out["range"][b][hit].double() - r_lin).abs().max()) <= 2e-5 * PC_RANGE[3]
        # the cartesian point lies on its beam: its norm is the range
        assert float((out["pred"][b].double().norm(dim=1) - out["range"][b][hit].double()).abs().max()) <= 1e-4
        cd = PP.cal_metrics(out["pred"][b], gt[b])
        assert math.isfinite(cd) and abs(out["cd"][b] - cd) <= 1e-6 * cd, (b, out["cd"][b], cd)
    share = total / (2 * R)
    print(f"hit share {share:.3f}")
    assert 0.10 <= share <= 0.90
    more = E.scan_point_clouds(vae, z, args, fx["az"], fx["el"], S, N_REFINE, surfaces=surf, metric_thresholds=(0.5, 2.0))
    assert len(more["metrics"]) == 2
    for b in range(2):
        assert torch.equal(more["pred"][b], out["pred"][b])
        assert abs(more["metrics"][b]["cd"] - out["cd"][b]) <= 1e-6 * out["cd"][b] and len(more["metrics"][b]["f_score"]) == 2
    none = E.scan_point_clouds(vae, z, args, fx["az"], fx["el"], S, N_REFINE)
    assert none["cd"] is None and torch.equal(none["pred"][1], out["pred"][1])


@gpu
def test_scan_normals_are_unit_or_zero():
    """normals=True: one vector per returned point, of length 1 (to 2^-22) or exactly zero; the points are those of the plain scan up to
    the rounding of the fused transform (1e-4 m), the beams the same."""
    from rald_amd import engine_generation as E
    fx = _fixture()
    vae, z, args = fx["vae"], fx["z"], fx["args"]
    plain = E.scan_point_clouds(vae, z, args, fx["az"], fx["el"], S, N_REFINE)
    out = E.scan_point_clouds(vae, z, args, fx["az"], fx["el"], S, N_REFINE, normals=True)
    for b in range(2):
        n = out["normals"][b]
        assert n.shape == out["pred"][b].shape == plain["pred"][b].shape and torch.equal(out["beam_index"][b], plain["beam_index"][b])
        assert float((out["pred"][b] - plain["pred"][b]).abs().max()) <= 1e-4
        length = n.double().norm(dim=1)
        zero = (n == 0).all(dim=1)
        assert bool(((length - 1).abs() <= 2.0 ** -22)[~zero].all()) and int((~zero).sum()) >= 1


@gpu
def test_a_frame_without_returns_is_empty_with_infinite_chamfer():
    """The same weights with the bias below every logit along every beam: no beam returns; 'pred' and 'beam_index' are empty, 'range' all
    NaN, cd = inf, also with normals."""
    from rald_amd import engine_generation as E
    fx = _fixture()
    surf = (torch.rand(2, 100, 3, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    for normals in (False, True):
        out = E.scan_point_clouds(fx["empty"], fx["z"], fx["args"], fx["az"], fx["el"], S, N_REFINE, surfaces=surf, normals=normals)
        for b in range(2):
            assert out["pred"][b].shape == (0, 3) and out["beam_index"][b].numel() == 0 and out["cd"][b] == float("inf")
        assert bool(torch.isnan(out["range"]).all())
