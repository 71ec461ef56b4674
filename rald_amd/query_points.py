"""Query generation + refine on the device: the numpy code the reference runs on
the host between ``model.sample`` and ``vae.decode`` (engine_generation.py:250-300), with the same
function names and argument meaning as ``utils/utils.py`` (``generate_query_points``, ``norm_points``,
``remove_points_outside_fov``) and ``datasets/utils/query_helper.py`` (``aug_query_helper``), returning
CUDA tensors through ``rald_query_*`` (include/rald_hip.h).

Random numbers: ``rng=None`` replays the reference's draws from numpy's GLOBAL RNG in the reference's
order, so ``np.random.seed(s)`` gives bit-identical queries (the draws are uploaded, the arithmetic runs
on the device); ``rng=torch.Generator(device)`` draws on the device instead (same distribution,
different stream, no host work).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._handles import _doubles, _f32c, _need_cuda, _opt, _ragged_batch, _stream
from ._lib import check, lib

Rng = Optional[torch.Generator]


def _uniform(shape, device, rng: Rng) -> torch.Tensor:
    """float64 U[0,1): numpy's global stream (reference order) or a device generator."""
    if rng is None:
        return torch.from_numpy(np.random.random_sample(shape)).to(device)
    return torch.rand(shape, dtype=torch.float64, device=device, generator=rng)


def _device(device, rng: Rng) -> torch.device:
    if device is None:
        device = rng.device if rng is not None else "cuda"
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("rald_amd.query_points runs on the HIP device only (no CPU fallback)")
    return device


def generate_query_points(args, coordinate_type: str = "polar", device=None, rng: Rng = None) -> torch.Tensor:
    """utils/utils.py:147-175 -> float32 [num_query_points, 3] on the device (the reference's
    ``.astype('float32')`` of engine_generation.py:259 included)."""
    n = int(args.eval.inference.num_query_points)
    lidar = args.dataset.lidar
    if coordinate_type == "polar":
        pc_range = lidar.pc_range
    elif coordinate_type == "cart":
        pc_range = lidar.pc_range_cart
    else:
        raise ValueError("coordinate_type must be 'polar' or 'cart'")
    return uniform_queries(n, pc_range, lidar.norm_anisotropy, lidar.norm_isotropy, device, rng)


def uniform_queries(n: int, pc_range, norm_anisotropy: bool, norm_isotropy: bool, device=None, rng: Rng = None) -> torch.Tensor:
    device = _device(device, rng)
    if not (norm_anisotropy or norm_isotropy):
        raise ValueError("one of norm_anisotropy / norm_isotropy is required")
    u = _uniform((3, n), device, rng)                          # x draws, then y, then z - numpy's order
    out = torch.empty(n, 3, device=device, dtype=torch.float32)
    check(lib().rald_query_uniform(u.data_ptr(), n, _doubles(pc_range, 6, "pc_range"), int(norm_anisotropy), int(norm_isotropy),
                                   out.data_ptr(), _stream()))
    return out


def uniform_queries_from(u3n: torch.Tensor, pc_range, norm_anisotropy: bool, norm_isotropy: bool) -> torch.Tensor:
    """uniform_queries on given uniforms: u3n float64 [3,n] on the device (numpy's draw order) -> float32 [n,3]."""
    _need_cuda(u3n, "u3n")
    u3n = u3n.contiguous()
    n = u3n.shape[1]
    out = torch.empty(n, 3, device=u3n.device, dtype=torch.float32)
    check(lib().rald_query_uniform(u3n.data_ptr(), n, _doubles(pc_range, 6, "pc_range"), int(norm_anisotropy), int(norm_isotropy),
                                   out.data_ptr(), _stream()))
    return out


def cart_queries_from_uniform_device(u3n: torch.Tensor, args):
    """generate_cart_query_points on given uniforms, without its readback: -> (queries float32 [n,3], count int64 [1]), both on the
    device; the first `count` rows are the queries inside the field of view, in draw order."""
    _need_cuda(u3n, "u3n")
    u3n = u3n.contiguous()
    n, dev = u3n.shape[1], u3n.device
    lidar = args.dataset.lidar
    out = torch.empty(n, 3, device=dev, dtype=torch.float32)
    cnt = torch.zeros(1, device=dev, dtype=torch.int64)
    scratch = torch.empty(lib().rald_post_scratch_bytes(n), device=dev, dtype=torch.uint8)
    check(lib().rald_query_uniform_cart(u3n.data_ptr(), n, _doubles(lidar.pc_range_cart, 6, "pc_range_cart"), _doubles(lidar.pc_range, 6, "pc_range"),
                                        int(lidar.norm_anisotropy), int(lidar.norm_isotropy), out.data_ptr(), cnt.data_ptr(),
                                        scratch.data_ptr(), _stream()))
    return out, cnt


def generate_cart_query_points(args, device=None, rng: Rng = None) -> torch.Tensor:
    """The ``use_cart_query`` branch of engine_generation.py:251-256: uniform in the cartesian box,
    mapped to normalised polar coordinates, FoV-filtered -> float32 [n_kept, 3]."""
    device = _device(device, rng)
    n = int(args.eval.inference.num_query_points)
    lidar = args.dataset.lidar
    if not (lidar.norm_anisotropy or lidar.norm_isotropy):
        raise ValueError("one of norm_anisotropy / norm_isotropy is required")
    u = _uniform((3, n), device, rng)
    out = torch.empty(n, 3, device=device, dtype=torch.float32)
    cnt = torch.zeros(1, device=device, dtype=torch.int64)
    scratch = torch.empty(lib().rald_post_scratch_bytes(n), device=device, dtype=torch.uint8)
    check(lib().rald_query_uniform_cart(u.data_ptr(), n, _doubles(lidar.pc_range_cart, 6, "pc_range_cart"), _doubles(lidar.pc_range, 6, "pc_range"),
                                        int(lidar.norm_anisotropy), int(lidar.norm_isotropy), out.data_ptr(), cnt.data_ptr(),
                                        scratch.data_ptr(), _stream()))
    return out[:int(cnt.item())]


def norm_points(points: torch.Tensor, lidar_pc_range, norm_anisotropy: bool, norm_isotropy: bool) -> torch.Tensor:
    """utils/utils.py:77-104 on a float32 CUDA tensor [N,3]."""
    _need_cuda(points, "points")
    points = _f32c(points).reshape(-1, 3)
    out = torch.empty_like(points)
    check(lib().rald_query_norm_points(points.data_ptr(), points.shape[0], _doubles(lidar_pc_range, 6, "pc_range"), int(norm_anisotropy),
                                       int(norm_isotropy), out.data_ptr(), _stream()))
    return out


def remove_points_outside_fov(points: torch.Tensor) -> torch.Tensor:
    """utils/utils.py:106-112 (plumbing: a torch mask on the device; the fused form is generate_cart_query_points)."""
    return points[((points > -1) & (points < 1)).all(dim=1)]


def aug_query_helper(helper_points: torch.Tensor, aug_num: int, pc_range, voxel_size, aug_bias_scale: int = 2, rng: Rng = None,
                     norm: Optional[Sequence[bool]] = None) -> torch.Tensor:
    """datasets/utils/query_helper.py:3-42 -> float32 [aug_num, 3].  ``norm=(norm_anisotropy, norm_isotropy)``
    fuses the ``norm_points`` that engine_generation.py:295-296 applies next."""
    _need_cuda(helper_points, "helper_points")
    if helper_points.dim() != 2 or helper_points.shape[1] != 3:
        raise AssertionError("helper_points must be [N,3]")      # the reference asserts
    helper_points = _f32c(helper_points)
    dev = helper_points.device
    N, aug_num = helper_points.shape[0], int(aug_num)
    gen = aug_num - N
    sel = scales = u = None
    if gen > 0:
        if N == 0:
            raise ValueError("a must be greater than 0 unless no samples are taken")   # np.random.choice(0, ...) in the reference
        if rng is None:                                          # the reference's three draws, in its order
            sel = torch.from_numpy(np.random.choice(N, size=gen, replace=True).astype(np.int64)).to(dev)
            scales = torch.from_numpy(np.random.choice(np.arange(aug_bias_scale, step=1) + 1, size=gen).astype(np.int64)).to(dev)
            u = torch.from_numpy(np.random.rand(gen, 3)).to(dev)
        else:
            sel = torch.randint(0, N, (gen,), device=dev, generator=rng, dtype=torch.int64)
            scales = torch.randint(1, int(aug_bias_scale) + 1, (gen,), device=dev, generator=rng, dtype=torch.int64)
            u = torch.rand((gen, 3), dtype=torch.float64, device=dev, generator=rng)
    out = torch.empty(aug_num, 3, device=dev, dtype=torch.float32)
    aniso, iso = (bool(norm[0]), bool(norm[1])) if norm is not None else (False, False)
    check(lib().rald_query_refine(helper_points.data_ptr(), N, aug_num, _opt(sel), _opt(scales), _opt(u), _doubles(pc_range, 6, "pc_range"),
                                  _doubles(voxel_size, 3, "voxel_size"), int(aniso), int(iso), int(norm is not None), out.data_ptr(), _stream()))
    return out


def refine_queries(pred_points: torch.Tensor, args, rng: Rng = None) -> torch.Tensor:
    """engine_generation.py:292-297: jittered copies of the positive (un-normalised polar) points,
    normalised again -> [refine_query_aug_num, 3] ready for ``vae.decode``."""
    inf, lidar = args.eval.inference, args.dataset.lidar
    return aug_query_helper(pred_points, int(inf.refine_query_aug_num), lidar.pc_range, lidar.voxel_size, inf.refine_query_scale, rng,
                            norm=(lidar.norm_anisotropy, lidar.norm_isotropy))


def draw_tail_randoms(B: int, n_grid: int, aug_num: int, aug_bias_scale: int, generator: torch.Generator) -> dict:
    """Every random number the inference tail of a batch of B frames consumes, drawn from a DEVICE generator before anything is
    decoded: 'u3n' float64 [3,n_grid] (the query grid the frames share), and per frame the refine draws 'u_sel' float64 [B,aug_num]
    in [0,1) (row g selects point min(floor(u_sel * N_b), N_b - 1) once N_b is known - on the device), 'scales' int64 [B,aug_num]
    in 1 .. aug_bias_scale and 'u_bias' float64 [B,aug_num,3]."""
    if generator is None or torch.device(generator.device).type != "cuda":
        raise ValueError("draw_tail_randoms needs a torch.Generator of the GPU")
    dev = generator.device
    B, n_grid, aug_num = int(B), int(n_grid), int(aug_num)
    return {"u3n": torch.rand((3, n_grid), dtype=torch.float64, device=dev, generator=generator),
            "u_sel": torch.rand((B, aug_num), dtype=torch.float64, device=dev, generator=generator),
            "scales": torch.randint(1, int(aug_bias_scale) + 1, (B, aug_num), device=dev, generator=generator, dtype=torch.int64),
            "u_bias": torch.rand((B, aug_num, 3), dtype=torch.float64, device=dev, generator=generator)}


def aug_query_helper_ragged(points: torch.Tensor, offsets: torch.Tensor, aug_num: int, pc_range, voxel_size, draws: dict,
                            norm: Optional[Sequence[bool]] = None):
    """aug_query_helper for a ragged batch: points [T,3], offsets int64 [B+1] on the device, draws = 'scales' [B,aug_num],
    'u_bias' [B,aug_num,3] and either 'sel' int64 [B,aug_num] or 'u_sel' float64 [B,aug_num] (draw_tail_randoms) ->
    (queries [B*aug_num,3], out_offsets int64 [B+1]): a frame with points gets aug_num rows, a frame without points gets none (the
    single-frame call raises there), the frames packed one behind the other.  No host read."""
    _need_cuda(points, "points")
    points = _f32c(points).reshape(-1, 3)
    dev = points.device
    B, aug_num = _ragged_batch(offsets, "offsets"), int(aug_num)
    sel, u_sel = draws.get("sel"), draws.get("u_sel")
    if sel is None and u_sel is None:
        raise ValueError("draws needs 'sel' or 'u_sel'")

    def field(t, dtype, shape, name):
        if t is None:
            return None
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_cuda:
            raise ValueError(f"draws[{name!r}] must be a {dtype} tensor of shape {shape} on the GPU")
        return t.contiguous()
    sel = field(sel, torch.int64, (B, aug_num), "sel")
    u_sel = field(u_sel, torch.float64, (B, aug_num), "u_sel") if sel is None else None
    scales = field(draws["scales"], torch.int64, (B, aug_num), "scales")
    u_bias = field(draws["u_bias"], torch.float64, (B, aug_num, 3), "u_bias")
    out = torch.empty(B * aug_num, 3, device=dev, dtype=torch.float32)
    out_offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    aniso, iso = (bool(norm[0]), bool(norm[1])) if norm is not None else (False, False)
    check(lib().rald_query_refine_ragged(points.data_ptr(), offsets.data_ptr(), B, aug_num, _opt(sel), _opt(u_sel), scales.data_ptr(),
                                         u_bias.data_ptr(), _doubles(pc_range, 6, "pc_range"), _doubles(voxel_size, 3, "voxel_size"),
                                         int(aniso), int(iso), int(norm is not None), out.data_ptr(), out_offsets.data_ptr(), _stream()))
    return out, out_offsets


def refine_queries_ragged(points: torch.Tensor, offsets: torch.Tensor, args, draws: dict):
    """refine_queries for a ragged batch of positive (un-normalised polar) points -> (queries [B*refine_query_aug_num,3] normalised,
    out_offsets int64 [B+1]) ready for ``vae.decode_ragged``."""
    inf, lidar = args.eval.inference, args.dataset.lidar
    return aug_query_helper_ragged(points, offsets, int(inf.refine_query_aug_num), lidar.pc_range, lidar.voxel_size, draws,
                                   norm=(lidar.norm_anisotropy, lidar.norm_isotropy))


def project_to_surface_ragged(vae, z_or_ctx: torch.Tensor, points_norm: torch.Tensor, offsets: torch.Tensor, max_per_sample: int,
                              steps: int = 3, max_step: float = 0.05):
    """Moves normalised points onto the decoder's surface (logit = 0) by `steps` clamped Newton steps along the logit's gradient, one
    gradient-decode launch per step (KLAutoEncoder.decode_ragged_with_gradient with project=True, each launch fed the previous one's
    projected points), then one more gradient launch at the final positions: -> (points_norm [T,3], logits [T], grad [T,3]), the
    logits and gradients OF the returned points.  z_or_ctx: the latents [B,M,C] (the autoencoder's memoised context is used) or a
    decoder context from AeHandle.decode_latents (uint8).  Ragged layout as decode_ragged; nothing is read back.  The refine pass of
    the reference only keeps jittered copies that stay positive; this uses where the decoder says the surface is."""
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    is_ctx = z_or_ctx.dtype == torch.uint8

    def decode(pts, project):
        if is_ctx:
            with torch.no_grad():
                return vae._handle().decode_queries_grad_ragged(z_or_ctx, pts, offsets, max_per_sample, project, max_step)
        return vae.decode_ragged_with_gradient(z_or_ctx, pts, offsets, max_per_sample, project, max_step)

    pts = _f32c(points_norm).reshape(-1, 3)
    for _ in range(steps):
        pts = decode(pts, True)[2]
    logits, grad = decode(pts, False)
    return pts, logits, grad



def beam_grid(az_min: float, az_max: float, n_az: int, el_min: float, el_max: float, n_el: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The beam directions of a spinning sensor: n_az azimuths from az_min to az_max and n_el elevations from el_min to el_max (degrees,
    both ends included, evenly spaced; a count of 1 takes the minimum) -> (az_deg [n], el_deg [n]) float64 on the host, n = n_el * n_az,
    elevation-major: beam i has elevation i // n_az and azimuth i % n_az."""
    n_az, n_el = int(n_az), int(n_el)
    if n_az < 1 or n_el < 1:
        raise ValueError("n_az and n_el must be at least 1")
    az = torch.linspace(float(az_min), float(az_max), n_az, dtype=torch.float64)
    el = torch.linspace(float(el_min), float(el_max), n_el, dtype=torch.float64)
    return az.repeat(n_el), el.repeat_interleave(n_az)


def _beam_tables(args, az_deg, el_deg):
    """beam_segments' host checks -> (az, el) float32 [n]: ValueError before any GPU work"""
    lidar = args.dataset.lidar
    view_cone = lidar.get("view_cone_mode", False) if hasattr(lidar, "get") else getattr(lidar, "view_cone_mode", False)
    if not view_cone:
        raise ValueError("beam_segments needs view_cone_mode: the field must live in (r, az, el) for a beam to be a straight segment")
    if not (lidar.norm_anisotropy or lidar.norm_isotropy):
        raise ValueError("one of norm_anisotropy / norm_isotropy is required")
    az, el = torch.as_tensor(az_deg), torch.as_tensor(el_deg)
    if az.dim() != 1 or el.dim() != 1 or az.numel() != el.numel() or az.numel() < 1:
        raise ValueError("az_deg and el_deg must be two vectors of the same length >= 1, one entry per beam")
    return az.to(torch.float32), el.to(torch.float32)


def beam_segments(args, az_deg, el_deg, r_min: Optional[float] = None, r_max: Optional[float] = None, device=None):
    """Sensor beams as segments of the decoder's normalised coordinates (view-cone mode: the field lives in (r, az deg, el deg), so the
    beam of direction (az, el) is the axis-0 segment from (r_min, az, el) to (r_max, az, el)): az_deg / el_deg [n] (beam_grid) ->
    (origins [n,3], dirs [n,3]) on the device, origins = norm_points(start), dirs = norm_points(end) - norm_points(start).  r_min /
    r_max default to pc_range[0] / pc_range[3].  ValueError outside view-cone mode and on shape errors, before any GPU work."""
    az, el = _beam_tables(args, az_deg, el_deg)
    lidar = args.dataset.lidar
    r0 = float(lidar.pc_range[0] if r_min is None else r_min)
    r1 = float(lidar.pc_range[3] if r_max is None else r_max)
    if not (r1 > r0):
        raise ValueError("r_max must be greater than r_min")
    dev = _device(device, None)
    az, el = az.to(dev), el.to(dev)
    start = norm_points(torch.stack((torch.full_like(az, r0), az, el), dim=1), lidar.pc_range, lidar.norm_anisotropy, lidar.norm_isotropy)
    end = norm_points(torch.stack((torch.full_like(az, r1), az, el), dim=1), lidar.pc_range, lidar.norm_anisotropy, lidar.norm_isotropy)
    return start, end - start


def field_grid(resolution) -> Tuple[Tuple[float, ...], Tuple[float, ...], Tuple[int, ...]]:
    """The node grid over the decoder's normalised box [-1, 1]^3 -> (lo, spacing, dims): `resolution` nodes per axis (an int, or one per
    axis; 2 .. 1024 each), the first at -1 and the last at 1 up to float32 rounding: spacing = float32(2 / (n - 1))."""
    from .postprocess import SURFACE_MAX_DIM, _f32
    res = (resolution,) * 3 if isinstance(resolution, int) and not isinstance(resolution, bool) else resolution
    try:
        ok = len(res) == 3 and all(isinstance(n, int) and not isinstance(n, bool) and 2 <= n <= SURFACE_MAX_DIM for n in res)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"resolution must be an integer, or three, in 2 .. {SURFACE_MAX_DIM}")
    return (-1.0, -1.0, -1.0), tuple(_f32(2.0 / (n - 1)) for n in res), tuple(int(n) for n in res)


def _grid_planes(dims3, i0, ni):
    i0 = int(i0)
    ni = dims3[0] - i0 if ni is None else int(ni)
    if i0 < 0 or ni < 1 or i0 + ni > dims3[0]:
        raise ValueError("planes i0 .. i0 + ni - 1 must lie in 0 .. nx - 1")
    return i0, ni


def grid_queries(lo, spacing, dims, i0: int = 0, ni: Optional[int] = None, device=None) -> torch.Tensor:
    """The nodes of x-planes i0 .. i0 + ni - 1 (default: all) of a regular grid -> float32 [ni * ny * nz, 3] on the device, z fastest:
    node (i, j, k) at lo + (i, j, k) * spacing, each product and sum rounded once in float32 (rald_query_grid) - the positions
    postprocess.extract_surface_batch gives the values of a volume [nx, ny, nz]."""
    import ctypes as C
    from .postprocess import _grid_spec
    lo3, h3, dims3 = _grid_spec(lo, spacing, dims)
    i0, ni = _grid_planes(dims3, i0, ni)
    device = _device(device, None)
    out = torch.empty(ni * dims3[1] * dims3[2], 3, device=device, dtype=torch.float32)
    with torch.cuda.device(device):
        check(lib().rald_query_grid((C.c_float * 3)(*lo3), (C.c_float * 3)(*h3), (C.c_int32 * 3)(*dims3), i0, ni, out.data_ptr(), _stream()))
    return out
