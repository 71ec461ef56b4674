"""Python owners of the C handles: device-memory plumbing (torch tensors -> raw pointers, the
current torch stream -> hipStream_t) around librald_hip.so.  No arithmetic happens here.

Calls into the library pass `t.data_ptr()` for a tensor, None for NULL (`_opt` for an optional tensor), a numpy array's
`.ctypes.data` for host memory and `_stream()` for the stream: the binding (_lib.py) declares every pointer as c_void_p."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import DitConfig, check, lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _opt(t: Optional[torch.Tensor]) -> Optional[int]:
    """Pointer argument of an optional tensor: None (NULL) when it is absent."""
    return t.data_ptr() if t is not None else None


def _need_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"rald_amd: {what} must live on the GPU (cuda tensor); this package has no CPU path")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _nbytes(n: int) -> int:
    """A size from a rald_*_workspace_bytes query; a negative one means the library refused the configuration."""
    if n < 0:
        check(1)
    return n


def _cached_workspace(cache: Dict[torch.device, torch.Tensor], nbytes: int, device) -> torch.Tensor:
    """The uint8 workspace of `device` in `cache`, kept between calls and grown to `nbytes` on demand."""
    ws = cache.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = cache[device] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _scratch(nbytes: int, device) -> torch.Tensor:
    """A uint8 scratch buffer for one call, at least 16 bytes, so its pointer is never NULL."""
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


def _doubles(vals: Sequence[float], n: int, what: str, layout: str = "") -> C.Array:
    """A host double[n] argument (Python floats of the reference's YAML -> doubles)."""
    if len(vals) != n:
        raise ValueError(f"{what} must have {n} elements{layout}")
    return (C.c_double * n)(*[float(v) for v in vals])


def _ragged_batch(offsets: torch.Tensor, what: str) -> int:
    """B of a ragged layout's offsets: a contiguous int64 [B+1] DEVICE tensor (checked by shape and dtype only: its values stay on the device)."""
    if not (isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.dtype == torch.int64 and offsets.dim() == 1
            and offsets.numel() >= 2 and offsets.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous int64 [B+1] tensor on the GPU")
    return offsets.numel() - 1


class _Handle:
    """Owner of one rald_<kind>* handle: created from `args` by rald_<kind>_create, destroyed by rald_<kind>_destroy when the owner
    drops it.  `_h` is the handle itself (a c_void_p) for the calls."""

    def __init__(self, kind: str, *args):
        self._kind = kind
        self._h = C.c_void_p()
        check(getattr(lib(), f"rald_{kind}_create")(*args, C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                getattr(lib(), f"rald_{self._kind}_destroy")(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def load(self, named: Iterable[Tuple[str, torch.Tensor]], fn: str = "load_weight", finalize: bool = True) -> None:
        """rald_<kind>_<fn>(name, fp32 data, nelem) for every (name, tensor), then rald_<kind>_finalize."""
        put = getattr(lib(), f"rald_{self._kind}_{fn}")
        for name, t in named:
            t = _f32c(t)                       # host or device fp32; the library stages either
            check(put(self._h, name.encode(), t.data_ptr(), t.numel()))
        if finalize:
            check(getattr(lib(), f"rald_{self._kind}_finalize")(self._h))


# Launch-bound regime (small batches): one sampler run is ~10 000 kernel launches of a few
# microseconds each, so the whole call is captured once into a hipGraph (torch.cuda.CUDAGraph on
# the current stream - the library only enqueues kernels on the stream it is given) and replayed.
# RALD_GRAPH=0 disables it; batches above GRAPH_MAX_BATCH run eagerly (they are GPU-bound).
GRAPH_MAX_BATCH = int(os.environ.get("RALD_GRAPH_MAX_BATCH", "16"))


def _graphs_enabled() -> bool:
    return os.environ.get("RALD_GRAPH", "1") != "0"


class _GraphCache:
    """key -> (CUDAGraph, static inputs, static outputs, workspace generation).  Everything a captured graph points at
    (handle workspace, sigma table, static tensors) must stay put.  The library may reallocate its workspace inside ANY
    call (a larger batch through denoise / encode_cond / forward), so every replay first compares the handle's
    workspace generation (rald_*_workspace_generation) with the one recorded after capture and re-captures on a
    mismatch; owners additionally call clear() when something on the Python side changes."""

    def __init__(self, generation=lambda: 0):
        self.entries: Dict[tuple, tuple] = {}
        self.generation = generation

    def clear(self):
        self.entries.clear()

    def run(self, key, inputs, make_outputs, fn):
        ent = self.entries.get(key)
        if ent is not None and ent[3] != self.generation():      # the workspace moved since capture: the graph is stale
            del self.entries[key]
            ent = None
        if ent is None:
            static_in = [t.clone() for t in inputs]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                   # warm-up outside capture: lazy allocations,
                outs = make_outputs()                       # function attributes, sigma tables
                fn(static_in, outs)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs = make_outputs()
                fn(static_in, outs)
            ent = (g, static_in, outs, self.generation())
            self.entries[key] = ent
        g, static_in, outs, _ = ent
        for dst, src in zip(static_in, inputs):
            dst.copy_(src, non_blocking=True)
        g.replay()
        return [o.clone() for o in outs]


class DitHandle(_Handle):
    """rald_dit* + its condition cache.  One handle per module per device."""

    def __init__(self, cfg: DitConfig):
        self.cfg = cfg
        super().__init__("dit", C.byref(cfg))
        self._graphs = _GraphCache(lambda: lib().rald_dit_workspace_generation(self._h))
        self._reserved = 0
        self._sched = None
        self._sched_churn = None
        # Two-stream schedule of an NFE between 128 and 255 samples: which of the two bit-identical schedules is faster depends on the box
        # (clocks under MFMA load differ by ~6 % across the pool; two interleaved half-batches measured +2.5 % on slower boxes and -1.5 % on the
        # fastest).  Opt-in: with autotune_two_stream = True the first NFE of such a batch times both (eight NFEs each way, once per handle
        # and batch size) and keeps the winner; off by default - the library's fixed threshold (256) then decides, and a profile of the process
        # shows one schedule only.  An explicit set_two_stream_min_batch() also turns it off.
        self.autotune_two_stream = False
        self._two_stream_tuned = {}

    def set_sigmas(self, sigmas) -> None:
        s = [float(v) for v in sigmas]
        arr = (C.c_float * len(s))(*s)
        check(lib().rald_dit_set_sigmas(self._h, arr, len(s), _stream()))

    def new_cache(self, batch: int, device) -> torch.Tensor:
        nbytes = lib().rald_dit_cond_cache_bytes(self._h, batch)
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    def encode_cond_tokens(self, tokens: torch.Tensor) -> torch.Tensor:
        _need_cuda(tokens, "condition tokens")
        tokens = _f32c(tokens)
        B, T, Cd = tokens.shape
        if T != self.cfg.n_cond_tokens or Cd != self.cfg.context_dim:
            raise RuntimeError(f"condition tokens must be [B,{self.cfg.n_cond_tokens},{self.cfg.context_dim}], got {tuple(tokens.shape)}")
        cache = self.new_cache(B, tokens.device)
        check(lib().rald_dit_encode_cond_tokens(self._h, tokens.data_ptr(), B, cache.data_ptr(), _stream()))
        return cache

    def encode_cond(self, cube: torch.Tensor, want_tokens: bool = True):
        _need_cuda(cube, "radar cube")
        cube = _f32c(cube)
        B = cube.shape[0]
        cache = self.new_cache(B, cube.device)
        tokens = None
        if want_tokens:
            tokens = torch.empty(B, self.cfg.n_cond_tokens, self.cfg.n_heads * self.cfg.d_head, device=cube.device, dtype=torch.float32)
        check(lib().rald_dit_encode_cond(self._h, cube.data_ptr(), B, _opt(tokens), cache.data_ptr(), _stream()))
        return tokens, cache

    def denoise(self, x: torch.Tensor, cache: torch.Tensor, sigma_row: int = 0, per_sample: bool = False,
                raw_F: bool = False) -> torch.Tensor:
        _need_cuda(x, "x")
        x = _f32c(x)
        if x.dim() != 3 or x.shape[1] != self.cfg.n_latents or x.shape[2] != self.cfg.channels:
            raise RuntimeError(f"x must be [B,{self.cfg.n_latents},{self.cfg.channels}], got {tuple(x.shape)}")
        if cache.dtype != torch.uint8 or not cache.is_cuda or cache.numel() != lib().rald_dit_cond_cache_bytes(self._h, x.shape[0]):
            raise RuntimeError(f"condition cache of {cache.numel()} bytes does not belong to a batch of {x.shape[0]} "
                               f"(expected {lib().rald_dit_cond_cache_bytes(self._h, x.shape[0])} bytes): encode the condition for the same batch")
        out = torch.empty_like(x)
        B = x.shape[0]
        if self.autotune_two_stream and 128 <= B < 256 and B not in self._two_stream_tuned and not torch.cuda.is_current_stream_capturing():
            self._tune_two_stream(x, cache, sigma_row, per_sample, raw_F, out)
        check(lib().rald_dit_denoise(self._h, x.data_ptr(), B, sigma_row, int(per_sample),
                                     cache.data_ptr(), out.data_ptr(), int(raw_F), _stream()))
        return out

    def _tune_two_stream(self, x, cache, sigma_row, per_sample, raw_F, out) -> None:
        """Times the whole-batch and the two-half-batch schedule of this NFE (same inputs, same bits out) and sets the library's threshold."""
        B = x.shape[0]
        prev = lib().rald_dit_two_stream_min_batch(self._h)

        def run(n):
            for _ in range(n):
                check(lib().rald_dit_denoise(self._h, x.data_ptr(), B, sigma_row, int(per_sample), cache.data_ptr(),
                                             out.data_ptr(), int(raw_F), _stream()))
        ms = {}
        for mode, mb in (("whole", 0), ("split", B)):
            self._set_two_stream(mb)
            run(2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(6)
            e1.record()
            e1.synchronize()
            ms[mode] = e0.elapsed_time(e1)
        split = ms["split"] < 0.995 * ms["whole"]
        self._two_stream_tuned[B] = (split, ms["whole"] / 6, ms["split"] / 6)
        self._set_two_stream(min(prev if prev > 0 else 256, B) if split else max(prev, B + 1))

    def _set_two_stream(self, min_batch: int) -> None:
        self._graphs.clear()                           # the workspace is re-planned
        check(lib().rald_dit_set_two_stream_min_batch(self._h, int(min_batch)))

    def set_two_stream_min_batch(self, min_batch: int) -> None:
        """From `min_batch` samples up an NFE runs as two half-batches on two HIP streams (default 256; 0 = never).  Setting it by hand
        switches the per-box choice for batches of 128-255 (see __init__) off."""
        self.autotune_two_stream = False
        self._set_two_stream(min_batch)

    def profile_begin(self) -> None:
        check(lib().rald_dit_profile_begin(self._h))

    def profile_set_kinds(self, mask: int) -> None:
        """Which kinds (bit k, see profile_end_kinds) are bracketed from now on; profile_begin resets to all four."""
        check(lib().rald_dit_profile_set_kinds(self._h, int(mask)))

    def profile_end(self):
        ms, n = C.c_double(0), C.c_int32(0)
        check(lib().rald_dit_profile_end(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_end_kinds(self):
        """[(ms, launches)] x 4: FF1 GEGLU GEMM, attn1 / attn2 output projection + residual + AdaLN (K = 512), FF2 + residual + AdaLN."""
        ms, n = (C.c_double * 4)(), (C.c_int32 * 4)()
        check(lib().rald_dit_profile_end_kinds(self._h, ms, n))
        return [(ms[i], n[i]) for i in range(4)]

    def reserve(self, batch: int) -> None:
        if batch > self._reserved:
            self._graphs.clear()                       # workspace may move: captured graphs are stale
            check(lib().rald_dit_reserve(self._h, batch))
            self._reserved = batch

    def _sample_eager(self, latents, cache, out, num_steps, sigma_min, sigma_max, rho):
        check(lib().rald_dit_sample(self._h, latents.data_ptr(), latents.shape[0], cache.data_ptr(), num_steps,
                                    sigma_min, sigma_max, rho, out.data_ptr(), _stream()))

    def sample(self, latents: torch.Tensor, cache: torch.Tensor, num_steps: int = 18, sigma_min: float = 0.002,
               sigma_max: float = 80.0, rho: float = 7.0, use_graph: Optional[bool] = None, S_churn: float = 0, S_min: float = 0,
               S_max: float = float("inf"), S_noise: float = 1, noise: Optional[torch.Tensor] = None,
               seeds: Optional[torch.Tensor] = None) -> torch.Tensor:
        _need_cuda(latents, "latents")
        latents = _f32c(latents)
        B = latents.shape[0]
        if cache.dtype != torch.uint8 or not cache.is_cuda or cache.numel() != lib().rald_dit_cond_cache_bytes(self._h, B):
            raise RuntimeError(f"condition cache of {cache.numel()} bytes does not belong to a batch of {B}: encode the condition for the same batch")
        if S_churn != 0:
            return self._sample_churn(latents, cache, num_steps, sigma_min, sigma_max, rho, use_graph, S_churn, S_min, S_max, S_noise, noise, seeds)
        self.reserve(B)
        sched = (num_steps, float(sigma_min), float(sigma_max), float(rho))
        if sched != self._sched:                       # the sampler's sigma table is rebuilt for a new schedule
            self._graphs.clear()
            self._sched = sched
        if use_graph is None:
            use_graph = _graphs_enabled() and B <= GRAPH_MAX_BATCH
        if not use_graph:
            out = torch.empty_like(latents)
            self._sample_eager(latents, cache, out, *sched)
            return out
        (out,) = self._graphs.run(("sample", B) + sched, [latents, cache], lambda: [torch.empty_like(latents)],
                                  lambda ins, outs: self._sample_eager(ins[0], ins[1], outs[0], *sched))
        return out

    def _sample_churn_eager(self, latents, cache, out, sched, noise, seeds):
        check(lib().rald_dit_sample_stochastic(self._h, latents.data_ptr(), latents.shape[0], cache.data_ptr(), *sched, _opt(noise), _opt(seeds),
                                               out.data_ptr(), _stream()))

    def _sample_churn(self, latents, cache, num_steps, sigma_min, sigma_max, rho, use_graph, S_churn, S_min, S_max, S_noise, noise, seeds):
        """edm_sampler with S_churn > 0 (rald_dit_sample_stochastic): `noise` [n_churned, B, n_latents, channels] - the churned steps'
        draws in step order - or `seeds` int64 [B] for noise generated inside the kernel (op_philox_normal's tag 1, step = i)."""
        if S_churn < 0 or S_noise < 0:
            raise ValueError("S_churn and S_noise must be >= 0")
        B = latents.shape[0]
        sched = (int(num_steps), float(sigma_min), float(sigma_max), float(rho), float(S_churn), float(S_min), float(S_max), float(S_noise))
        t, t_hat = edm_schedule(*sched[:7])
        n_churned = int((t_hat != t[:-1]).sum())
        if n_churned == 0:                             # nothing to add (the levels lie outside [S_min, S_max]): the deterministic loop
            return self.sample(latents, cache, *sched[:4], use_graph=use_graph)
        if (noise is None) == (seeds is None):
            raise ValueError(f"{n_churned} of the {num_steps} steps are churned: pass exactly one of `noise` (host-drawn) and `seeds` (device Philox)")
        if noise is not None:
            _need_cuda(noise, "noise")
            noise = _f32c(noise)
            if tuple(noise.shape) != (n_churned,) + tuple(latents.shape):
                raise ValueError(f"noise must be [{n_churned}, {B}, {self.cfg.n_latents}, {self.cfg.channels}] (the churned steps only, in order), "
                                 f"got {tuple(noise.shape)}")
            extra, mode = noise, "noise"
        else:
            if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int64 and tuple(seeds.shape) == (B,)):
                raise ValueError(f"seeds must be an int64 [{B}] tensor on the GPU")
            extra, mode = seeds.contiguous(), "seeds"
        self.reserve(B)
        if sched != self._sched_churn:                 # the stochastic sampler's sigma table is rebuilt for a new schedule
            self._graphs.clear()
            self._sched_churn = sched
        if use_graph is None:
            use_graph = _graphs_enabled() and B <= GRAPH_MAX_BATCH

        def run(lat, cc, ex, out):
            self._sample_churn_eager(lat, cc, out, sched, ex if mode == "noise" else None, ex if mode == "seeds" else None)
        if not use_graph:
            out = torch.empty_like(latents)
            run(latents, cache, extra, out)
            return out
        (out,) = self._graphs.run(("sample_churn", B, mode) + sched, [latents, cache, extra], lambda: [torch.empty_like(latents)],
                                  lambda ins, outs: run(ins[0], ins[1], ins[2], outs[0]))
        return out


def edm_schedule(num_steps: int, sigma_min: float = 0.002, sigma_max: float = 80.0, rho: float = 7.0, S_churn: float = 0, S_min: float = 0,
                 S_max: float = float("inf")):
    """(t [num_steps + 1], t_hat [num_steps]) float32 numpy arrays: the sampler's noise levels as the library computes them
    (rald_edm_schedule, host arithmetic, needs no GPU).  Step i is churned iff t_hat[i] != t[i]."""
    import numpy as np
    if int(num_steps) < 1:
        raise ValueError("num_steps must be positive")
    t, t_hat = np.zeros(int(num_steps) + 1, np.float32), np.zeros(int(num_steps), np.float32)
    check(lib().rald_edm_schedule(int(num_steps), sigma_min, sigma_max, rho, S_churn, S_min, S_max, t.ctypes.data, t_hat.ctypes.data))
    return t, t_hat


# ---- kernel-level wrappers used by the parity tests and microbenchmarks -----------------------
def op_philox_normal(seeds: torch.Tensor, n_per_sample: int, tag: int = 0, step: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """N(0,1) [B, n_per_sample] from the device generator (rald_amd/csrc/rng.hip): a pure function of (seeds[b] mod 2^32, tag, step, element).
    seeds int64 [B] on the GPU; tag 0 = initial latents, 1 = churn noise of sampler step `step`."""
    _need_cuda(seeds, "seeds")
    if seeds.dtype != torch.int64 or seeds.dim() != 1:
        raise ValueError("seeds must be an int64 [B] tensor")
    seeds = seeds.contiguous()
    B = seeds.shape[0]
    if out is None:
        out = torch.empty(B, int(n_per_sample), device=seeds.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.numel() == B * int(n_per_sample)
    check(lib().rald_op_philox_normal(seeds.data_ptr(), B, int(n_per_sample), int(tag), int(step), out.data_ptr(), _stream()))
    return out


def op_gemm_nt(A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = 0,
               C_inout: Optional[torch.Tensor] = None, alpha: float = 1.0) -> torch.Tensor:
    """A [batch?,M,K] bf16, B [batch?,N,K] bf16 -> C.  epilogue 0 bf16, 1 f32, 2 f32 accumulate into
    C_inout, 3 GEGLU (B rows / bias pre-packed), 4 softmax over aligned groups of 64 columns (exp2 units, bf16), 5 fp16 slab =
    2^-6 x the product, saturating (the split-K partial sums of the small-batch path)."""
    batched = A.dim() == 3 or B.dim() == 3
    batch = (A.shape[0] if A.dim() == 3 else B.shape[0]) if batched else 1
    M, K = A.shape[-2], A.shape[-1]
    N = B.shape[-2]
    sA = A.stride(0) if A.dim() == 3 else 0
    sB = B.stride(0) if B.dim() == 3 else 0
    nc = N // 2 if epilogue == 3 else N
    if epilogue == 2:
        out = C_inout
    else:
        shape = (batch, M, nc) if batched else (M, nc)
        out = torch.empty(shape, device=A.device, dtype=torch.float16 if epilogue == 5 else (torch.bfloat16 if epilogue in (0, 3, 4) else torch.float32))
    sC = out.stride(0) if out.dim() == 3 else 0
    check(lib().rald_op_gemm_nt(A.data_ptr(), A.stride(-2), sA, B.data_ptr(), B.stride(-2), sB, out.data_ptr(), out.stride(-2), sC, _opt(bias), M, N,
                                K, batch, alpha, epilogue, _stream()))
    return out


def op_gemm_nt_256(A: torch.Tensor, B: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = 0, alpha: float = 1.0,
                   alpha_ncols: int = 1 << 30, persistent: int = 1, max_workgroups: int = 1 << 30) -> torch.Tensor:
    """The 256 x 256 LDS-DMA tiles on one problem, whatever its tile count: A [M,K], B [N,K] bf16 (row slices allowed) into the caller's bf16
    `out` [M, N] (epilogue 0; alpha on columns < alpha_ncols) or [M, N/2] (epilogue 3, GEGLU).  persistent=1: the persistent tile loop on at
    most max_workgroups workgroups; persistent=0: the one-tile kernel."""
    (M, K), N = A.shape, B.shape[0]
    assert A.dtype == B.dtype == out.dtype == torch.bfloat16 and A.stride(1) == B.stride(1) == out.stride(1) == 1
    assert out.shape == (M, N // 2 if epilogue == 3 else N) and B.shape[1] == K
    check(lib().rald_op_gemm_nt_256(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), out.stride(0), _opt(bias), M, N, K,
                                    alpha, int(alpha_ncols), int(epilogue), int(persistent), int(max_workgroups), _stream()))
    return out


def op_gemm_nt_256_batched(A: torch.Tensor, B: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = 0,
                           alpha: float = 1.0, alpha_ncols: int = 1 << 30, persistent: int = 1, max_workgroups: int = 1 << 30) -> torch.Tensor:
    """op_gemm_nt_256 with a batch: A [batch,M,K] or [M,K] (shared), B [batch,N,K] or [N,K] (shared), into the caller's bf16 `out`
    [batch,M,N] (epilogue 0, or 4: softmax over every 64 columns of alpha * A.B^T in exp2 units) or [batch,M,N/2] (epilogue 3).  The
    persistent tile loop takes a batch for epilogue 4 only."""
    batch, M, nc = out.shape
    K, N = A.shape[-1], B.shape[-2]
    assert A.dtype == B.dtype == out.dtype == torch.bfloat16 and A.stride(-1) == B.stride(-1) == out.stride(-1) == 1
    assert A.shape[-2] == M and B.shape[-1] == K and nc == (N // 2 if epilogue == 3 else N)
    assert all(t.dim() == 2 or t.shape[0] == batch for t in (A, B))
    check(lib().rald_op_gemm_nt_256_batched(A.data_ptr(), A.stride(-2), A.stride(0) if A.dim() == 3 else 0, B.data_ptr(), B.stride(-2),
                                            B.stride(0) if B.dim() == 3 else 0, out.data_ptr(), out.stride(-2), out.stride(0), _opt(bias), M, N, K,
                                            batch, 1, alpha, int(alpha_ncols), int(epilogue), int(persistent), int(max_workgroups), _stream()))
    return out


def op_gemm_tn(A: torch.Tensor, B: torch.Tensor, C_inout: torch.Tensor, colsum: Optional[torch.Tensor] = None, atomics: bool = True) -> torch.Tensor:
    """C_inout [N1,N2] f32 += A^T.B for row-major bf16 A [M,N1], B [M,N2] (column slices allowed); colsum [N1] f32 += column sums of A.
    atomics=False: the row ranges meet in a workspace and are added in order by a second launch (bit-reproducible)."""
    M, N1 = A.shape
    N2 = B.shape[1]
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and C_inout.dtype == torch.float32 and B.shape[0] == M
    assert A.stride(1) == 1 and B.stride(1) == 1 and C_inout.stride(1) == 1 and C_inout.shape == (N1, N2)
    ws, nbytes = None, 0
    if not atomics:
        nbytes = lib().rald_op_gemm_tn_workspace_bytes(M, N1, N2)
        ws = _scratch(nbytes, A.device)
    check(lib().rald_op_gemm_tn(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C_inout.data_ptr(), C_inout.stride(0),
                                _opt(colsum), M, N1, N2, _opt(ws), nbytes, _stream()))
    return C_inout


def op_gemm_resid_ln(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, x: torch.Tensor, g: torch.Tensor, b: torch.Tensor,
                     gstride: int = 0, rows_per_group: int = 1 << 30, add_one: float = 0.0, eps: float = 1e-5) -> torch.Tensor:
    """x [M,512] f32 += A [M,K] bf16 @ W [512,K]^T + bias (in place); returns h = LN(x)*(add_one+g)+b as bf16."""
    M, K = A.shape
    h = torch.empty(M, 512, device=A.device, dtype=torch.bfloat16)
    check(lib().rald_op_gemm_resid_ln(A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), bias.data_ptr(),
                                      x.data_ptr(), h.data_ptr(), g.data_ptr(), b.data_ptr(), gstride,
                                      rows_per_group, add_one, eps, M, K, _stream()))
    return h


def op_resid_gemm_ln(x: torch.Tensor, bias: torch.Tensor, M: int, K: int, A: Optional[torch.Tensor] = None, W: Optional[torch.Tensor] = None,
                     A8: Optional[torch.Tensor] = None, SA: Optional[torch.Tensor] = None, W8: Optional[torch.Tensor] = None,
                     SW: Optional[torch.Tensor] = None, h: Optional[torch.Tensor] = None, h8: Optional[torch.Tensor] = None,
                     hs: Optional[torch.Tensor] = None, g: Optional[torch.Tensor] = None, b: Optional[torch.Tensor] = None, gstride: int = 0,
                     rows_per_group: int = 1 << 30, add_one: float = 0.0, eps: float = 1e-5, strideW: int = 0, w_rows: int = 0, nt_io: int = 1,
                     route: int = 0, scratch: Optional[torch.Tensor] = None, lda: Optional[int] = None, ldw: Optional[int] = None) -> None:
    """x [M,512] f32 += A.W^T + bias in place, then h (bf16) or h8 / hs (MXFP8) = LN(x)*(add_one+g)+b, all into the caller's buffers.
    Operands bf16 (A [M,K], W [groups?,512,K]) or MXFP8 (A8 / SA, W8 / SW); strideW / w_rows: one W per w_rows rows; g = None: no
    LayerNorm (route 0).  route 0 = resid_gemm_ln, the dispatcher of the latent stacks (needs `scratch` where it splits K); route 1 = the
    fused kernel gemm_resid_ln."""
    a, w = (A, W) if A is not None else (A8, W8)
    lda = a.stride(-2) if lda is None else lda
    ldw = w.stride(-2) if ldw is None else ldw
    check(lib().rald_op_resid_gemm_ln(_opt(A), _opt(A8), _opt(SA), lda, _opt(W), _opt(W8), _opt(SW), ldw, strideW, w_rows, bias.data_ptr(),
                                      x.data_ptr(), _opt(h), _opt(h8), _opt(hs), _opt(g), _opt(b), gstride, rows_per_group, add_one, eps, M, K,
                                      nt_io, route, _opt(scratch), 0 if scratch is None else scratch.numel() * scratch.element_size(), _stream()))


CONV_ENGINES = ("igemm", "line", "plane", "pplane", "igemm-split")     # what rald_op_conv3d_route returns, by index


def op_conv3d_route(B: int, ID: int, IH: int, IW: int, Cin: int, Cout: int, stride: int = 1, pad: int = 1, allow_split: int = 0):
    """(engine name, split count) of a Conv3d k3 shape: the library's one engine-choice function (host arithmetic, needs no GPU)."""
    splits = C.c_int32(0)
    e = lib().rald_op_conv3d_route(B, ID, IH, IW, Cin, Cout, stride, pad, int(allow_split), C.addressof(splits))
    if e < 0:
        check(1)
    return CONV_ENGINES[e], splits.value


def op_conv3d_wgrad_route(B: int, ID: int, IH: int, IW: int, Cin: int, Cout: int, stride: int = 1, pad: int = 1):
    """(kernel "line" | "generic", voxel ranges that do work, 64-voxel steps (line) or rows (generic) per range) of a Conv3d weight gradient:
    the plan op_conv3d_wgrad's launch itself uses (host arithmetic, needs no GPU)."""
    ranges, per = C.c_int32(0), C.c_int32(0)
    e = lib().rald_op_conv3d_wgrad_route(B, ID, IH, IW, Cin, Cout, stride, pad, C.addressof(ranges), C.addressof(per))
    if e < 0:
        check(1)
    return ("generic", "line")[e], ranges.value, per.value


def op_conv3d_full(x16: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, B: int, ID: int, IH: int, IW: int, Cin: int, Cout: int,
                   out: Optional[torch.Tensor] = None, out_bf16: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                   gn_part: Optional[torch.Tensor] = None, split_ws: Optional[torch.Tensor] = None, allow_split: int = 0, stride: int = 1,
                   pad: int = 1) -> None:
    """Conv3d k3 of x16 (bf16 [B,ID,IH,IW,Cin]) with packed weights wp [Cout,27,Cin] into the caller's buffers: out (f32, + resid; resid may
    be `out` itself) or out_bf16; gn_part (f64 [B*So/128,32,2]) takes the GroupNorm partials of the output from the epilogue.
    allow_split = 1: the route the encoder takes (split K through split_ws where op_conv3d_route says "igemm-split"); 0: one pass."""
    check(lib().rald_op_conv3d_full(x16.data_ptr(), wp.data_ptr(), bias.data_ptr(), _opt(resid), _opt(out), _opt(out_bf16), _opt(gn_part),
                                    _opt(split_ws), 0 if split_ws is None else split_ws.numel() * split_ws.element_size(), int(allow_split),
                                    B, ID, IH, IW, Cin, Cout, stride, pad, _stream()))


def op_gn_finish(part: torch.Tensor, stats: torch.Tensor, B: int, nblk: int) -> None:
    """stats f64 [B,32,2] = per sample the in-order sum of its nblk slots part [B*nblk,32,2] (partials of op_conv3d_full's gn_part)."""
    check(lib().rald_op_gn_finish(part.data_ptr(), stats.data_ptr(), B, nblk, _stream()))


def op_upsample2_cast(x: torch.Tensor, y16: torch.Tensor, B: int, D: int, H: int, W: int, Cc: int) -> None:
    """x f32 [B,D,H,W,C] -> y16 bf16 [B,2D,2H,2W,C], nearest neighbour (the radar decoder's Upsample before its convolution)."""
    check(lib().rald_op_upsample2_cast(x.data_ptr(), y16.data_ptr(), B, D, H, W, Cc, _stream()))


def op_pad_cast64(z: torch.Tensor, y16: torch.Tensor, rows: int, zc: int) -> None:
    """z f32 [rows,zc] -> y16 bf16 [rows,64], zero beyond zc."""
    check(lib().rald_op_pad_cast64(z.data_ptr(), y16.data_ptr(), rows, zc, _stream()))


def op_radar_tokens(z: torch.Tensor, Wp: torch.Tensor, bp: torch.Tensor, r_emb: torch.Tensor, a_emb: torch.Tensor, e_emb: torch.Tensor,
                    tokens: torch.Tensor, B: int, R: int, A: int, E: int, zc: int, Cc: int) -> None:
    """tokens f32 [B,R*A*E,C] = z [B,R,A,E,zc] . Wp [C,zc]^T + bp + r_emb[r] + a_emb[a] + e_emb[e] (the tokeniser without the encoder)."""
    check(lib().rald_op_radar_tokens(z.data_ptr(), Wp.data_ptr(), bp.data_ptr(), r_emb.data_ptr(), a_emb.data_ptr(), e_emb.data_ptr(),
                                     tokens.data_ptr(), B, R, A, E, zc, Cc, _stream()))


def op_gemm_geglu_mx8out(bias_packed: torch.Tensor, M: int, N: int, K: int, A: Optional[torch.Tensor] = None, W: Optional[torch.Tensor] = None,
                         A8: Optional[torch.Tensor] = None, SA: Optional[torch.Tensor] = None, W8: Optional[torch.Tensor] = None,
                         SW: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out8: Optional[torch.Tensor] = None,
                         outs: Optional[torch.Tensor] = None, ldc: Optional[int] = None) -> None:
    """The GEGLU projection (W rows and bias packed as for op_gemm_nt's epilogue 3) on bf16 or MXFP8 operands, into `out` (bf16 [M, N/2]) or
    into the MXFP8 form out8 [M, N/2] / outs [M, N/64] (the caller's buffers)."""
    a, w = (A, W) if A is not None else (A8, W8)
    ldc = (out if out is not None else out8).stride(-2) if ldc is None else ldc
    check(lib().rald_op_gemm_geglu_mx8out(_opt(A), _opt(A8), _opt(SA), a.stride(-2), _opt(W), _opt(W8), _opt(SW), w.stride(-2),
                                          bias_packed.data_ptr(), _opt(out), _opt(out8), _opt(outs), ldc, M, N, K, _stream()))


def op_layernorm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, gstride: int = 0, rows_per_group: int = 1,
                 add_one: float = 0.0, eps: float = 1e-5) -> torch.Tensor:
    M, D = x.shape
    out = torch.empty(M, D, device=x.device, dtype=torch.bfloat16)
    check(lib().rald_op_layernorm(x.data_ptr(), out.data_ptr(), M, D, g.data_ptr(), b.data_ptr(),
                                  gstride, rows_per_group, add_one, eps, _stream()))
    return out


def op_attention(Q: torch.Tensor, K: torch.Tensor, Vt: torch.Tensor, nk: int, heads: int, scale: float, prescaled: bool = False) -> torch.Tensor:
    """Q [B,nq,H*64], K [B,k_rows,H*64], Vt [B,H*64,ldvt] (bf16) -> O [B,nq,H*64] bf16.  prescaled: Q is already multiplied by
    scale*log2(e) and `scale` is ignored."""
    Bn, nq, HD = Q.shape
    O = torch.empty(Bn, nq, HD, device=Q.device, dtype=torch.bfloat16)
    check(lib().rald_op_attention(Q.data_ptr(), Q.stride(1), Q.stride(0), K.data_ptr(), K.stride(1), K.stride(0),
                                  Vt.data_ptr(), Vt.stride(1), Vt.stride(0), O.data_ptr(), O.stride(1), O.stride(0),
                                  nq, nk, K.shape[1], heads, Bn, scale, int(prescaled), _stream()))
    return O


def op_attention_split(Q: torch.Tensor, K: torch.Tensor, Vt: torch.Tensor, nk: int, heads: int, scale: float, ksplit: int) -> torch.Tensor:
    """op_attention with the keys split over `ksplit` workgroups per query block (+ combine pass)."""
    Bn, nq, HD = Q.shape
    O = torch.empty(Bn, nq, HD, device=Q.device, dtype=torch.bfloat16)
    scratch = _scratch(lib().rald_op_attention_split_scratch_bytes(max(ksplit, 32), nq, heads, Bn), Q.device)
    check(lib().rald_op_attention_split(Q.data_ptr(), Q.stride(1), Q.stride(0), K.data_ptr(), K.stride(1), K.stride(0),
                                        Vt.data_ptr(), Vt.stride(1), Vt.stride(0), O.data_ptr(), O.stride(1), O.stride(0),
                                        nq, nk, K.shape[1], heads, Bn, scale, ksplit, scratch.data_ptr(), _stream()))
    return O


def op_attention_vrow(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """Q [B,nq,H*64], K / V [B,nk,H*64] (bf16, possibly column slices of one fused buffer) -> O [B,nq,H*64] bf16."""
    Bn, nq, HD = Q.shape
    O = torch.empty(Bn, nq, HD, device=Q.device, dtype=torch.bfloat16)
    check(lib().rald_op_attention_vrow(Q.data_ptr(), Q.stride(1), Q.stride(0), K.data_ptr(), K.stride(1), K.stride(0),
                                       V.data_ptr(), V.stride(1), V.stride(0), O.data_ptr(), O.stride(1), O.stride(0),
                                       nq, K.shape[1], heads, Bn, scale, _stream()))
    return O


def op_attention_f16kv(Q: torch.Tensor, KV: torch.Tensor, nk: int, heads: int, ksplit: int = -1, shared_q: bool = False) -> torch.Tensor:
    """Folded-encoder attention: Q fp32 [B,nq,H*64] ([nq,H*64] with shared_q) already times scale*log2(e); KV fp16 [B,k_rows,64] = key AND
    value row of every head (rows nk.. must be zero) -> O bf16 [B,nq,H*64].  ksplit: -1 pick, 0/1 off, > 1 workgroups per query block."""
    Bn, k_rows = KV.shape[0], KV.shape[1]
    nq, HD = Q.shape[-2], Q.shape[-1]
    assert Q.dtype == torch.float32 and KV.dtype == torch.float16 and Q.is_contiguous() and KV.is_contiguous() and HD == heads * 64
    O = torch.empty(Bn, nq, HD, device=KV.device, dtype=torch.bfloat16)
    scratch = _scratch(lib().rald_op_attention_split_scratch_bytes(max(ksplit, 32), nq, heads, Bn), KV.device)
    check(lib().rald_op_attention_f16kv(Q.data_ptr(), HD, 0 if shared_q else nq * HD, KV.data_ptr(), O.data_ptr(), HD, nq * HD,
                                        nq, nk, k_rows, heads, Bn, ksplit, scratch.data_ptr(), _stream()))
    return O


def op_attention_args(O: torch.Tensor, K: torch.Tensor, nq: int, nk: int, heads: int, k_rows: int, Q: Optional[torch.Tensor] = None,
                      Qf: Optional[torch.Tensor] = None, Vt: Optional[torch.Tensor] = None, V: Optional[torch.Tensor] = None, scale: float = 1.0,
                      q_prescaled: bool = False, f16: bool = False, hsk: int = 64, v_padded: bool = False, ksplit: int = 0,
                      scratch: Optional[torch.Tensor] = None, strideQ: Optional[int] = None) -> None:
    """attention_d64 with every field of its argument block: O / K / Q or Qf / Vt or V are 3-D views [batch, rows, columns] (column and
    row slices of wider buffers are fine: leading dimensions and batch strides are the views' strides; strideQ = 0 shares the queries),
    written into the caller's O.  ksplit < 0 = pick; `scratch` is needed when the keys are split."""
    q = Q if Q is not None else Qf
    v = Vt if Vt is not None else V
    sv = (v.stride(1), v.stride(0))
    check(lib().rald_op_attention_args(_opt(Q), _opt(Qf), q.stride(1), q.stride(0) if strideQ is None else strideQ, K.data_ptr(), K.stride(1),
                                       K.stride(0), k_rows, _opt(Vt), *(sv if Vt is not None else (0, 0)), _opt(V), *(sv if V is not None else (0, 0)),
                                       O.data_ptr(), O.stride(1), O.stride(0), nq, nk, heads, O.shape[0], scale, int(q_prescaled), int(f16), hsk,
                                       int(v_padded), ksplit, _opt(scratch), 0 if scratch is None else scratch.numel() * scratch.element_size(),
                                       _stream()))


def op_attn_self_proj(qkv: torch.Tensor, Wo: torch.Tensor, part: torch.Tensor, n_latents: int, heads: int, batch: int, ld: Optional[int] = None,
                      part_f16: Optional[bool] = None) -> None:
    """part [heads, batch*n_latents, 512] (fp32, or fp16 holding 2^-6 x the value) = per head softmax(q k^T) v . Wo[:, 64h:64h+64]^T of the
    fused q|k|v rows qkv [batch*n_latents, ld] (q pre-multiplied by scale*log2 e)."""
    f16 = part.dtype == torch.float16 if part_f16 is None else part_f16
    check(lib().rald_op_attn_self_proj_slabs(qkv.data_ptr(), qkv.stride(0) if ld is None else ld, Wo.data_ptr(), part.data_ptr(), n_latents, heads,
                                             batch, int(f16), _stream()))


def op_xattn_q2_proj(hin: torch.Tensor, Wq: torch.Tensor, Kc: torch.Tensor, Vt: torch.Tensor, Wo: torch.Tensor, part: torch.Tensor, n_latents: int,
                     qscale: float, heads: int = 8, n_keys: int = 64, part_f16: Optional[bool] = None) -> None:
    """part [heads, M, 512] = per head softmax(qscale to_q(hin) Kc^T) Vc . Wo[:, 64h:64h+64]^T; Kc [batch, 64, >= 512] and Vt [batch, >= 512, 64]
    are views of the condition cache (this block's 512 columns / rows)."""
    f16 = part.dtype == torch.float16 if part_f16 is None else part_f16
    check(lib().rald_op_xattn_q2_proj_slabs(hin.data_ptr(), Wq.data_ptr(), Kc.data_ptr(), Kc.stride(1), Kc.stride(0), Vt.data_ptr(), Vt.stride(1),
                                            Vt.stride(0), Wo.data_ptr(), part.data_ptr(), hin.shape[0], n_latents, heads, n_keys, qscale, int(f16),
                                            _stream()))


def op_reduce_resid_ln(part: torch.Tensor, bias: torch.Tensor, x: torch.Tensor, h: Optional[torch.Tensor] = None, g: Optional[torch.Tensor] = None,
                       b: Optional[torch.Tensor] = None, gstride: int = 0, rows_per_group: int = 1 << 30, add_one: float = 0.0,
                       eps: float = 1e-5) -> None:
    """x [M,512] f32 += bias + sum_s part[s] in place (part [S, M, 512] fp32, or fp16 holding 2^-6 x the value); h = LN(x)*(add_one+g)+b."""
    check(lib().rald_op_reduce_resid_ln_slabs(part.data_ptr(), part.shape[0], part.stride(0), bias.data_ptr(), x.data_ptr(), _opt(h), x.shape[0],
                                              _opt(g), _opt(b), gstride, rows_per_group, add_one, eps, int(part.dtype == torch.float16), _stream()))


def f16_saturation_attn(reset: bool = True) -> int:
    """4-element groups of fp16 slab values that attn_self_proj / xattn_q2_proj clamped since the last reset (synchronises)."""
    n = lib().rald_debug_f16_saturation_attn(int(reset))
    if n < 0:
        check(1)
    return n


def op_ae_enc_features(pc: torch.Tensor, basis: torch.Tensor, var_factor: torch.Tensor):
    """pc [B,P,3] fp32, basis [3,24], var_factor [52,52] -> (F, G) fp16 [B, round_up(P,64), 64] (rald_amd/csrc/ae_encode.hip)."""
    Bn, P = pc.shape[0], pc.shape[1]
    Pp = (P + 63) // 64 * 64
    F = torch.empty(Bn, Pp, 64, device=pc.device, dtype=torch.float16)
    G = torch.empty_like(F)
    check(lib().rald_op_ae_enc_features(_f32c(pc).data_ptr(), _f32c(basis).data_ptr(), _f32c(var_factor).data_ptr(),
                                        F.data_ptr(), G.data_ptr(), Bn, P, Pp, _stream()))
    return F, G


def op_ae_enc_qproj(xin: Optional[torch.Tensor], X0: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, T1: torch.Tensor,
                    Q: torch.Tensor, rows: int) -> None:
    """The step between the folded encoder's two attentions (rald_amd/csrc/ae_encode.hip), into the caller's buffers: x [rows, dim] fp32 =
    (xin [rows, dim], or nothing when it is None) + X0 [M, dim][row % M]; Q [rows, 64] fp32 = LayerNorm(x; gamma, beta) . T1 [dim, 64].
    xin may be x itself (the product runs it in place).  dim 256 or 512."""
    for t, what in ((xin, "xin"), (X0, "X0"), (x, "x"), (gamma, "gamma"), (beta, "beta"), (T1, "T1"), (Q, "Q")):
        if t is not None:
            _need_cuda(t, what)
            assert t.dtype == torch.float32 and t.is_contiguous(), f"{what} must be contiguous fp32"
    assert X0.dim() == 2, "X0 must be [num_latents, dim]"
    M, dim = X0.shape
    assert rows >= 1 and x.numel() == rows * dim and Q.numel() == rows * 64, "x must hold rows * dim and Q rows * 64 floats"
    assert xin is None or xin.numel() == rows * dim, "xin must hold rows * dim floats"
    assert gamma.numel() == dim and beta.numel() == dim and T1.shape == (dim, 64), "gamma / beta [dim], T1 [dim, 64]"
    check(lib().rald_op_ae_enc_qproj(_opt(xin), X0.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), T1.data_ptr(), Q.data_ptr(),
                                     rows, M, dim, _stream()))


def _decode_tables(x, gamma, beta, t2aug, l_img, basis, queries=None):
    """the checks and conversions op_ae_decode, op_ae_decode_grad and op_ae_cast_rays share -> (x, gamma, beta, t2aug, basis) contiguous
    fp32 and (B, M, dim); `queries`, when given, is held to the device with the tables (before any shape is looked at)"""
    for t, what in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (t2aug, "t2aug"), (l_img, "l_img"), (basis, "basis"), (queries, "queries")):
        if t is not None:
            _need_cuda(t, what)
    assert l_img.dtype in (torch.float16, torch.int16) and l_img.numel() == 64 * 64 and l_img.is_contiguous()
    x, gamma, beta, t2aug, basis = (_f32c(t) for t in (x, gamma, beta, t2aug, basis))
    B, M, dim = x.shape
    assert t2aug.shape == (dim, 64) and gamma.numel() == dim and beta.numel() == dim and basis.shape == (3, 24)
    return x, gamma, beta, t2aug, basis, (B, M, dim)


def op_ae_decode(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, t2aug: torch.Tensor, l_img: torch.Tensor, basis: torch.Tensor,
                 c0: float, queries: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The streaming query decoder on caller-made tables (rald_amd/csrc/ae_decode.hip): x fp32 [B,M,dim] (output of the latent stack),
    gamma / beta [dim] (norm_context), t2aug fp32 [dim,64] and l_img [64*64] fp16 (or its bits as int16) as rald_op_ae_decode_tables writes
    them, basis [3,24], queries fp32 [B,Q,3] -> logits fp32 [B,Q], written to `out` (B*Q contiguous floats) when it is given."""
    x, gamma, beta, t2aug, basis, (B, M, dim) = _decode_tables(x, gamma, beta, t2aug, l_img, basis, queries)
    queries = _f32c(queries)
    Q = queries.shape[1]
    assert queries.shape[0] == B and queries.shape[2] == 3
    if out is None:
        out = torch.empty(B, Q, device=x.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.numel() == B * Q
    nbytes = _nbytes(lib().rald_op_ae_decode_scratch_bytes(B, M))
    scratch = _scratch(nbytes, x.device)
    check(lib().rald_op_ae_decode(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), t2aug.data_ptr(), l_img.data_ptr(), basis.data_ptr(), c0,
                                  queries.data_ptr(), out.data_ptr(), B, Q, M, dim, scratch.data_ptr(), nbytes, _stream()))
    return out.view(B, Q)


def op_ae_decode_grad(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, t2aug: torch.Tensor, l_img: torch.Tensor, basis: torch.Tensor,
                      c0: float, queries: torch.Tensor, out: torch.Tensor, grad: torch.Tensor, projected: Optional[torch.Tensor] = None,
                      max_step: float = 0.05, offsets: Optional[torch.Tensor] = None, max_per_sample: Optional[int] = None) -> None:
    """The gradient decoder on caller-made tables (rald_op_ae_decode_grad; arguments as op_ae_decode): queries [B,Q,3], or with
    `offsets` (int64 [B+1] on the device) [T,3] concatenated and max_per_sample the host bound of the longest segment.  Writes the
    caller's buffers: out (one float per query), grad and, when given, projected (three per query)."""
    x, gamma, beta, t2aug, basis, (B, M, dim) = _decode_tables(x, gamma, beta, t2aug, l_img, basis, queries)
    queries = _f32c(queries)
    assert queries.shape[-1] == 3
    if offsets is None:
        assert queries.dim() == 3 and queries.shape[0] == B
        n, total = queries.shape[1], B * queries.shape[1]
    else:
        assert _ragged_batch(offsets, "offsets") == B and queries.dim() == 2
        n, total = int(max_per_sample), queries.shape[0]
    for t, k in ((out, 1), (grad, 3), (projected, 3)):
        assert t is None or (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == k * total)
    nbytes = _nbytes(lib().rald_op_ae_decode_scratch_bytes(B, M))
    scratch = _scratch(nbytes, x.device)
    check(lib().rald_op_ae_decode_grad(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), t2aug.data_ptr(), l_img.data_ptr(), basis.data_ptr(), c0,
                                       queries.data_ptr(), _opt(offsets), out.data_ptr(), grad.data_ptr(), _opt(projected), float(max_step),
                                       B, n, M, dim, scratch.data_ptr(), nbytes, _stream()))


def _ray_tables(origins: torch.Tensor, dirs: torch.Tensor, B: int):
    """origins / dirs [R,3] (one table for every sample) or [B,R,3] -> (origins, dirs, ray_batch_stride in floats, R), contiguous fp32"""
    _need_cuda(origins, "origins")
    _need_cuda(dirs, "dirs")
    origins, dirs = _f32c(origins), _f32c(dirs)
    if origins.shape != dirs.shape or origins.dim() not in (2, 3) or origins.shape[-1] != 3 or origins.shape[-2] < 1:
        raise ValueError("origins and dirs must both be [R,3] or both [B,R,3], R >= 1")
    if origins.dim() == 3 and origins.shape[0] != B:
        raise ValueError(f"origins / dirs hold {origins.shape[0]} samples, the latents {B}")
    R = origins.shape[-2]
    return origins, dirs, (3 * R if origins.dim() == 3 else 0), R


def _ray_counts(n_steps, n_refine):
    """the march's and the bisection's step counts, checked on the host (ValueError) -> ints"""
    if int(n_steps) != n_steps or not 1 <= int(n_steps) <= 65535:
        raise ValueError("n_steps must be an integer in [1, 65535]")
    if int(n_refine) != n_refine or not 0 <= int(n_refine) <= 30:
        raise ValueError("n_refine must be an integer in [0, 30]")
    return int(n_steps), int(n_refine)


def op_ae_cast_rays(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, t2aug: torch.Tensor, l_img: torch.Tensor, basis: torch.Tensor,
                    c0: float, origins: torch.Tensor, dirs: torch.Tensor, ray_batch_stride: int, n_steps: int, n_refine: int,
                    out_t: torch.Tensor, out_logit: torch.Tensor, out_step: torch.Tensor, out_points: Optional[torch.Tensor] = None,
                    n_rays: Optional[int] = None) -> int:
    """First-return beam casting on caller-made tables (rald_op_ae_cast_rays; tables as op_ae_decode): origins / dirs contiguous fp32
    holding [R,3] (ray_batch_stride 0) or [B,R,3] (3 * R) in the caller's buffers, out_t / out_logit fp32 and out_step int32 of B * R
    elements, out_points None or fp32 of 3 * B * R; n_rays = R (default: out_step's elements / B).  What the entry checks is not checked
    here (any pointer may be None): -> its status (0 = done), the message in rald_last_error."""
    x, gamma, beta, t2aug, basis, (B, M, dim) = _decode_tables(x, gamma, beta, t2aug, l_img, basis)
    R = int(n_rays) if n_rays is not None else out_step.numel() // B
    for t, dt, k in ((origins, torch.float32, None), (dirs, torch.float32, None), (out_t, torch.float32, 1), (out_logit, torch.float32, 1),
                     (out_step, torch.int32, 1), (out_points, torch.float32, 3)):
        assert t is None or (t.dtype == dt and t.is_cuda and t.is_contiguous())
    nbytes = _nbytes(lib().rald_op_ae_decode_scratch_bytes(B, M))
    scratch = _scratch(nbytes, x.device)
    return lib().rald_op_ae_cast_rays(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), t2aug.data_ptr(), l_img.data_ptr(), basis.data_ptr(), c0,
                                      _opt(origins), _opt(dirs), int(ray_batch_stride), int(n_steps), int(n_refine), _opt(out_t),
                                      _opt(out_logit), _opt(out_step), _opt(out_points), B, R, M, dim, scratch.data_ptr(), nbytes, _stream())


class AeHandle(_Handle):
    """rald_ae*: encode / decode_latents / decode_queries of the set-latent autoencoder."""

    def __init__(self, cfg):
        self.cfg = cfg
        super().__init__("ae", C.byref(cfg))
        self._graphs = _GraphCache(lambda: lib().rald_ae_workspace_generation(self._h))
        self._dec_batch = 0

    def encode(self, pc: torch.Tensor, eps: torch.Tensor, want_moments: bool = False):
        _need_cuda(pc, "point cloud")
        pc, eps = _f32c(pc), _f32c(eps).to(pc.device)
        B = pc.shape[0]
        M, L = self.cfg.num_latents, self.cfg.latent_dim
        if pc.shape[1] != self.cfg.num_inputs:
            raise AssertionError(f"encode expects {self.cfg.num_inputs} points, got {pc.shape[1]}")   # models_ae.py:354
        z = torch.empty(B, M, L, device=pc.device, dtype=torch.float32)
        kl = torch.empty(B, device=pc.device, dtype=torch.float32)
        mean = torch.empty_like(z) if want_moments else None
        logvar = torch.empty_like(z) if want_moments else None
        check(lib().rald_ae_encode(self._h, pc.data_ptr(), B, eps.data_ptr(),
                                   _opt(mean), _opt(logvar),
                                   z.data_ptr(), kl.data_ptr(), _stream()))
        return (kl, z, mean, logvar) if want_moments else (kl, z)

    def _decode_latents_eager(self, z, ctx):
        check(lib().rald_ae_decode_latents(self._h, z.data_ptr(), z.shape[0], ctx.data_ptr(), _stream()))

    def decode_latents(self, z: torch.Tensor, use_graph: Optional[bool] = None) -> torch.Tensor:
        _need_cuda(z, "latents")
        z = _f32c(z)
        B = z.shape[0]
        nbytes = lib().rald_ae_ctx_bytes(self._h, B)
        if use_graph is None:
            use_graph = _graphs_enabled() and B <= GRAPH_MAX_BATCH
        if B > self._dec_batch:                        # the latent-stack workspace grows: captured graphs are stale
            self._graphs.clear()
            self._dec_batch = B
        if not use_graph:
            ctx = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
            self._decode_latents_eager(z, ctx)
            return ctx
        (ctx,) = self._graphs.run(("dec", B), [z], lambda: [torch.empty(nbytes, dtype=torch.uint8, device=z.device)],
                                  lambda ins, outs: self._decode_latents_eager(ins[0], outs[0]))
        return ctx

    def decode_queries(self, ctx: torch.Tensor, queries: torch.Tensor) -> torch.Tensor:
        _need_cuda(queries, "queries")
        queries = _f32c(queries)
        B, Q, _ = queries.shape
        self._check_ctx(ctx, B, "queries")
        out = torch.empty(B, Q, device=queries.device, dtype=torch.float32)
        check(lib().rald_ae_decode_queries(self._h, ctx.data_ptr(), queries.data_ptr(), B, Q, out.data_ptr(), _stream()))
        return out

    def decode_queries_ragged(self, ctx: torch.Tensor, queries: torch.Tensor, offsets: torch.Tensor, max_per_sample: int) -> torch.Tensor:
        """queries [T,3] = the samples' query sets concatenated, offsets int64 [B+1] on the device (sample b owns rows
        offsets[b] .. offsets[b+1]-1), max_per_sample a host upper bound of the longest set -> logits [T].  Nothing is read back."""
        _need_cuda(queries, "queries")
        queries = _f32c(queries).reshape(-1, 3)
        B = _ragged_batch(offsets, "offsets")
        self._check_ctx(ctx, B, "offsets")
        out = torch.empty(queries.shape[0], device=queries.device, dtype=torch.float32)
        check(lib().rald_ae_decode_queries_ragged(self._h, ctx.data_ptr(), queries.data_ptr(), offsets.data_ptr(), B, int(max_per_sample),
                                                  out.data_ptr(), _stream()))
        return out

    def _check_ctx(self, ctx: torch.Tensor, B: int, what: str) -> None:
        if ctx.dtype != torch.uint8 or not ctx.is_cuda or ctx.numel() != lib().rald_ae_ctx_bytes(self._h, B):
            raise RuntimeError(f"decoder context of {ctx.numel()} bytes does not belong to a batch of {B}: decode_latents(z) and the {what} "
                               "must have the same batch size")

    def decode_queries_grad(self, ctx: torch.Tensor, queries: torch.Tensor, project: bool = False, max_step: float = 0.05):
        """queries [B,Q,3] -> (logits [B,Q] - decode_queries' bit for bit -, d logit / d query [B,Q,3] in the normalised coordinates
        [, the queries after one clamped Newton step towards logit = 0, [B,Q,3]]): one launch, closed form."""
        _need_cuda(queries, "queries")
        queries = _f32c(queries)
        B, Q, _ = queries.shape
        self._check_ctx(ctx, B, "queries")
        out = torch.empty(B, Q, device=queries.device, dtype=torch.float32)
        grad = torch.empty(B, Q, 3, device=queries.device, dtype=torch.float32)
        proj = torch.empty_like(grad) if project else None
        check(lib().rald_ae_decode_queries_grad(self._h, ctx.data_ptr(), queries.data_ptr(), B, Q, out.data_ptr(), grad.data_ptr(), _opt(proj),
                                                float(max_step), _stream()))
        return (out, grad, proj) if project else (out, grad)

    def decode_queries_grad_ragged(self, ctx: torch.Tensor, queries: torch.Tensor, offsets: torch.Tensor, max_per_sample: int,
                                   project: bool = False, max_step: float = 0.05):
        """decode_queries_grad on the ragged layout of decode_queries_ragged: queries [T,3] -> (logits [T], grad [T,3][, projected [T,3]]).
        Nothing is read back."""
        _need_cuda(queries, "queries")
        queries = _f32c(queries).reshape(-1, 3)
        B = _ragged_batch(offsets, "offsets")
        self._check_ctx(ctx, B, "offsets")
        out = torch.empty(queries.shape[0], device=queries.device, dtype=torch.float32)
        grad = torch.empty(queries.shape[0], 3, device=queries.device, dtype=torch.float32)
        proj = torch.empty_like(grad) if project else None
        check(lib().rald_ae_decode_queries_grad_ragged(self._h, ctx.data_ptr(), queries.data_ptr(), offsets.data_ptr(), B, int(max_per_sample),
                                                       out.data_ptr(), grad.data_ptr(), _opt(proj), float(max_step), _stream()))
        return (out, grad, proj) if project else (out, grad)

    def cast_rays(self, ctx: torch.Tensor, batch: int, origins: torch.Tensor, dirs: torch.Tensor, n_steps: int = 256, n_refine: int = 8,
                  points: bool = True):
        """First returns of the segments o -> o + d through the decoder field of `ctx`, the context of `batch` samples
        (rald_ae_cast_rays): origins / dirs [R,3] (shared by the samples) or [B,R,3], normalised coordinates ->
        (t [B,R] in [0,1] or -1, logit [B,R] or NaN, step int32 [B,R] or -1[, points [B,R,3] or NaN]).  One launch, nothing read back."""
        n_steps, n_refine = _ray_counts(n_steps, n_refine)
        B = int(batch)
        origins, dirs, stride, R = _ray_tables(origins, dirs, B)
        self._check_ctx(ctx, B, "ray tables")
        dev = origins.device
        t = torch.empty(B, R, device=dev, dtype=torch.float32)
        logit = torch.empty(B, R, device=dev, dtype=torch.float32)
        step = torch.empty(B, R, device=dev, dtype=torch.int32)
        pts = torch.empty(B, R, 3, device=dev, dtype=torch.float32) if points else None
        check(lib().rald_ae_cast_rays(self._h, ctx.data_ptr(), origins.data_ptr(), dirs.data_ptr(), stride, B, R, n_steps, n_refine,
                                      t.data_ptr(), logit.data_ptr(), step.data_ptr(), _opt(pts), _stream()))
        return (t, logit, step, pts) if points else (t, logit, step)



# ---- MXFP8 (OCP microscaling: e4m3 elements + one e8m0 scale per 32 K-elements) -----------------------
def op_quantize_mx8(x: torch.Tensor):
    """x [..., K] f32 or bf16 (last dim contiguous) -> (q uint8 [..., K] e4m3 bytes, scales uint8 [..., K/32] e8m0)."""
    _need_cuda(x, "x")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("op_quantize_mx8: float32 or bfloat16 input expected")
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    rows = x2.shape[0]
    q = torch.empty(rows, K, device=x.device, dtype=torch.uint8)
    s = torch.empty(rows, K // 32, device=x.device, dtype=torch.uint8)
    check(lib().rald_op_quantize_mx8(x2.data_ptr(), int(x.dtype == torch.bfloat16), x2.stride(0), q.data_ptr(), K,
                                     s.data_ptr(), rows, K, _stream()))
    return q.reshape(*x.shape), s.reshape(*x.shape[:-1], K // 32)


def op_gemm_mx8(A8: torch.Tensor, sA: torch.Tensor, B8: torch.Tensor, sB: torch.Tensor, bias: Optional[torch.Tensor] = None,
                epilogue: int = 0, C_inout: Optional[torch.Tensor] = None, alpha: float = 1.0, alpha_ncols: int = 1 << 30) -> torch.Tensor:
    """A8 [batch?,M,K] / B8 [batch?,N,K] uint8 (e4m3) with scales [.., K/32] uint8 (e8m0) -> C = alpha*A.B^T + bias.
    epilogue 0 bf16, 1 f32, 2 f32 accumulate into C_inout (with 0 / 1 a given C_inout is the output buffer, of the epilogue's type);
    alpha applies to the columns n < alpha_ncols only."""
    batched = A8.dim() == 3 or B8.dim() == 3
    batch = (A8.shape[0] if A8.dim() == 3 else B8.shape[0]) if batched else 1
    M, K = A8.shape[-2], A8.shape[-1]
    N = B8.shape[-2]
    if B8.shape[-1] != K or sA.shape[-1] != K // 32 or sB.shape[-1] != K // 32 or not (sA.is_contiguous() and sB.is_contiguous()):
        raise ValueError("op_gemm_mx8: operand / scale shapes do not match")
    if epilogue == 2 or C_inout is not None:
        out = C_inout
    else:
        shape = (batch, M, N) if batched else (M, N)
        out = torch.empty(shape, device=A8.device, dtype=torch.bfloat16 if epilogue == 0 else torch.float32)
    check(lib().rald_op_gemm_mx8(A8.data_ptr(), sA.data_ptr(), A8.stride(-2), A8.stride(0) if A8.dim() == 3 else 0,
                                 sA.stride(0) if sA.dim() == 3 else 0, B8.data_ptr(), sB.data_ptr(), B8.stride(-2),
                                 B8.stride(0) if B8.dim() == 3 else 0, sB.stride(0) if sB.dim() == 3 else 0, out.data_ptr(),
                                 out.stride(-2), out.stride(0) if out.dim() == 3 else 0, _opt(bias),
                                 M, N, K, batch, alpha, epilogue, _stream(), alpha_ncols))
    return out


def op_layernorm_mx8(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, gstride: int = 0, rows_per_group: int = 1,
                     add_one: float = 0.0, eps: float = 1e-5):
    M, D = x.shape
    q = torch.empty(M, D, device=x.device, dtype=torch.uint8)
    s = torch.empty(M, D // 32, device=x.device, dtype=torch.uint8)
    check(lib().rald_op_layernorm_mx8(x.data_ptr(), q.data_ptr(), s.data_ptr(), M, D, g.data_ptr(),
                                      b.data_ptr(), gstride, rows_per_group, add_one, eps, _stream()))
    return q, s
