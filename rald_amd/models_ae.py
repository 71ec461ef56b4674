"""Drop-in for the reference's ``model/models_ae.py``: same factory names (``kl_d512_m512_l32_mix``
..., looked up via ``models_ae.__dict__[name](N=...)``, main_generation.py:110), same
``KLAutoEncoder.encode / decode / forward`` signatures and return values (:351-432) and the same
``state_dict`` keys.  Arithmetic runs in librald_hip.so (include/rald_hip.h); no PyTorch compute
path exists.  Under ``train()`` + grad mode ``forward`` is differentiable (``_AeForwardFn`` over rald_amd.train_ae), so the
reference's stage-1 loop (engine_ae.py:33-104) trains the module as written.

Scope: query_type='mix' (the shipped config, configs/ae/*cone.yml:85) and 'learnable' (:325-326,
:378-379); query_type='point' needs torch_cluster.fps (a CUDA extension that is neither vendored
nor installed; SURVEY.md §8c 'parity unpinned') and raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import weights as _w
from ._handles import AeHandle
from ._lib import AeConfig
from .models_radar_generation import _HipBacked, build_param_tree


class DiagonalGaussianDistribution(object):
    """models_ae.py:141-179 (moments only; sampling happens inside rald_ae_encode)."""

    def __init__(self, mean, logvar, deterministic=False):
        self.mean = mean
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def mode(self):
        return self.mean


class KLAutoEncoder(_HipBacked):
    def __init__(self, *, depth=24, dim=512, queries_dim=512, output_dim=1, num_inputs=2048, num_latents=512,
                 latent_dim=64, heads=8, dim_head=64, weight_tie_layers=False, decoder_ff=False, query_type='point'):
        super().__init__()
        if query_type not in ('mix', 'learnable'):
            raise NotImplementedError(f"query_type={query_type!r}: 'mix' (the shipped config) and 'learnable' are built; "
                                      "'point' needs torch_cluster.fps")
        if weight_tie_layers or decoder_ff or output_dim != 1 or queries_dim != dim:
            raise NotImplementedError("only the create_autoencoder() configuration is built (models_ae.py:447-458)")
        self.depth, self.num_inputs, self.num_latents = depth, num_inputs, num_latents
        self.dim, self.latent_dim, self.heads, self.dim_head = dim, latent_dim, heads, dim_head
        self.query_type = query_type
        spec = _w.ae_spec(dim=dim, num_latents=num_latents, latent_dim=latent_dim, depth=depth, heads=heads,
                          dim_head=dim_head, query_type=query_type)
        build_param_tree(self, spec, buffers=("point_embed.basis",))
        self._hip = None
        self._hip_fp = None
        self._ctx_memo = None

    def _handle(self) -> AeHandle:
        fp = self._state_fingerprint()
        if self._hip is None or self._hip_fp != fp:
            cfg = AeConfig(dim=self.dim, num_latents=self.num_latents, latent_dim=self.latent_dim, depth=self.depth,
                           heads=self.heads, dim_head=self.dim_head, num_inputs=self.num_inputs,
                           query_type={'mix': 0, 'learnable': 1}[self.query_type])
            h = AeHandle(cfg)
            h.load(self.state_dict().items())
            self._hip, self._hip_fp, self._ctx_memo = h, fp, None
        return self._hip

    def encode(self, pc):
        """pc [B,N,3] -> (kl [B], z [B,M,latent_dim]); posterior noise from torch.randn on the CPU
        global RNG, exactly where the reference draws it (:153)."""
        B, N, D = pc.shape
        assert N == self.num_inputs
        eps = torch.randn(B, self.num_latents, self.latent_dim)
        kl, z = self._handle().encode(pc, eps)
        return kl, z

    def _context(self, x):
        """Latent stack + decoder context for latents x; memoised on the tensor OBJECT (+ its version; the entry keeps
        the tensor alive, see _HipBacked._memo_hit), so the reference's pattern of several decode() calls on the same
        `sampled_tokens` (engine_generation.py:204, :275, :300) runs the 24-layer stack once."""
        if not self._memo_hit(self._ctx_memo, x):
            self._ctx_memo = (x, x._version, self._handle().decode_latents(x))
        return self._ctx_memo[2]

    def decode(self, x, queries):
        """x [B,M,latent_dim], queries [B,Q,3] -> logits [B,Q,1] (:408-424)."""
        h = self._handle()
        return h.decode_queries(self._context(x), queries).unsqueeze(-1)

    def decode_volume(self, x, lo, spacing, dims, max_queries=1 << 22):
        """The decoder field on a regular grid: x [B,M,latent_dim]; node (i, j, k) at lo + (i, j, k) * spacing, dims = (nx, ny, nz)
        (query_points.field_grid / grid_queries) -> logits [B,nx,ny,nz], the volume postprocess.extract_surface_batch meshes.  Decoded in
        slabs of whole x-planes of at most max_queries nodes per sample, through decode's path and its memoised context.  The decoder cuts
        a query set into chunks of 64 from its first row, so a slab holds a multiple of 64 / gcd(64, ny * nz) planes (at least that many,
        also where they exceed max_queries): every slab starts on a chunk boundary of the whole grid and every logit is decode's on
        grid_queries(lo, spacing, dims), bit for bit."""
        import math
        from . import query_points as QP
        from .postprocess import _grid_spec
        lo3, h3, dims3 = _grid_spec(lo, spacing, dims)
        if isinstance(max_queries, bool) or not isinstance(max_queries, int) or max_queries < 1:
            raise ValueError("max_queries must be an integer >= 1")
        if not (isinstance(x, torch.Tensor) and x.dim() == 3):
            raise ValueError("x must be the latents [B, M, latent_dim]")
        plane = dims3[1] * dims3[2]
        step = 64 // math.gcd(64, plane)
        per_slab = max(step, max_queries // plane // step * step)
        h, ctx = self._handle(), self._context(x)
        B = x.shape[0]
        out = torch.empty(B, dims3[0] * plane, device=x.device, dtype=torch.float32)
        for i0 in range(0, dims3[0], per_slab):
            ni = min(per_slab, dims3[0] - i0)
            q = QP.grid_queries(lo3, h3, dims3, i0, ni, device=out.device)
            out[:, i0 * plane:(i0 + ni) * plane] = h.decode_queries(ctx, q.unsqueeze(0).expand(B, -1, -1))
        return out.view(B, *dims3)

    def decode_ragged(self, x, queries, offsets, max_per_sample):
        """decode for query sets of different sizes: x [B,M,latent_dim], queries [T,3] = the B sets concatenated, offsets int64 [B+1]
        on the device, max_per_sample = a host upper bound of the longest set (too small a bound leaves the rows behind it undecoded,
        with no error) -> logits [T].  Same memoised context as decode; set b's logits are row b of decode on the same batch x with
        its queries (not bitwise those of decode(x[b:b+1], ...): the latent stack picks its engines by batch rows)."""
        h = self._handle()
        return h.decode_queries_ragged(self._context(x), queries, offsets, max_per_sample)

    def decode_with_gradient(self, x, queries, project=False, max_step=0.05):
        """decode + the gradient of each logit with respect to its query point, forward mode in one launch (no autograd, no graph):
        x [B,M,latent_dim], queries [B,Q,3] -> (logits [B,Q,1] - decode's bit for bit -, grad [B,Q,3] in the normalised coordinates
        [, projected [B,Q,3]: the queries after one Newton step towards the surface, at most max_step long, inside [-1,1]^3])."""
        with torch.no_grad():
            out = self._handle().decode_queries_grad(self._context(x), queries, project, max_step)
        return (out[0].unsqueeze(-1),) + tuple(out[1:])

    def decode_ragged_with_gradient(self, x, queries, offsets, max_per_sample, project=False, max_step=0.05):
        """decode_with_gradient on decode_ragged's layout -> (logits [T], grad [T,3][, projected [T,3]])."""
        with torch.no_grad():
            return self._handle().decode_queries_grad_ragged(self._context(x), queries, offsets, max_per_sample, project, max_step)

    def cast_rays(self, x, origins, dirs, n_steps=256, n_refine=8, points=True):
        """First-return scan of the decoder field, one launch: x [B,M,latent_dim]; origins / dirs [R,3] (one beam table
        for every sample) or [B,R,3], in the decoder's normalised coordinates, beam r the segment from o to o + d.  The beam is sampled at
        t_k = k / n_steps, k = 0 .. n_steps; it returns at the first sample whose logit is > 0, refined by n_refine bisection steps between
        that sample and the one before.  -> (t [B,R] in [0,1], -1 without a return; logit [B,R] at the returned point - decode's bit for
        bit there -, NaN without; step int32 [B,R], the first positive sample, -1 without[; points [B,R,3] = o + t d, NaN without]).
        Same memoised context as decode; no autograd."""
        with torch.no_grad():
            return self._handle().cast_rays(self._context(x), x.shape[0], origins, dirs, n_steps, n_refine, points)

    def forward(self, pc, queries):
        # Route like EDMPrecond.forward: model.train() + grad mode + trainable parameters = the stage-1 training step
        # (engine_ae.py:51, :73-104); eval() / no_grad = the inference path below, unchanged.
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._train_forward(pc, queries)
        kl, x = self.encode(pc)
        o = self.decode(x, queries).squeeze(-1)
        return {'logits': o, 'kl': kl}

    def _train_forward(self, pc, queries, masks=None, eps=None):
        """The differentiable forward (_AeForwardFn).  ``masks`` (1 + 2*depth drop-path scales [B] for 'mix', 2*depth for 'learnable')
        and ``eps`` [B, M, latent_dim] default to the reference's draws: timm's DropPath on the device RNG in forward order, then
        torch.randn on the CPU global RNG (:153)."""
        if pc.requires_grad or queries.requires_grad:
            raise NotImplementedError("gradients with respect to the points / the query points are not built into autograd (the reference "
                                      "trains the parameters only); the logit's forward-mode gradient with respect to the query points is "
                                      "KLAutoEncoder.decode_with_gradient")
        if self.dim != 512 or self.heads * self.dim_head != 512 or self.dim_head != 64 or self.num_latents != 512 \
                or self.latent_dim < 32 or self.latent_dim % 32:
            raise NotImplementedError("the differentiable autoencoder covers dim 512, 8 x 64 heads, 512 latents and latent_dim a multiple "
                                      "of 32 (kl_d512_m512_l32_mix and its 'learnable' twin); use eval() / no_grad for the others")
        if pc.dim() != 3 or queries.dim() != 3 or pc.shape[0] != queries.shape[0] or pc.shape[-1] != 3 or queries.shape[-1] != 3:
            raise RuntimeError(f"pc must be [B,N,3] and queries [B,Q,3]; got {tuple(pc.shape)} and {tuple(queries.shape)}")
        tr = self._autograd_trainers()
        B = pc.shape[0]
        dev = self._device()
        if masks is None:
            from .train_ae import drop_path_masks
            masks = drop_path_masks(B, tr["ae"].n_masks, dev)
        if eps is None:
            eps = torch.randn(B, self.num_latents, self.latent_dim)
        self._last_drop_path_masks = masks
        params = [p for _, p in self.named_parameters()]
        logits, kl = _AeForwardFn.apply(self, pc.to(device=dev, dtype=torch.float32), queries.to(device=dev, dtype=torch.float32), eps,
                                        masks, *params)
        return {'logits': logits, 'kl': kl}

    def _autograd_trainers(self):
        """As EDMPrecond._autograd_trainers: shadow Parameters sharing the real parameters' storage (the trainer accumulates into
        their `.grad`; the real `.grad`s belong to autograd), rebuilt when a parameter's storage moved, bf16 copies refreshed when a
        parameter's version changed (an optimizer step)."""
        from .train_ae import AeTrainer
        named = list(self.named_parameters())
        ptrs = tuple(p.data_ptr() for _, p in named)
        vers = tuple(p._version for _, p in named)
        tr = self.__dict__.get("_ag_trainers")
        if tr is None or tr["ptrs"] != ptrs:
            shadow = {n: nn.Parameter(p.detach(), requires_grad=True) for n, p in named}
            tr = dict(shadow=shadow, names=[n for n, _ in named], ptrs=ptrs, vers=vers,
                      ae=AeTrainer(shadow, self.point_embed.basis, self.depth, self.latent_dim, self.query_type, heads=self.heads))
            self.__dict__["_ag_trainers"] = tr
        elif tr["vers"] != vers:
            tr["ae"].refresh_weights()
            tr["vers"] = vers
        return tr


class _AeForwardFn(torch.autograd.Function):
    """KLAutoEncoder.forward as an autograd node: forward = rald_amd.train_ae.AeTrainer.forward (HIP kernels, activations kept),
    backward = its hand-written backward.  The parameters are inputs of the node, so ``loss.backward()`` fills ``p.grad`` the
    ordinary way (GradScaler, clip_grad_norm_, torch.optim and DDP hooks see ordinary gradients)."""

    @staticmethod
    def forward(ctx, module, pc, queries, eps, masks, *params):
        tr = module._autograd_trainers()
        logits, kl, st = tr["ae"].forward(pc, queries, eps, masks)
        ctx.module, ctx.st = module, st
        return logits, kl

    @staticmethod
    def backward(ctx, dlogits, dkl):
        if ctx.st is None:
            raise RuntimeError("KLAutoEncoder.forward: backward through the same forward a second time - the saved activations are "
                               "released by the first backward; retain_graph is not supported")
        tr = ctx.module._autograd_trainers()
        for sh in tr["shadow"].values():
            sh.grad = None
        tr["ae"].backward(ctx.st, dlogits.contiguous() if dlogits is not None else None, dkl.contiguous() if dkl is not None else None)
        ctx.st = None
        grads = tuple(tr["shadow"][n].grad if tr["shadow"][n].grad is not None else torch.zeros_like(tr["shadow"][n])
                      for n in tr["names"])
        return (None, None, None, None, None) + grads


class AutoEncoder(nn.Module):
    """models_ae.py:181 ('not actually used' in the reference) - needs torch_cluster.fps."""

    def __init__(self, **kw):
        super().__init__()
        raise NotImplementedError("the deterministic AutoEncoder needs torch_cluster.fps and is unused by the reference")


def create_autoencoder(dim=512, M=512, latent_dim=64, N=2048, determinisitc=False, query_type='point'):
    if determinisitc:
        return AutoEncoder()
    return KLAutoEncoder(depth=24, dim=dim, queries_dim=dim, output_dim=1, num_inputs=N, num_latents=M,
                         latent_dim=latent_dim, heads=8, dim_head=64, query_type=query_type)


# ---- factories (:461-512); the 'mix' and 'learnable' ones construct, the others need torch_cluster.fps (module docstring)
def kl_d512_m512_l512(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=512, N=N, determinisitc=False)


def kl_d512_m512_l64(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=64, N=N, determinisitc=False)


def kl_d512_m512_l32(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=32, N=N, determinisitc=False)


def kl_d512_m512_l32_learn(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=32, N=N, determinisitc=False, query_type='learnable')


def kl_d512_m512_l32_mix(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=32, N=N, determinisitc=False, query_type='mix')


def kl_d512_m512_l16(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=16, N=N, determinisitc=False)


def kl_d512_m512_l8(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=8, N=N, determinisitc=False)


def kl_d512_m512_l4(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=4, N=N, determinisitc=False)


def kl_d512_m512_l2(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=2, N=N, determinisitc=False)


def kl_d512_m512_l1(N=2048):
    return create_autoencoder(dim=512, M=512, latent_dim=1, N=N, determinisitc=False)


def ae_d512_m512(N=2048):
    return create_autoencoder(dim=512, M=512, N=N, determinisitc=True)


def ae_d512_m256(N=2048):
    return create_autoencoder(dim=512, M=256, N=N, determinisitc=True)


def ae_d512_m128(N=2048):
    return create_autoencoder(dim=512, M=128, N=N, determinisitc=True)


def ae_d512_m64(N=2048):
    return create_autoencoder(dim=512, M=64, N=N, determinisitc=True)


def ae_d256_m512(N=2048):
    return create_autoencoder(dim=256, M=512, N=N, determinisitc=True)


def ae_d128_m512(N=2048):
    return create_autoencoder(dim=128, M=512, N=N, determinisitc=True)


def ae_d64_m512(N=2048):
    return create_autoencoder(dim=64, M=512, N=N, determinisitc=True)
