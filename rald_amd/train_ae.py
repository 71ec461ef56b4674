"""Training step of the set-latent autoencoder on the HIP kernels: forward with the activations kept, and the hand-written
backward of ``KLAutoEncoder.forward`` (model/models_ae.py:351-432) for stage 1 of the reference's training
(engine_ae.py:33-104: BCE on the occupancy logits + 1e-3 * KL, backward, clip, AdamW, EMA).

``AeTrainer`` plays the role ``train_dit.DitTrainer`` plays for the denoiser: it owns the bf16 compute copies of the fp32
parameters it is given, ``forward`` returns (logits [B, Q], kl [B], state) and ``backward(state, dlogits, dkl)`` accumulates into
the parameters' ``.grad``.  ``models_ae._AeForwardFn`` wraps the two as an autograd node.

Composition (every product a bf16 MFMA GEMM with fp32 accumulation; weight gradients through the atomic-free ``gemm_tn`` workspace
form, so a backward pass is bit-reproducible):
  encoder   PointEmbed -> ['mix': LN -> 8 x 64 attention over the N raw embeddings (key tail masked in csrc/attn_bwd.hip) -> to_out,
            drop-path, + s_latents -> query_proj | 'learnable': latents] -> 1-head dim-512 cross-attention with norm_context + residual
            -> GEGLU FF + residual -> [mean | logvar] -> posterior (z, kl)
  decoder   proj -> depth x (LN -> 8 x 64 self-attention, drop-path residual; LN -> GEGLU FF, drop-path residual) -> PointEmbed of the
            queries -> 1-head dim-512 cross-attention onto the latents (norm_context) -> to_outputs
The two 1-head dim-512 attentions run unfused: S = q.k^T / sqrt(512) as one batched GEMM with K = 512 (fp32, keys padded to a multiple of
64), the row softmax, P.V; backward dP = dO.V^T, csrc/ae_train.hip's softmax backward, dQ = dS.K and the key side through gemm_tn.
The kernels specific to the AE (affine LayerNorm backward, PointEmbed weight gradient, posterior backward, drop-path rows, the masked
softmax backward) are in csrc/ae_train.hip.

``AeStepTrainer`` / ``GraphedAeStep`` are the stage-1 counterparts of ``train_dit.EdmTrainer`` / ``GraphedTrainStep``: the whole iteration
(forward, ``train_ops.ae_loss``, backward, clip, fused AdamW / EMA) on ``train_utils.FlatAdamW`` storage with no host sync, eagerly or
with the forward + loss + backward captured in one hipGraph.  ``engine_ae.train_one_epoch`` drives either.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import train_ops as TO
from ._handles import _opt, _scratch, _stream, op_attention, op_attention_vrow, op_gemm_nt, op_gemm_tn, op_layernorm
from ._lib import check, lib
from .train_ops import HEAD, param_grad, sgemm_acc

DROP_PATH_RATE = 0.1
LN_EPS = 1e-5


def drop_path_masks(batch: int, n_masks: int, device) -> List[torch.Tensor]:
    """The per-sample drop-path scales of one forward, drawn as timm's DropPath draws them (rate 0.1, scale_by_keep):
    ``x.new_empty((B, 1, 1)).bernoulli_(0.9).div_(0.9)`` on the activations' device, in the reference's forward order (mix_attn_layer,
    then layers.0 attention, layers.0 FF, ...).  Returns ``n_masks`` fp32 tensors [B]."""
    keep = 1.0 - DROP_PATH_RATE
    out = []
    for _ in range(n_masks):
        out.append(torch.empty((batch, 1, 1), device=device, dtype=torch.float32).bernoulli_(keep).div_(keep).reshape(batch))
    return out


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _f32(*shape, device):
    return torch.empty(*shape, device=device, dtype=torch.float32)


def _zeros(*shape, device):
    return torch.zeros(*shape, device=device, dtype=torch.float32)


def ln_affine_bwd(x: torch.Tensor, dh: torch.Tensor, gamma: torch.Tensor, dx: torch.Tensor, dgamma: torch.Tensor, dbeta: torch.Tensor,
                  dx_bf16: Optional[torch.Tensor] = None) -> None:
    """nn.LayerNorm(512) backward (csrc/ae_train.hip): dx [rows, 512] fp32 += dLN(dh); dgamma / dbeta [512] += their column sums in a
    fixed order; dx_bf16 (optional) receives the updated dx as bf16."""
    rows = x.shape[0]
    nbytes = lib().rald_op_ln_affine_bwd_scratch_bytes(rows)
    scratch = _scratch(nbytes, x.device)
    check(lib().rald_op_ln_affine_bwd(x.data_ptr(), dh.data_ptr(), gamma.data_ptr(), LN_EPS, rows, dx.data_ptr(), _opt(dx_bf16), dgamma.data_ptr(),
                                      dbeta.data_ptr(), scratch.data_ptr(), nbytes, _stream()))


def pe_wgrad(dY: torch.Tensor, pts: torch.Tensor, basis: torch.Tensor, dW: torch.Tensor, db: torch.Tensor) -> None:
    """PointEmbed.mlp gradient: dW [512, 51] += dY^T . features(pts), db += column sums of dY (fixed order; features recomputed)."""
    rows = dY.shape[0]
    nbytes = lib().rald_op_pe_wgrad_scratch_bytes(rows)
    scratch = _scratch(nbytes, dY.device)
    check(lib().rald_op_pe_wgrad(dY.data_ptr(), pts.data_ptr(), basis.data_ptr(), rows, dW.data_ptr(), db.data_ptr(), scratch.data_ptr(), nbytes,
                                 _stream()))


def scale_rows_add(y: torch.Tensor, s: torch.Tensor, x: torch.Tensor, rows_per_sample: int) -> None:
    """x += s[row // rows_per_sample] * y (the drop-path residual)."""
    check(lib().rald_op_scale_rows(y.data_ptr(), s.data_ptr(), x.data_ptr(), None, y.shape[0], y.shape[1], rows_per_sample, _stream()))


def scale_rows_bf16(dx: torch.Tensor, s: torch.Tensor, rows_per_sample: int) -> torch.Tensor:
    out = torch.empty(dx.shape, device=dx.device, dtype=torch.bfloat16)
    check(lib().rald_op_scale_rows(dx.data_ptr(), s.data_ptr(), None, out.data_ptr(), dx.shape[0], dx.shape[1], rows_per_sample, _stream()))
    return out


def wgrad_narrow(dy: torch.Tensor, x: torch.Tensor, n: int):
    """(dy[:, :n]^T . x, column sums of dy[:, :n]) for a narrow fp32 dy [R, n] (n <= 64: mean_fc | logvar_fc, to_outputs).  gemm_tn keeps
    fp32 atomics for outputs of at most 64 rows, so dy is zero-padded to 128 columns and the workspace form runs: reproducible."""
    C_ = torch.zeros(128, x.shape[1], device=dy.device, dtype=torch.float32)
    cs = torch.zeros(128, device=dy.device, dtype=torch.float32)
    TO.lin_wgrad(TO.pad_channels(dy, 128), x, C_, cs, atomics=False)
    return C_[:n], cs[:n]


class AeTrainer:
    """Forward + backward of ``KLAutoEncoder`` (query_type 'mix' or 'learnable', dim 512, 8 x 64 heads); gradients go to ``param.grad``
    of the parameters given (names as in ``KLAutoEncoder.state_dict()``)."""

    def __init__(self, named_params: Dict[str, torch.nn.Parameter], basis: torch.Tensor, depth: int, latent_dim: int, query_type: str,
                 heads: int = 8):
        if query_type not in ("mix", "learnable"):
            raise NotImplementedError(f"AeTrainer: query_type={query_type!r} (only 'mix' and 'learnable' are built)")
        if heads * HEAD != 512 or latent_dim < 32 or latent_dim % 32:
            raise NotImplementedError("AeTrainer: dim 512 with 8 x 64 heads and latent_dim a multiple of 32 (>= 32) are built")
        self.P, self.depth, self.L, self.H, self.mix = named_params, depth, latent_dim, heads, query_type == "mix"
        dev = next(iter(named_params.values())).device
        if dev.type != "cuda":
            raise RuntimeError("AeTrainer runs on the HIP device only (no CPU fallback)")
        self.dev = dev
        self.basis = basis.to(device=dev, dtype=torch.float32).contiguous()
        self.W: Dict[str, torch.Tensor] = {}
        self.refresh_weights()

    @property
    def n_masks(self) -> int:
        return (1 if self.mix else 0) + 2 * self.depth

    # -- bf16 compute copies (and transposes for the input-gradient products) of the fp32 parameters -----------------------------
    def refresh_weights(self) -> None:
        P, W = self.P, {}
        d = lambda n: P[n].data

        def mat(key, t):
            W[key] = TO.cast_bf16(t.contiguous())
            W[key + "T"] = TO.T2(t.contiguous())

        def attn(p, fused_qkv):
            if fused_qkv:
                mat(p + "qkv", torch.cat([d(p + "fn.to_q.weight"), d(p + "fn.to_kv.weight")], 0))
            else:
                mat(p + "q", d(p + "fn.to_q.weight"))
                mat(p + "kv", d(p + "fn.to_kv.weight"))
            mat(p + "o", d(p + "fn.to_out.weight"))

        def ff(p):
            mat(p + "w1", d(p + "fn.net.0.weight"))
            mat(p + "w2", d(p + "fn.net.2.weight"))

        for i in range(self.depth):
            attn(f"layers.{i}.0.", True)
            ff(f"layers.{i}.1.")
        if self.mix:
            attn("mix_attn_layer.", False)
            mat("query_proj", d("query_proj.weight"))
        attn("cross_attend_blocks.0.", False)
        ff("cross_attend_blocks.1.")
        attn("decoder_cross_attn.", False)
        W["pe"] = TO.pad_channels(d("point_embed.mlp.weight"), 64)                            # [512, 64], features 51.. zero
        mv = torch.cat([d("mean_fc.weight"), d("logvar_fc.weight")], 0)                      # [2L, 512]
        mat("mv", mv)
        W["b_mv"] = torch.cat([d("mean_fc.bias"), d("logvar_fc.bias")], 0).contiguous()
        Lp = _round_up(self.L, 64)
        W["proj"] = TO.pad_channels(d("proj.weight"), Lp)                                    # [512, Lp]
        W["projT"] = TO.T2(d("proj.weight").contiguous())                                   # [L, 512]
        to = torch.zeros(4, 512, device=self.dev, dtype=torch.float32)
        to[0] = d("to_outputs.weight")[0]
        W["to"] = TO.cast_bf16(to)                                                           # [4, 512], rows 1..3 zero
        self.W = W

    # -- building blocks --------------------------------------------------------------------------------------------------------
    def _point_embed(self, pts: torch.Tensor) -> torch.Tensor:
        """pts [R, 3] fp32 -> PointEmbed [R, 512] fp32 (features in bf16, one K = 64 GEMM)."""
        R = pts.shape[0]
        feat = torch.empty(R, 64, device=self.dev, dtype=torch.bfloat16)
        check(lib().rald_op_point_features(pts.data_ptr(), self.basis.data_ptr(), feat.data_ptr(), R, _stream()))
        return op_gemm_nt(feat, self.W["pe"], bias=self.P["point_embed.mlp.bias"].data, epilogue=1)

    def _ln(self, x: torch.Tensor, p: str) -> torch.Tensor:
        return op_layernorm(x, self.P[p + ".weight"].data, self.P[p + ".bias"].data, gstride=0, rows_per_group=1 << 30, add_one=0.0, eps=LN_EPS)

    def _ln_bwd(self, x, dh, p, dx, dx_bf16=None):
        ln_affine_bwd(x, dh, self.P[p + ".weight"].data, dx, param_grad(self.P[p + ".weight"]), param_grad(self.P[p + ".bias"]), dx_bf16)

    def _lin_bwd(self, dy, x_in, wname, bname=None):
        TO.lin_wgrad(dy, x_in, param_grad(self.P[wname]), param_grad(self.P[bname]) if bname is not None else None, atomics=False)

    def _attn512_fwd(self, q: torch.Tensor, kv: torch.Tensor, Bn: int, nq: int, kp: int, nk: int):
        """1-head dim-512 attention: q [Bn*nq, 512] bf16, kv [Bn*kp, 1024] bf16 (k | v, rows nk.. of each sample padding) ->
        (O [Bn*nq, 512] bf16, S [Bn, nq, kp] fp32 scores times 512^-0.5, the only thing the backward keeps)."""
        D = 512
        kv3 = kv.view(Bn, kp, 2 * D)
        S = op_gemm_nt(q.view(Bn, nq, D), kv3[:, :, :D], epilogue=1, alpha=D ** -0.5)
        P = TO.softmax_rows(S, nk)
        vT = TO.transpose(kv[:, D:], kp, D, 2 * D, Bn, kp * 2 * D).view(Bn, D, kp)
        O = op_gemm_nt(P, vT, epilogue=0)
        return O.view(Bn * nq, D), S

    def _attn512_bwd(self, q, kv, O, S, dO, Bn: int, nq: int, kp: int, nk: int):
        """-> (dq [Bn*nq, 512] bf16, dkv [Bn*kp, 1024] bf16; padded key rows zero)."""
        D = 512
        kv3 = kv.view(Bn, kp, 2 * D)
        dP = op_gemm_nt(dO.view(Bn, nq, D), kv3[:, :, D:], epilogue=1)
        delta = TO.rowdot(dO, O)
        P = torch.empty(Bn, nq, kp, device=self.dev, dtype=torch.bfloat16)
        dS = torch.empty(Bn, nq, kp, device=self.dev, dtype=torch.bfloat16)
        check(lib().rald_op_softmax_bwd_rows(S.data_ptr(), dP.data_ptr(), delta.data_ptr(), Bn * nq, kp, nk, D ** -0.5, P.data_ptr(), dS.data_ptr(),
                                             _stream()))
        del dP
        kT = TO.transpose(kv[:, :D], kp, D, 2 * D, Bn, kp * 2 * D).view(Bn, D, kp)
        dq = op_gemm_nt(dS, kT, epilogue=0).view(Bn * nq, D)
        dkv32 = _zeros(Bn * kp, 2 * D, device=self.dev)
        q3, dO3 = q.view(Bn, nq, D), dO.view(Bn, nq, D)
        for b in range(Bn):
            rows = slice(b * kp, (b + 1) * kp)
            op_gemm_tn(dS[b], q3[b], dkv32[rows, :D], atomics=False)                   # dK = dS^T . q
            op_gemm_tn(P[b], dO3[b], dkv32[rows, D:], atomics=False)                   # dV = P^T . dO
        return dq, TO.cast_bf16(dkv32)

    def _resid(self, A, wkey, bname, x, scale, rows_per_sample):
        """x += A . W^T + b (epilogue 2), or x += scale[sample] * (A . W^T + b) under drop-path."""
        if scale is None:
            op_gemm_nt(A, self.W[wkey], bias=self.P[bname].data, epilogue=2, C_inout=x)
        else:
            scale_rows_add(op_gemm_nt(A, self.W[wkey], bias=self.P[bname].data, epilogue=1), scale, x, rows_per_sample)

    def _ff_fwd(self, x: torch.Tensor, p: str, scale=None, rows_per_sample: int = 1) -> dict:
        sv = dict(x=x.clone())
        sv["h"] = self._ln(x, p + "norm")
        sv["u"] = op_gemm_nt(sv["h"], self.W[p + "w1"], bias=self.P[p + "fn.net.0.bias"].data)
        sv["hid"] = TO.geglu_fwd(sv["u"])
        self._resid(sv["hid"], p + "w2", p + "fn.net.2.bias", x, scale, rows_per_sample)
        return sv

    def _ff_bwd(self, sv, p, dbranch, dx, dxb):
        """dbranch bf16 = gradient w.r.t. the FF output; dx (fp32) / dxb (its bf16 copy) = the residual stream's gradient, accumulated."""
        self._lin_bwd(dbranch, sv["hid"], p + "fn.net.2.weight", p + "fn.net.2.bias")
        du = TO.geglu_bwd(sv["u"], op_gemm_nt(dbranch, self.W[p + "w2T"]))
        self._lin_bwd(du, sv["h"], p + "fn.net.0.weight", p + "fn.net.0.bias")
        self._ln_bwd(sv["x"], op_gemm_nt(du, self.W[p + "w1T"], epilogue=1), p + "norm", dx, dxb)

    def _self_attn_fwd(self, x: torch.Tensor, p: str, scale, Bn: int, M: int) -> dict:
        D = 512
        sv = dict(x=x.clone())
        sv["h"] = self._ln(x, p + "norm")
        qkv = op_gemm_nt(sv["h"], self.W[p + "qkv"])                                         # [B*M, 1536] = q | k | v
        q3 = qkv.view(Bn, M, 3 * D)
        sv["qkv"] = qkv
        sv["o"] = op_attention_vrow(q3[:, :, :D], q3[:, :, D:2 * D], q3[:, :, 2 * D:], self.H, HEAD ** -0.5).reshape(Bn * M, D)
        self._resid(sv["o"], p + "o", p + "fn.to_out.bias", x, scale, M)
        return sv

    def _self_attn_bwd(self, sv, p, dbranch, dx, dxb, Bn: int, M: int):
        D = 512
        self._lin_bwd(dbranch, sv["o"], p + "fn.to_out.weight", p + "fn.to_out.bias")
        dO = op_gemm_nt(dbranch, self.W[p + "oT"])
        qkv = sv["qkv"]
        dqkv = torch.empty_like(qkv)
        TO.attention_backward(qkv[:, :D], 3 * D, qkv[:, D:2 * D], 3 * D, qkv[:, 2 * D:], 3 * D, sv["o"], dO, Bn, self.H, M, M,
                              dqkv[:, :D], 3 * D, dqkv[:, D:2 * D], 3 * D, dqkv[:, 2 * D:], 3 * D)
        self._lin_bwd(dqkv[:, :D], sv["h"], p + "fn.to_q.weight")
        self._lin_bwd(dqkv[:, D:], sv["h"], p + "fn.to_kv.weight")
        self._ln_bwd(sv["x"], op_gemm_nt(dqkv, self.W[p + "qkvT"], epilogue=1), p + "norm", dx, dxb)

    def _cross_fwd(self, x: torch.Tensor, ctx: torch.Tensor, p: str, Bn: int, nq: int, kp: int, nk: int, resid: bool):
        """PreNorm(norm_context) + 1-head dim-512 Attention: x [Bn*nq, 512] fp32 queries, ctx [Bn*kp, 512] fp32 context.  resid: x += out
        in place; else returns the output (fp32)."""
        sv = dict(x=x.clone() if resid else x, ctx=ctx)
        sv["xn"] = self._ln(x, p + "norm")
        sv["cn"] = self._ln(ctx, p + "norm_context")
        sv["q"] = op_gemm_nt(sv["xn"], self.W[p + "q"])
        sv["kv"] = op_gemm_nt(sv["cn"], self.W[p + "kv"])
        sv["o"], sv["S"] = self._attn512_fwd(sv["q"], sv["kv"], Bn, nq, kp, nk)
        if resid:
            op_gemm_nt(sv["o"], self.W[p + "o"], bias=self.P[p + "fn.to_out.bias"].data, epilogue=2, C_inout=x)
            return sv, None
        return sv, op_gemm_nt(sv["o"], self.W[p + "o"], bias=self.P[p + "fn.to_out.bias"].data, epilogue=1)

    def _cross_bwd(self, sv, p, dout_b, dx, dxb, dctx, Bn: int, nq: int, kp: int, nk: int):
        """dout_b bf16 = gradient w.r.t. the block's output; accumulates the query side into dx (+ dxb) and the context side into dctx."""
        self._lin_bwd(dout_b, sv["o"], p + "fn.to_out.weight", p + "fn.to_out.bias")
        dO = op_gemm_nt(dout_b, self.W[p + "oT"])
        dq, dkv = self._attn512_bwd(sv["q"], sv["kv"], sv["o"], sv["S"], dO, Bn, nq, kp, nk)
        sv["S"] = None
        self._lin_bwd(dq, sv["xn"], p + "fn.to_q.weight")
        self._lin_bwd(dkv, sv["cn"], p + "fn.to_kv.weight")
        self._ln_bwd(sv["ctx"], op_gemm_nt(dkv, self.W[p + "kvT"], epilogue=1), p + "norm_context", dctx)
        self._ln_bwd(sv["x"], op_gemm_nt(dq, self.W[p + "qT"], epilogue=1), p + "norm", dx, dxb)

    # -- forward ----------------------------------------------------------------------------------------------------------------
    def forward(self, pc: torch.Tensor, queries: torch.Tensor, eps: torch.Tensor, masks: List[torch.Tensor]):
        """pc [B, N, 3], queries [B, Q, 3], eps [B, M, L] (the posterior noise), masks = ``n_masks`` drop-path scales [B] ->
        (logits [B, Q] fp32, kl [B] fp32, state for ``backward``)."""
        P, W, dev, D, H, L = self.P, self.W, self.dev, 512, self.H, self.L
        Bn, N, _ = pc.shape
        Q = queries.shape[1]
        M = (P["d_latents.weight"] if self.mix else P["latents.weight"]).shape[0]
        if len(masks) != self.n_masks:
            raise ValueError(f"AeTrainer.forward: {self.n_masks} drop-path masks expected, got {len(masks)}")
        if M % 128:
            raise NotImplementedError("AeTrainer: num_latents must be a multiple of 128")
        if N < 32:
            raise NotImplementedError("AeTrainer: at least 32 points per sample")
        Np = max(_round_up(N, 64), 128)              # keys padded per sample; >= 128 rows keeps the key-side gemm_tn atomic-free
        masks = [m.to(device=dev, dtype=torch.float32).reshape(Bn).contiguous() for m in masks]
        st = dict(Bn=Bn, N=N, Np=Np, Q=Q, M=M, masks=masks)
        # ---- points, padded per sample to a multiple of 64 rows (zero points: finite embeddings, masked as keys) ----------------
        pcp = torch.zeros(Bn, Np, 3, device=dev, dtype=torch.float32)
        pcp[:, :N] = pc.to(device=dev, dtype=torch.float32)
        pcp = pcp.view(Bn * Np, 3)
        emb = self._point_embed(pcp)                                                          # [B*Np, 512] fp32
        st.update(pcp=pcp, emb=emb)
        # ---- query tokens --------------------------------------------------------------------------------------------------------
        if self.mix:
            p = "mix_attn_layer."
            embb = TO.cast_bf16(emb)
            mx = dict(x=P["d_latents.weight"].data.repeat(Bn, 1).contiguous(), embb=embb)
            mx["h"] = self._ln(mx["x"], p + "norm")                                          # no norm_context: keys are the raw embeddings
            mx["q"] = op_gemm_nt(mx["h"], W[p + "q"])
            mx["kv"] = op_gemm_nt(embb, W[p + "kv"])                                           # [B*Np, 1024]
            kv3 = mx["kv"].view(Bn, Np, 2 * D)
            vT = TO.transpose(mx["kv"][:, D:], Np, D, 2 * D, Bn, Np * 2 * D).view(Bn, D, Np)
            mx["o"] = op_attention(mx["q"].view(Bn, M, D), kv3[:, :, :D], vT, N, H, HEAD ** -0.5).view(Bn * M, D)
            x0 = P["s_latents.weight"].data.repeat(Bn, 1).contiguous()
            self._resid(mx["o"], p + "o", p + "fn.to_out.bias", x0, masks[0], M)              # static + drop_path(dynamic), no residual
            mx["x0b"] = TO.cast_bf16(x0)
            x = op_gemm_nt(mx["x0b"], W["query_proj"], bias=P["query_proj.bias"].data, epilogue=1)
            st["mix"] = mx
        else:
            x = P["latents.weight"].data.repeat(Bn, 1).contiguous()
        # ---- cross_attend_blocks: attention onto the points (norm_context) + residual, FF + residual -----------------------------
        st["ca"], _ = self._cross_fwd(x, emb, "cross_attend_blocks.0.", Bn, M, Np, N, resid=True)
        st["cf"] = self._ff_fwd(x, "cross_attend_blocks.1.")
        # ---- posterior -------------------------------------------------------------------------------------------------------------
        x3b = TO.cast_bf16(x)
        ml = op_gemm_nt(x3b, W["mv"], bias=W["b_mv"], epilogue=1)                            # [B*M, 2L] raw mean | logvar
        eps_d = eps.to(device=dev, dtype=torch.float32).reshape(Bn * M, L).contiguous()
        z = _f32(Bn * M, L, device=dev)
        kl = _f32(Bn, device=dev)
        check(lib().rald_op_posterior(ml.data_ptr(), eps_d.data_ptr(), z.data_ptr(), kl.data_ptr(), Bn, M, L, _stream()))
        st.update(x3b=x3b, ml=ml, eps=eps_d)
        # ---- decoder: proj, latent stack ---------------------------------------------------------------------------------------------
        zb = TO.pad_channels(z, _round_up(L, 64))
        x = op_gemm_nt(zb, W["proj"], bias=P["proj.bias"].data, epilogue=1)                  # [B*M, 512]
        st["zb"] = zb
        layers = []
        for i in range(self.depth):
            sa = self._self_attn_fwd(x, f"layers.{i}.0.", masks[st_off(self.mix) + 2 * i], Bn, M)
            sf = self._ff_fwd(x, f"layers.{i}.1.", masks[st_off(self.mix) + 2 * i + 1], M)
            layers.append((sa, sf))
        st["layers"] = layers
        # ---- decoder cross-attention from the query points onto the latents, to_outputs -----------------------------------------------
        qp = queries.to(device=dev, dtype=torch.float32).reshape(Bn * Q, 3).contiguous()
        qe = self._point_embed(qp)
        st["dc"], lat = self._cross_fwd(qe, x, "decoder_cross_attn.", Bn, Q, M, M, resid=False)
        latb = TO.cast_bf16(lat)
        logits4 = op_gemm_nt(latb, W["to"], epilogue=1)                                     # [B*Q, 4], column 0 = logits - bias
        logits = (logits4[:, 0] + P["to_outputs.bias"].data).view(Bn, Q)
        st.update(qp=qp, latb=latb)
        return logits, kl, st

    # -- backward ---------------------------------------------------------------------------------------------------------------
    def backward(self, st: dict, dlogits: Optional[torch.Tensor], dkl: Optional[torch.Tensor]) -> None:
        """Accumulates into every ``param.grad`` the gradient of a scalar whose gradients w.r.t. logits [B, Q] and kl [B] are given
        (None = zero).  Consumes the state."""
        P, W, dev, D, L = self.P, self.W, self.dev, 512, self.L
        Bn, N, Np, Q, M, masks = st["Bn"], st["N"], st["Np"], st["Q"], st["M"], st["masks"]
        off = st_off(self.mix)
        if dlogits is None:
            dlogits = torch.zeros(Bn, Q, device=dev)
        dlog = dlogits.to(device=dev, dtype=torch.float32).reshape(Bn * Q, 1).contiguous()
        dkl_d = (dkl.to(device=dev, dtype=torch.float32).reshape(Bn).contiguous() if dkl is not None else torch.zeros(Bn, device=dev))
        # ---- to_outputs: logits = lat . w^T + b ------------------------------------------------------------------------------------
        gto, gtb = wgrad_narrow(dlog, st["latb"], 1)
        param_grad(P["to_outputs.weight"]).add_(gto)
        param_grad(P["to_outputs.bias"]).add_(gtb)
        dlat = _zeros(Bn * Q, D, device=dev)
        sgemm_acc(dlog, P["to_outputs.weight"].data, dlat, trans_b=True)                     # dlat = dlogits x w (K = 1)
        # ---- decoder cross-attention ------------------------------------------------------------------------------------------------
        dqe = _zeros(Bn * Q, D, device=dev)
        dxl = _zeros(Bn * M, D, device=dev)                                                  # gradient w.r.t. the latent stack's output
        self._cross_bwd(st["dc"], "decoder_cross_attn.", TO.cast_bf16(dlat), dqe, None, dxl, Bn, Q, M, M)
        del dlat
        pe_wgrad(dqe, st["qp"], self.basis, param_grad(P["point_embed.mlp.weight"]), param_grad(P["point_embed.mlp.bias"]))
        del dqe
        # ---- latent stack ---------------------------------------------------------------------------------------------------------
        dxb = TO.cast_bf16(dxl)
        for i in reversed(range(self.depth)):
            sa, sf = st["layers"][i]
            self._ff_bwd(sf, f"layers.{i}.1.", scale_rows_bf16(dxl, masks[off + 2 * i + 1], M), dxl, dxb)
            self._self_attn_bwd(sa, f"layers.{i}.0.", scale_rows_bf16(dxl, masks[off + 2 * i], M), dxl, dxb, Bn, M)
            st["layers"][i] = None
        # ---- proj, posterior ----------------------------------------------------------------------------------------------------------
        zb = st["zb"]
        gp = _zeros(D, zb.shape[1], device=dev)
        op_gemm_tn(dxb, zb, gp, param_grad(P["proj.bias"]), atomics=False)
        param_grad(P["proj.weight"]).add_(gp[:, :L])
        dz = op_gemm_nt(dxb, W["projT"], epilogue=1)                                        # [B*M, L]
        dml = _f32(Bn * M, 2 * L, device=dev)
        check(lib().rald_op_posterior_bwd(dz.data_ptr(), dkl_d.data_ptr(), st["ml"].data_ptr(), st["eps"].data_ptr(), dml.data_ptr(), Bn, M, L,
                                          _stream()))
        dmlb = TO.cast_bf16(dml)
        gmv, gmb = wgrad_narrow(dml, st["x3b"], 2 * L)
        param_grad(P["mean_fc.weight"]).add_(gmv[:L])
        param_grad(P["mean_fc.bias"]).add_(gmb[:L])
        param_grad(P["logvar_fc.weight"]).add_(gmv[L:])
        param_grad(P["logvar_fc.bias"]).add_(gmb[L:])
        dx = op_gemm_nt(dmlb, W["mvT"], epilogue=1)                                          # [B*M, 512]
        dxb = TO.cast_bf16(dx)
        # ---- cross_attend_blocks ------------------------------------------------------------------------------------------------------
        demb = _zeros(Bn * Np, D, device=dev)
        self._ff_bwd(st["cf"], "cross_attend_blocks.1.", dxb, dx, dxb)
        self._cross_bwd(st["ca"], "cross_attend_blocks.0.", dxb, dx, dxb, demb, Bn, M, Np, N)
        # ---- query tokens ------------------------------------------------------------------------------------------------------------
        if self.mix:
            mx, p = st["mix"], "mix_attn_layer."
            self._lin_bwd(dxb, mx["x0b"], "query_proj.weight", "query_proj.bias")
            dx0 = op_gemm_nt(dxb, W["query_projT"], epilogue=1)                              # d(static + dynamic)
            param_grad(P["s_latents.weight"]).add_(dx0.view(Bn, M, D).sum(0))
            dbranch = scale_rows_bf16(dx0, masks[0], M)
            self._lin_bwd(dbranch, mx["o"], p + "fn.to_out.weight", p + "fn.to_out.bias")
            dO = op_gemm_nt(dbranch, W[p + "oT"])
            dq = torch.empty_like(mx["q"])
            dkv = torch.zeros_like(mx["kv"])                                                 # key rows N .. Np-1 stay zero
            TO.attention_backward(mx["q"], D, mx["kv"], 2 * D, mx["kv"][:, D:], 2 * D, mx["o"], dO, Bn, self.H, M, N, dq, D, dkv, 2 * D, dkv[:, D:],
                                  2 * D, k_rows=Np)
            self._lin_bwd(dq, mx["h"], p + "fn.to_q.weight")
            self._lin_bwd(dkv, mx["embb"], p + "fn.to_kv.weight")
            op_gemm_nt(dkv, W[p + "kvT"], epilogue=2, C_inout=demb)
            dd = _zeros(Bn * M, D, device=dev)
            self._ln_bwd(mx["x"], op_gemm_nt(dq, W[p + "qT"], epilogue=1), p + "norm", dd)
            param_grad(P["d_latents.weight"]).add_(dd.view(Bn, M, D).sum(0))
        else:
            param_grad(P["latents.weight"]).add_(dx.view(Bn, M, D).sum(0))
        pe_wgrad(demb, st["pcp"], self.basis, param_grad(P["point_embed.mlp.weight"]), param_grad(P["point_embed.mlp.bias"]))
        st.clear()


def st_off(mix: bool) -> int:
    """Index of layers.0's attention mask in the drop-path list (the mix layer draws first)."""
    return 1 if mix else 0


class AeStepTrainer:
    """The reference's stage-1 iteration (engine_ae.py:55-116) on flat storage, as ``train_dit.EdmTrainer`` is for stage 2:

        opt = FlatAdamW(model.parameters(), lr=..., ema=True)
        step = AeStepTrainer(model, opt)
        losses, counts, grad_norm = step.step(surface, points, labels, in_voxel_num)

    One ``AeTrainer`` sits directly on the model's parameters: their ``.grad`` are views of ``opt.flat_g``, so ``backward`` fills the flat
    gradient with no shadow copies.  The loss, its metrics and its gradient are ``train_ops.ae_loss`` (two launches, no host sync);
    ``losses`` is the float64 device tensor [total, vol, near, kl], ``counts`` the int32 device tensor [B, 3] of ``ae_loss``.  ``logits``
    and ``kl`` of the last forward stay on the object."""

    def __init__(self, model, opt, reducer=None):
        named = dict(model.named_parameters())
        self.tr = AeTrainer(named, model.point_embed.basis, model.depth, model.latent_dim, model.query_type, heads=model.heads)
        base, end = opt.flat_g.data_ptr(), opt.flat_g.data_ptr() + opt.flat_g.numel() * 4
        for n, p in named.items():
            if p.grad is None or not base <= p.grad.data_ptr() < end:
                raise RuntimeError(f"AeStepTrainer: the gradient of {n} is not a view of opt.flat_g (build FlatAdamW over model.parameters())")
        self.model, self.opt, self.reducer = model, opt, reducer
        self.logits = self.kl = self.masks = None                   # of the last forward_backward
        self._window_open = False

    def refresh_weights(self) -> None:
        self.tr.refresh_weights()

    def draw(self, batch: int, eps=None, masks=None):
        """The reference's draws for what is not given, in the autograd route's order (models_ae.KLAutoEncoder._train_forward): timm's
        DropPath on the device RNG, then torch.randn on the CPU global RNG - one torch seed gives both routes the same masks and noise."""
        if masks is None:
            masks = drop_path_masks(batch, self.tr.n_masks, self.tr.dev)
        if eps is None:
            eps = torch.randn(batch, self.model.num_latents, self.model.latent_dim)
        return eps, masks

    def forward_backward(self, pc, queries, labels, in_voxel_num, eps=None, masks=None, grad_scale: float = 1.0, vol_weight: float = 1.0,
                         near_weight: float = 0.1, kl_weight: float = 1e-3):
        """AeTrainer.forward -> ae_loss -> AeTrainer.backward(st, dlogits, dkl): accumulates the gradient of grad_scale * loss into the flat
        gradient.  Returns (losses, counts) as device tensors."""
        eps, masks = self.draw(pc.shape[0], eps, masks)
        self.masks = masks
        logits, kl, st = self.tr.forward(pc, queries, eps, masks)
        losses, counts, dlogits, dkl = TO.ae_loss(logits, labels.to(self.tr.dev), kl, in_voxel_num, vol_weight, near_weight, kl_weight, grad_scale)
        self.tr.backward(st, dlogits, dkl)
        self.logits, self.kl = logits, kl
        return losses, counts

    def _begin(self) -> None:
        if not self._window_open:                                   # optimizer.zero_grad() at :46 and after every update (:111-112)
            self.opt.zero_grad()
            self._window_open = True

    def _finish(self, update: bool, max_norm, ema_rate: float, refresh):
        """engine_ae.py:107-116 after the backward pass: on an update iteration clip, AdamW with the EMA in the same pass, and the bf16
        copies; otherwise the EMA alone (the reference updates it every iteration)."""
        if not update:
            self.opt.update_ema(ema_rate)
            return None
        pre = 1.0
        if self.reducer is not None:
            self.reducer.start()
            pre = self.reducer.finish()
        norm = self.opt.clip_grad_norm_(max_norm, pre_scale=pre)
        self.opt.step(ema_rate=ema_rate)
        refresh()
        self._window_open = False
        return norm

    def step(self, pc, queries, labels, in_voxel_num, eps=None, masks=None, update: bool = True, accum_iter: int = 1, max_norm=None,
             ema_rate: float = 0.999, vol_weight: float = 1.0, near_weight: float = 0.1, kl_weight: float = 1e-3):
        """One iteration: ``update`` is the reference's ``(data_iter_step + 1) % accum_iter == 0``.  Returns (losses, counts, total gradient
        norm or None) - device tensors, no host sync."""
        self._begin()
        losses, counts = self.forward_backward(pc, queries, labels, in_voxel_num, eps, masks, 1.0 / accum_iter, vol_weight, near_weight, kl_weight)
        return losses, counts, self._finish(update, max_norm, ema_rate, self.tr.refresh_weights)


class GraphedAeStep:
    """``AeStepTrainer.step`` with its launches captured in two hipGraphs (torch.cuda.CUDAGraph on the current stream), after the pattern of
    ``train_dit.GraphedTrainStep``:
      graph A = forward + loss + backward on static input buffers (pc, queries, labels, eps, the drop-path scales as one [n_masks, B]
                tensor, the int32 in_voxel_num the loss kernels read),
      eager   = zero_grad when an accumulation window starts, the mask / noise draws, the input copies, clip + fused AdamW / EMA (or the EMA
                alone between updates), the optional reducer,
      graph B = refresh of the bf16 weight copies.
    Shapes, the loss weights and accum_iter (it is the gradient scale inside graph A) are fixed at construction.  The trainer's bf16 copies
    live in graph B's pool afterwards: drive the trainer through this object only.  The returned tensors are the graphs' static outputs,
    rewritten by the next call."""

    def __init__(self, step_trainer: AeStepTrainer, B: int, N: int, Q: int, accum_iter: int = 1, vol_weight: float = 1.0, near_weight: float = 0.1,
                 kl_weight: float = 1e-3):
        self.st, self.B, self.N, self.Q = step_trainer, B, N, Q
        tr, opt, m = step_trainer.tr, step_trainer.opt, step_trainer.model
        dev = tr.dev
        self.fixed = dict(accum_iter=int(accum_iter), vol_weight=float(vol_weight), near_weight=float(near_weight), kl_weight=float(kl_weight))
        z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self.pc, self.queries, self.labels, self.eps = z(B, N, 3), z(B, Q, 3), z(B, Q), z(B, m.num_latents, m.latent_dim)
        self.masks = torch.full((tr.n_masks, B), 1.0 / (1.0 - DROP_PATH_RATE), device=dev, dtype=torch.float32)
        self.n_in = torch.full((1,), Q // 2, device=dev, dtype=torch.int32)
        fb = lambda: step_trainer.forward_backward(self.pc, self.queries, self.labels, self.n_in, eps=self.eps, masks=list(self.masks.unbind(0)),
                                                   grad_scale=1.0 / accum_iter, vol_weight=vol_weight, near_weight=near_weight,
                                                   kl_weight=kl_weight)
        grad = opt.flat_g.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                          # warm-up outside capture (lazy allocations, function attributes)
            fb()
            tr.refresh_weights()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.g_refresh = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_refresh):
            tr.refresh_weights()                               # tr.W now lives in the graph's pool, rewritten by every replay
        self.g_fb = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_fb):
            self.losses, self.counts = fb()
        self.logits, self.kl = step_trainer.logits, step_trainer.kl
        opt.flat_g.copy_(grad)                                 # the warm-up pass and the capture leave the gradient as they found it
        self.g_refresh.replay()

    def __call__(self, pc, queries, labels, in_voxel_num, eps=None, masks=None, update: bool = True, accum_iter: int = None, max_norm=None,
                 ema_rate: float = 0.999, vol_weight: float = None, near_weight: float = None, kl_weight: float = None):
        """``AeStepTrainer.step`` with the same arguments; accum_iter and the weights, when given, must be those of the capture."""
        for k, v in dict(accum_iter=accum_iter, vol_weight=vol_weight, near_weight=near_weight, kl_weight=kl_weight).items():
            if v is not None and float(v) != float(self.fixed[k]):
                raise ValueError(f"GraphedAeStep: {k}={v} differs from the captured {self.fixed[k]}")
        if tuple(pc.shape) != (self.B, self.N, 3) or tuple(queries.shape) != (self.B, self.Q, 3) or tuple(labels.shape) != (self.B, self.Q):
            raise ValueError(f"GraphedAeStep: captured for pc [{self.B},{self.N},3], queries [{self.B},{self.Q},3], labels [{self.B},{self.Q}]")
        st = self.st
        st._begin()
        eps, masks = st.draw(self.B, eps, masks)
        self.pc.copy_(pc, non_blocking=True)
        self.queries.copy_(queries, non_blocking=True)
        self.labels.copy_(labels, non_blocking=True)
        self.eps.copy_(eps, non_blocking=True)
        self.masks.copy_(torch.stack([m.reshape(self.B) for m in masks]), non_blocking=True)
        if isinstance(in_voxel_num, torch.Tensor):
            self.n_in.copy_(in_voxel_num.reshape(1), non_blocking=True)
        else:
            self.n_in.fill_(int(in_voxel_num))
        self.g_fb.replay()
        return self.losses, self.counts, st._finish(update, max_norm, ema_rate, self.g_refresh.replay)
