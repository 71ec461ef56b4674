"""The training-side kernel wrappers of all three trainers: the denoiser (train_dit.py), the radar encoder (train_encoder.py) and
the autoencoder (train_ae.py).  A training entry point of the library that more than one trainer uses is called from here only.

Backward pass of the denoiser's transformer block on the HIP kernels ("backward
kernels for K2-K5").  ``block_forward`` / ``block_backward`` restate what autograd derives for
``BasicTransformerBlock`` (models_radar_generation.py:133-169: AdaLayerNorm -> self-attention -> AdaLayerNorm ->
radar cross-attention -> AdaLayerNorm -> GEGLU feed-forward, residual after each) as explicit launches:
every product is a bf16 MFMA GEMM through ``rald_op_gemm_nt[2]`` (fp32 accumulate; dX = dY.W with the
transposed weight, dW = dY^T.X with transposed activations), everything else a streaming kernel of
``csrc/train_kernels.hip``.  PyTorch only owns the buffers.

Attention backward is two fused launches (csrc/attn_bwd.hip: a query-side and a key-side kernel that recompute the
probabilities from the log-sum-exp, flash-attention style); shapes they do not cover take the unfused form: S = Q.K^T
and dP = dO.V^T per head as batched K = 64 GEMMs, the softmax backward element-wise, the key-side gradients in the
transposed orientation.

Gradient parity against autograd of the CPU oracle: tests/test_train_block.py (one block, whole denoiser);
the loop over blocks, embeddings and loss live in train_dit.py, the radar encoder in train_encoder.py, the autoencoder in train_ae.py.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ._handles import _opt, _stream, op_attention, op_attention_vrow, op_gemm_nt, op_gemm_tn, op_layernorm
from ._lib import check, lib

HEAD = 64


def param_grad(p: torch.nn.Parameter) -> torch.Tensor:
    """p.grad, created as zeros on first use: the trainers accumulate every gradient into it."""
    if p.grad is None:
        p.grad = torch.zeros_like(p.data)
    return p.grad


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    check(lib().rald_op_cast_bf16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()))
    return out


def gemm2(A, lda, sA, sA2, B, ldb, sB, sB2, out, ldc, sC, sC2, M, N, K, batch, batch2, epilogue=0, alpha=1.0, bias=None):
    """C = alpha * A.B^T (+bias) with an outer and an inner batch; operands are (tensor-with-offset, ld, strides)."""
    check(lib().rald_op_gemm_nt2(A.data_ptr(), lda, sA, sA2, B.data_ptr(), ldb, sB, sB2, out.data_ptr(), ldc, sC, sC2, _opt(bias), M, N, K, batch,
                                 batch2, alpha, epilogue, _stream()))
    return out


def transpose(x: torch.Tensor, rows: int, cols: int, ld_in: int, batch: int = 1, stride_in: int = 0, batch2: int = 1, stride_in2: int = 0):
    """[batch][batch2] matrices of `rows` x `cols` inside x (f32 or bf16) -> bf16 [batch, batch2, cols, rows]."""
    out = torch.empty(batch, batch2, cols, rows, device=x.device, dtype=torch.bfloat16)
    check(lib().rald_op_transpose(x.data_ptr(), int(x.dtype == torch.bfloat16), ld_in, stride_in, stride_in2, out.data_ptr(), rows,
                                  batch2 * cols * rows, cols * rows, rows, cols, batch, batch2, _stream()))
    return out


def T2(x: torch.Tensor) -> torch.Tensor:
    """plain [R, C] -> bf16 [C, R]"""
    return transpose(x, x.shape[0], x.shape[1], x.stride(0)).reshape(x.shape[1], x.shape[0])


def ln_mod_bwd(x, dh, scale, gstride, rows_per_group, add_one, dx, dscale, dshift, eps=1e-5, dx_bf16=None):
    """dx += LayerNorm-mod backward of dh (fp32, in place); dx_bf16 (optional, bf16 [rows, 512]) receives the updated dx rounded to bf16."""
    check(lib().rald_op_ln_mod_bwd(x.data_ptr(), dh.data_ptr(), scale.data_ptr(), gstride, rows_per_group, add_one, eps, x.shape[0], x.shape[1],
                                   dx.data_ptr(), _opt(dx_bf16), dscale.data_ptr(), dshift.data_ptr(), _stream()))


def geglu_fwd(u: torch.Tensor) -> torch.Tensor:
    M, two_i = u.shape
    hid = torch.empty(M, two_i // 2, device=u.device, dtype=torch.bfloat16)
    check(lib().rald_op_geglu_fwd(u.data_ptr(), hid.data_ptr(), M, two_i // 2, _stream()))
    return hid


def geglu_bwd(u: torch.Tensor, dhid: torch.Tensor) -> torch.Tensor:
    du = torch.empty_like(u)
    check(lib().rald_op_geglu_bwd(u.data_ptr(), dhid.data_ptr(), du.data_ptr(), u.shape[0], u.shape[1] // 2, _stream()))
    return du


def lin_wgrad(dy: torch.Tensor, x_in: torch.Tensor, dW: torch.Tensor, dbias: Optional[torch.Tensor] = None, atomics: Optional[bool] = None) -> None:
    """dW [N1, N2] f32 += dy^T . x_in for dy [M, N1], x_in [M, N2] (bf16, or f32: cast first); dbias [N1] += column sums of dy.
    atomics: the form of ``op_gemm_tn``; None picks it by the size of dW (the denoiser and the encoder), False always takes the workspace
    form (the autoencoder: its backward pass is bit-reproducible)."""
    if dy.dtype != torch.bfloat16:
        dy = cast_bf16(dy)
    if x_in.dtype != torch.bfloat16:
        x_in = cast_bf16(x_in)
    if atomics is None:
        # large gradients: the row ranges meet in a workspace and are summed in order (no atomics: reproducible, and 59 -> 38 us for ff.net.2
        # at 4 096 rows); a 512 x 512 gradient has too few ranges for the extra launch to pay (20.9 vs 24.0 us)
        atomics = dy.shape[1] * x_in.shape[1] < 512 * 1024
    op_gemm_tn(dy, x_in, dW, dbias, atomics=atomics)


def sgemm_acc(A, B, out, trans_a=False, trans_b=False, alpha=1.0, M=None, N=None, K=None):
    """out[m, n] += alpha * sum_k A(m, k) B(n, k) in fp32 (see rald_op_sgemm_acc)."""
    M = M if M is not None else (A.shape[1] if trans_a else A.shape[0])
    K = K if K is not None else (A.shape[0] if trans_a else A.shape[1])
    N = N if N is not None else (B.shape[1] if trans_b else B.shape[0])
    check(lib().rald_op_sgemm_acc(A.data_ptr(), A.stride(0), int(trans_a), B.data_ptr(), B.stride(0), int(trans_b), out.data_ptr(), out.stride(0), M,
                                  N, K, alpha, _stream()))
    return out


def colsum(x: torch.Tensor, out: torch.Tensor) -> None:
    """out[n] += sum_m x[m, n]"""
    check(lib().rald_op_colsum(x.data_ptr(), int(x.dtype == torch.bfloat16), x.stride(0), x.shape[0], x.shape[1], out.data_ptr(), _stream()))


def attention_backward(q, ldq, k, ldk, v, ldv, O, dO, Bn: int, H: int, nq: int, nk: int, dq, ld_dq, dk, ld_dk, dv, ld_dv, k_rows: int = 0):
    """Gradients of O = softmax(q k^T / 8) v per head (models_radar_generation.py:56-74).  q/k/v/dq/dk/dv are bf16
    tensors (possibly column slices of a fused buffer: pass the slice and its row stride); O, dO [Bn*nq, H*64] bf16.
    The key-side buffers (k, v, dk, dv) hold nk rows per sample, or k_rows >= nk when given: the autoencoder's mix attention keeps its nk
    point embeddings in a buffer padded to a multiple of 64 rows.
    Two launches of csrc/attn_bwd.hip (nothing score-shaped in memory; the last key tile is masked when nk % 64 != 0) when nq % 128 == 0
    and the key rows per sample are a multiple of 64 - the denoiser's 512 latents x 512 / 64 keys, the autoencoder's 512 latents; other
    shapes take the unfused GEMM form below (nk rows per sample)."""
    k_rows = k_rows or nk
    if nq % 128 or k_rows % 64:
        assert k_rows == nk, "attention_backward: the unfused form reads nk key rows per sample"
        return attention_backward_unfused(q, ldq, k, ldk, v, ldv, O, dO, Bn, H, nq, nk, dq, ld_dq, dk, ld_dk, dv, ld_dv)
    scratch = torch.empty(2, Bn * H * nq, device=O.device, dtype=torch.float32)
    check(lib().rald_op_attention_bwd(q.data_ptr(), ldq, nq * ldq, k.data_ptr(), ldk, k_rows * ldk, v.data_ptr(), ldv, k_rows * ldv, O.data_ptr(),
                                      O.stride(0), nq * O.stride(0), dO.data_ptr(), dO.stride(0), nq * dO.stride(0), dq.data_ptr(), ld_dq,
                                      nq * ld_dq, dk.data_ptr(), ld_dk, k_rows * ld_dk, dv.data_ptr(), ld_dv, k_rows * ld_dv, scratch[0].data_ptr(),
                                      scratch[1].data_ptr(), nq, nk, H, Bn, HEAD ** -0.5, _stream()))


def attention_backward_unfused(q, ldq, k, ldk, v, ldv, O, dO, Bn: int, H: int, nq: int, nk: int, dq, ld_dq, dk, ld_dk, dv, ld_dv):
    """The same gradients as batched GEMMs + element-wise passes (any nq, nk): S = Q.K^T and dP = dO.V^T per head as K = 64 GEMMs
    with fp32 results, the softmax backward element-wise, the key side in the transposed orientation."""
    dev, scale = O.device, HEAD ** -0.5
    f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    b16 = lambda *s: torch.empty(*s, device=dev, dtype=torch.bfloat16)
    S, dP = f32(Bn, H, nq, nk), f32(Bn, H, nq, nk)
    gemm2(q, ldq, nq * ldq, HEAD, k, ldk, nk * ldk, HEAD, S, nk, H * nq * nk, nq * nk, nq, nk, HEAD, Bn, H, epilogue=1)
    gemm2(dO, H * HEAD, nq * H * HEAD, HEAD, v, ldv, nk * ldv, HEAD, dP, nk, H * nq * nk, nq * nk, nq, nk, HEAD, Bn, H, epilogue=1)
    lse, delta = row_lse(S, scale), f32(Bn, H, nq)
    check(lib().rald_op_rowdot_heads(dO.data_ptr(), O.data_ptr(), Bn * nq, H, nq, delta.data_ptr(), _stream()))
    dS = b16(Bn, H, nq, nk)
    attn_bwd_elem(S, dP, lse, delta, Bn * H, nq, nk, nq, 1, scale, 0, None, dS)
    kT = transpose(k, nk, HEAD, ldk, Bn, nk * ldk, H, HEAD)                     # [Bn, H, 64, nk]
    gemm2(dS, nk, H * nq * nk, nq * nk, kT, nk, H * HEAD * nk, HEAD * nk, dq, ld_dq, nq * ld_dq, HEAD, nq, HEAD, nk, Bn, H)
    # key side: transposed orientation
    ST, dPT = f32(Bn, H, nk, nq), f32(Bn, H, nk, nq)
    gemm2(k, ldk, nk * ldk, HEAD, q, ldq, nq * ldq, HEAD, ST, nq, H * nk * nq, nk * nq, nk, nq, HEAD, Bn, H, epilogue=1)
    gemm2(v, ldv, nk * ldv, HEAD, dO, H * HEAD, nq * H * HEAD, HEAD, dPT, nq, H * nk * nq, nk * nq, nk, nq, HEAD, Bn, H, epilogue=1)
    PT, dST = b16(Bn, H, nk, nq), b16(Bn, H, nk, nq)
    attn_bwd_elem(ST, dPT, lse, delta, Bn * H, nk, nq, nq, 1, scale, 1, PT, dST)
    qT = transpose(q, nq, HEAD, ldq, Bn, nq * ldq, H, HEAD)                     # [Bn, H, 64, nq]
    dOT = transpose(dO, nq, HEAD, H * HEAD, Bn, nq * H * HEAD, H, HEAD)
    gemm2(dST, nq, H * nk * nq, nk * nq, qT, nq, H * HEAD * nq, HEAD * nq, dk, ld_dk, nk * ld_dk, HEAD, nk, HEAD, nq, Bn, H)
    gemm2(PT, nq, H * nk * nq, nk * nq, dOT, nq, H * HEAD * nq, HEAD * nq, dv, ld_dv, nk * ld_dv, HEAD, nk, HEAD, nq, Bn, H)


def row_lse(S: torch.Tensor, scale: float) -> torch.Tensor:
    """fp32 S [..., cols] -> lse [...] fp32 = log sum_c exp(scale * S[..., c])."""
    lse = torch.empty(S.shape[:-1], device=S.device, dtype=torch.float32)
    check(lib().rald_op_row_lse(S.data_ptr(), lse.numel(), S.shape[-1], scale, lse.data_ptr(), _stream()))
    return lse


def attn_bwd_elem(S, dP, lse, delta, batch: int, R: int, cols: int, vbatch_stride: int, vstride: int, scale: float, by_col: int,
                  P: Optional[torch.Tensor], dS: torch.Tensor) -> None:
    """Softmax backward of S [batch][R][cols] (fp32 scores, dP their gradient), element-wise: P = exp(scale*S - lse[i]) (bf16, optional),
    dS = P*(dP - delta[i])*scale (bf16), i = the row (by_col 0) or the column (by_col 1); see rald_op_attn_bwd_elem."""
    check(lib().rald_op_attn_bwd_elem(S.data_ptr(), dP.data_ptr(), lse.data_ptr(), delta.data_ptr(), batch, R, cols, vbatch_stride, vstride, scale,
                                      by_col, _opt(P), dS.data_ptr(), _stream()))


def rowdot(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bf16 a, b [M, C] -> fp32 [M] of the row dot products (the delta = <dO, O> of a 1-head attention backward)."""
    out = torch.empty(a.shape[0], device=a.device, dtype=torch.float32)
    check(lib().rald_op_rowdot(a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], out.data_ptr(), _stream()))
    return out


def softmax_rows(S: torch.Tensor, n: int) -> torch.Tensor:
    """fp32 S [..., ld] -> bf16 P of the same shape: the softmax of each row's first n entries, zero past them."""
    P = torch.empty(S.shape, device=S.device, dtype=torch.bfloat16)
    ld = S.shape[-1]
    check(lib().rald_op_softmax_rows(S.data_ptr(), ld, P.data_ptr(), ld, S.numel() // ld, n, _stream()))
    return P


def pad_channels(x: torch.Tensor, cols: int) -> torch.Tensor:
    """fp32 [..., C] -> bf16 [..., cols] with zero columns C .. cols-1."""
    out = torch.empty(*x.shape[:-1], cols, device=x.device, dtype=torch.bfloat16)
    check(lib().rald_op_pad_channels(x.data_ptr(), out.data_ptr(), x.numel() // x.shape[-1], x.shape[-1], cols, _stream()))
    return out


def ae_loss(logits: torch.Tensor, labels: torch.Tensor, kl: torch.Tensor, in_voxel_num, vol_weight: float = 1.0, near_weight: float = 0.1,
            kl_weight: float = 1e-3, grad_scale: float = 1.0, want_grad: bool = True):
    """The autoencoder's stage-1 loss on the device (engine_ae.py:70-101; csrc/ae_train.hip): fp32 logits / labels [B, Q] (labels 0 or 1),
    kl [B] -> (losses float64 [4] = [vol_weight vol + near_weight near + kl_weight kl, vol, near, kl], counts int32 [B, 3] =
    (#(pred == label), #(pred and label), #(pred or label)) with pred = logits >= 0, dlogits [B, Q], dkl [B]); the gradients are those of
    grad_scale * total, None when want_grad is False (evaluation).  ``in_voxel_num`` reaches the kernels as one int32 in device memory (the same captured
    graph serves any split point): a device int32 tensor of one element passes as it is, a Python int or another tensor is copied there
    first.  No host sync."""
    B, Q = logits.shape
    dev = logits.device
    if not (logits.is_cuda and labels.is_cuda and kl.is_cuda):
        raise RuntimeError("ae_loss runs on the HIP device only (no CPU fallback)")
    if labels.shape != logits.shape or kl.numel() != B:
        raise ValueError(f"ae_loss: logits {tuple(logits.shape)}, labels {tuple(labels.shape)} and kl {tuple(kl.shape)} do not belong together")
    if not isinstance(in_voxel_num, torch.Tensor):
        in_voxel_num = torch.tensor([int(in_voxel_num)], dtype=torch.int32)
    if in_voxel_num.numel() != 1:
        raise ValueError("ae_loss: in_voxel_num must be a Python int or a tensor of one element")
    in_voxel_num = in_voxel_num.reshape(1).to(device=dev, dtype=torch.int32)          # the graphed step's int32 device buffer passes as it is
    f32c = lambda t: t.detach().to(torch.float32).contiguous()
    logits, labels, kl = f32c(logits), f32c(labels), f32c(kl)
    losses = torch.empty(4, device=dev, dtype=torch.float64)
    counts = torch.empty(B, 3, device=dev, dtype=torch.int32)
    dlogits = torch.empty(B, Q, device=dev, dtype=torch.float32) if want_grad else None
    dkl = torch.empty(B, device=dev, dtype=torch.float32) if want_grad else None
    nbytes = lib().rald_op_ae_loss_scratch_bytes(B, Q)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    check(lib().rald_op_ae_loss(logits.data_ptr(), labels.data_ptr(), kl.data_ptr(), in_voxel_num.data_ptr(), B, Q, float(vol_weight),
                                float(near_weight), float(kl_weight), float(grad_scale), losses.data_ptr(), counts.data_ptr(), _opt(dlogits),
                                _opt(dkl), scratch.data_ptr(), nbytes, _stream()))
    return losses, counts, dlogits, dkl


def prepare_block_weights(sd: Dict[str, torch.Tensor], prefix: str, device) -> Dict[str, torch.Tensor]:
    """bf16 compute copies (and their transposes for the dX products) of one block's fp32 master weights."""
    g = lambda n: sd[prefix + n].to(device=device, dtype=torch.float32)
    b16 = lambda t: t.to(torch.bfloat16).contiguous()
    W = {"qkv": b16(torch.cat([g("attn1.to_q.weight"), g("attn1.to_k.weight"), g("attn1.to_v.weight")], 0)),
         "o": b16(g("attn1.to_out.0.weight")), "bo": g("attn1.to_out.0.bias").contiguous(),
         "q2": b16(g("attn2.to_q.weight")), "k2": b16(g("attn2.to_k.weight")), "v2": b16(g("attn2.to_v.weight")),
         "o2": b16(g("attn2.to_out.0.weight")), "bo2": g("attn2.to_out.0.bias").contiguous(),
         "w1": b16(g("ff.net.0.proj.weight")), "b1": g("ff.net.0.proj.bias").contiguous(),
         "w2": b16(g("ff.net.2.weight")), "b2": g("ff.net.2.bias").contiguous()}
    for n in ("qkv", "o", "q2", "k2", "v2", "o2", "w1", "w2"):
        W[n + "T"] = T2(W[n])
    return W


def block_forward(W, x: torch.Tensor, mod: torch.Tensor, cond: torch.Tensor, Bn: int, NL: int, H: int = 8):
    """x [Bn*NL, 512] f32 (updated in place), mod [Bn, 3, 1024] f32 = (scale | shift) of norm1..3 (may be a strided
    view of the whole model's table), cond [Bn*T, Cd] bf16.  Returns the saved activations for ``block_backward``."""
    D, M, T = H * HEAD, Bn * NL, cond.shape[0] // Bn
    sv = {"mod": mod, "cond": cond, "Bn": Bn, "NL": NL, "H": H, "T": T}
    ln = lambda j: op_layernorm(x, mod[:, j, :D], mod[:, j, D:], gstride=mod.stride(0), rows_per_group=NL, add_one=1.0)
    sv["x0"] = x.clone()
    sv["h1"] = ln(0)
    qkv = op_gemm_nt(sv["h1"], W["qkv"])                                          # [M, 1536]
    q3 = qkv.view(Bn, NL, 3 * D)
    if NL % 64 == 0:                                                                # V read row-major from the fused buffer (no transposed copy)
        o1 = op_attention_vrow(q3[:, :, :D], q3[:, :, D:2 * D], q3[:, :, 2 * D:], H, HEAD ** -0.5)
    else:
        vt = transpose(qkv[:, 2 * D:], NL, D, 3 * D, Bn, NL * 3 * D).reshape(Bn, D, NL)
        o1 = op_attention(q3[:, :, :D], q3[:, :, D:2 * D], vt, NL, H, HEAD ** -0.5)
    sv["qkv"], sv["o1"] = qkv, o1.reshape(M, D)
    op_gemm_nt(sv["o1"], W["o"], bias=W["bo"], epilogue=2, C_inout=x)
    sv["x1"] = x.clone()
    sv["h2"] = ln(1)
    sv["q2"] = op_gemm_nt(sv["h2"], W["q2"])
    sv["kc"], sv["vc"] = op_gemm_nt(cond, W["k2"]), op_gemm_nt(cond, W["v2"])     # [Bn*T, 512]
    if T % 64 == 0:
        sv["o2"] = op_attention_vrow(sv["q2"].view(Bn, NL, D), sv["kc"].view(Bn, T, D), sv["vc"].view(Bn, T, D), H, HEAD ** -0.5).reshape(M, D)
    else:
        vct = transpose(sv["vc"], T, D, D, Bn, T * D).reshape(Bn, D, T)
        sv["o2"] = op_attention(sv["q2"].view(Bn, NL, D), sv["kc"].view(Bn, T, D), vct, T, H, HEAD ** -0.5).reshape(M, D)
    op_gemm_nt(sv["o2"], W["o2"], bias=W["bo2"], epilogue=2, C_inout=x)
    sv["x2"] = x.clone()
    sv["h3"] = ln(2)
    sv["u"] = op_gemm_nt(sv["h3"], W["w1"], bias=W["b1"])                         # [M, 4096] = [a | g]
    sv["hid"] = geglu_fwd(sv["u"])
    op_gemm_nt(sv["hid"], W["w2"], bias=W["b2"], epilogue=2, C_inout=x)
    return sv


def block_backward(W, sv, dx: torch.Tensor, dmod: torch.Tensor = None, grads: Dict[str, torch.Tensor] = None, dxb: torch.Tensor = None):
    """dx [M, 512] f32 = gradient w.r.t. the block's output; on return it holds the gradient w.r.t. its input.
    ``dmod`` (same shape AND strides as the ``mod`` given to block_forward, accumulated into) and ``grads`` (fp32
    destinations keyed like ``prepare_block_weights``, accumulated into - e.g. views of the flat gradient) are
    allocated when omitted.  ``dxb`` (optional): a bf16 [M, 512] buffer that holds bf16(dx) on entry and on return (every
    LayerNorm backward of the block writes it beside dx, so no separate cast pass runs between the sub-blocks; the caller hands
    the same buffer from block to block).  Returns (grads, dmod, dcond [Bn*T, Cd] f32)."""
    Bn, NL, H, T, mod, cond = sv["Bn"], sv["NL"], sv["H"], sv["T"], sv["mod"], sv["cond"]
    D, M, dev = H * HEAD, Bn * NL, dx.device
    G: Dict[str, torch.Tensor] = grads if grads is not None else {}
    if dmod is None:
        dmod = torch.zeros_like(mod)
    if dmod.stride() != mod.stride():
        raise ValueError("block_backward: dmod must have the strides of mod")
    zeros = lambda *n: torch.zeros(*n, device=dev, dtype=torch.float32)
    ms = mod.stride(0)

    def lin_bwd(dy, x_in, name, bias=None):
        """G[name] += dy^T . x_in (and G[bias] += column sums of dy): one launch of the row-contracting GEMM (csrc/gemm_tn.hip) on the
        operands as they lie - no transposed copies, the bias gradient from the same pass"""
        if name not in G:
            G[name] = zeros(dy.shape[1], x_in.shape[1])
        if bias is not None and bias not in G:
            G[bias] = zeros(dy.shape[1])
        lin_wgrad(dy, x_in, G[name], G[bias] if bias is not None else None)

    if dxb is None:
        dxb = cast_bf16(dx)

    def ada_bwd(j, x_saved, dh):
        ln_mod_bwd(x_saved, dh, mod[:, j, :D], ms, NL, 1.0, dx, dmod[:, j, :D], dmod[:, j, D:], dx_bf16=dxb)

    # ---- feed-forward: x3 = x2 + hid.W2^T + b2 --------------------------------------------------------
    lin_bwd(dxb, sv["hid"], "w2", "b2")
    du = geglu_bwd(sv["u"], op_gemm_nt(dxb, W["w2T"]))                              # [M, 4096]
    lin_bwd(du, sv["h3"], "w1", "b1")
    ada_bwd(2, sv["x2"], op_gemm_nt(du, W["w1T"], epilogue=1))
    # ---- cross-attention: x2 = x1 + o2.Wo2^T + bo2 ---------------------------------------------------
    lin_bwd(dxb, sv["o2"], "o2", "bo2")
    dO2 = op_gemm_nt(dxb, W["o2T"])
    dq2 = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    dkc, dvc = torch.empty(Bn * T, D, device=dev, dtype=torch.bfloat16), torch.empty(Bn * T, D, device=dev, dtype=torch.bfloat16)
    attention_backward(sv["q2"], D, sv["kc"], D, sv["vc"], D, sv["o2"], dO2, Bn, H, NL, T, dq2, D, dkc, D, dvc, D)
    lin_bwd(dq2, sv["h2"], "q2")
    lin_bwd(dkc, cond, "k2")
    lin_bwd(dvc, cond, "v2")
    dcond = op_gemm_nt(dkc, W["k2T"], epilogue=1)
    op_gemm_nt(dvc, W["v2T"], epilogue=2, C_inout=dcond)
    ada_bwd(1, sv["x1"], op_gemm_nt(dq2, W["q2T"], epilogue=1))
    # ---- self-attention: x1 = x0 + o1.Wo^T + bo ------------------------------------------------------
    lin_bwd(dxb, sv["o1"], "o", "bo")
    dO1 = op_gemm_nt(dxb, W["oT"])
    qkv = sv["qkv"]
    dqkv = torch.empty_like(qkv)
    attention_backward(qkv[:, :D], 3 * D, qkv[:, D:2 * D], 3 * D, qkv[:, 2 * D:], 3 * D, sv["o1"], dO1, Bn, H, NL, NL,
                       dqkv[:, :D], 3 * D, dqkv[:, D:2 * D], 3 * D, dqkv[:, 2 * D:], 3 * D)
    lin_bwd(dqkv, sv["h1"], "qkv")
    ada_bwd(0, sv["x0"], op_gemm_nt(dqkv, W["qkvT"], epilogue=1))
    return G, dmod, dcond
