"""CPU ORACLE (test infrastructure only) for the MXFP8 format of the fp8 QKV/proj path (BASELINE config
#5): OCP Microscaling Formats v1.0 - blocks of 32 consecutive K elements share one e8m0 scale, the
smallest power of two with amax / scale <= 448 (= 2^(floor(log2 amax) - 8), one more when amax's mantissa
exceeds 1.75, so nothing saturates); elements are e4m3fn, round-to-nearest-even.  The reference has no fp8 path (fp32 throughout), so there is no golden vector for this format:
the restatement is pinned by (a) torch's own float8_e4m3fn conversion for the element rounding and (b)
exact-integer GEMM identities in tests/test_fp8.py; model-level parity of the fp8 mode is measured
against the same fp32 goldens as the bf16 mode."""
import numpy as np
import torch


def quantize_mx8(x):
    """x [..., K] float -> (q uint8 e4m3 bytes [..., K], scales uint8 e8m0 [..., K/32]).

    Pinned byte for byte by the float64 reference of tests/test_mx8_host.py (a table of the e4m3 magnitudes, no float8 type) at every
    rounding and scale boundary, fp32-subnormal blocks included (nothing flushes).

    Non-finite inputs are outside the format's contract (e4m3fn has no infinity, and the e8m0 NaN byte 255 is never written).  What each
    side does with them all the same:
      +-Inf: this oracle and the HIP quantiser (csrc/mx8.h) agree - the block's scale byte is 247, the element is +-448 and the block's
        finite elements are taken at 2^-120 (tests/test_gpu_mx8.py::test_quantize_non_finite_inputs);
      NaN: this oracle gives the element 0x7F (NaN) and the block scale byte 247, because amax is NaN; the HIP quantiser drops the NaN
        from amax (fmaxf), keeps the scale of the block's finite elements and writes -448 (0xFE) for the element (the clamp's fmaxf /
        fminf).  Neither touches another block."""
    x = torch.as_tensor(x, dtype=torch.float32)
    K = x.shape[-1]
    blk = x.reshape(*x.shape[:-1], K // 32, 32)
    amax = blk.abs().amax(dim=-1)
    bits = amax.view(torch.int32)
    e = ((bits >> 23) & 0xFF) + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)   # see the module docstring
    sb = torch.clamp(e - 8, min=0)
    inv = ((254 - sb) << 23).to(torch.int32).view(torch.float32)  # 2^(127 - sb)
    scaled = torch.clamp(blk * inv[..., None], -448.0, 448.0)
    q = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    return q.reshape(x.shape), sb.to(torch.uint8)


def dequantize_mx8(q, scales, dtype=torch.float32):
    """element x 2^(scale byte - 127) in `dtype`.  float32 holds every value the quantiser above produces from float32 input; bytes built by
    hand can exceed it (4 x 2^127 at scale byte 254): float64 holds them all."""
    q = torch.as_tensor(q).view(torch.float8_e4m3fn).to(dtype)
    K = q.shape[-1]
    s = torch.pow(2.0, torch.as_tensor(scales).to(dtype) - 127.0)
    return (q.reshape(*q.shape[:-1], K // 32, 32) * s[..., None]).reshape(q.shape)


def gemm_mx8(qa, sa, qb, sb, bias=None, alpha=1.0):
    """alpha * A . B^T + bias in float64 on the dequantised operands (what the scaled MFMA computes exactly,
    up to fp32 accumulation order)."""
    a, b = dequantize_mx8(qa, sa).double(), dequantize_mx8(qb, sb).double()
    c = alpha * (a @ b.transpose(-1, -2))
    return c + bias.double() if bias is not None else c
