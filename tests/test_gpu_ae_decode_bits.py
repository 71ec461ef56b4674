"""The decoder's three kernels against recorded bits (tests/golden/g2x_decode_bits.npz).

ae_decode_stream_kernel and ae_decode_rays_kernel evaluate the field through one shared function, and ae_decode_grad_stream_kernel
through parts of it (rald_amd/csrc/ae_decode_core.h), so the tests that compare them with each other (test_gpu_ae_decode_grad.py,
test_gpu_ae_rays.py) cannot see a change that they take together.  The fixture holds what the three op entries returned on an MI355X from the commit before
the function was shared, when each kernel still had its own text; every output is compared as int32 bits.

Inputs are rebuilt here from fixed seeds with the builders of test_gpu_ae_decode.py (the fixture holds outputs only): B = 2, dim = 256,
M = 64 and 512, the shipped (block-diagonal) basis and the rotated (dense) one.
  decode, decode-grad   Q = 130: two full 64-query chunks and a tail of 2 (the clamp q < Q, and the gradient kernel's break at a half
                        without a query); decode-grad also ragged with the segments (130, 0) - an empty one - and (1, 129), with the
                        projected output.  The plain decoder's ragged form has no op entry (it takes a module handle); test_gpu_infer_batch.py
                        holds it to the dense form with torch.equal.
  rays                  R = 70, n_steps = 8, n_refine = 3, per-sample ray tables, out_points.  c0 is set on the CPU (minus the 0.6 quantile
                        of the float64 formula's logits at the march's sample points, rounded to 1/64) so that the level logit = 0 cuts
                        the rays; the writer checks that hits at k = 0, later hits and misses all occur.

`python tests/test_gpu_ae_decode_bits.py [path]` writes the fixture from the library it is run against."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_ae_decode import _formula, _real_case, _rotated_basis, _run
from test_gpu_ae_decode_grad import _run_grad
from test_gpu_ae_rays import _at, _cast, _dev, _rays

gpu = pytest.mark.gpu
FIXTURE = "g2x_decode_bits.npz"
CONFIGS = [(64, "shipped"), (64, "dense"), (512, "shipped"), (512, "dense")]
Q, SEGMENTS, MAX_STEP = 130, ((130, 0), (1, 129)), 0.05
R, S, N_REFINE = 70, 8, 3

_CASES = {}


def _case(M, basis_kind):
    """(case, ray origins, ray directions); the case's c0 is the rays' (see above), which only shifts the decoders' logits"""
    if (M, basis_kind) not in _CASES:
        basis = None if basis_kind == "shipped" else _rotated_basis("dense")
        case = _real_case(256, M, 2, Q, basis=basis, seed=41)[1]
        o, d = _rays(2, R, 500 + M, True)
        pts = torch.cat([_at(o, torch.tensor(float(k)) / torch.tensor(float(S)), d) for k in range(S + 1)], dim=1)
        level = float(torch.quantile(_formula(dict(case, q=pts))[0].flatten(), 0.6))
        case["c0"] = round((case["c0"] - level) * 64) / 64
        _CASES[(M, basis_kind)] = (case, o, d)
    return _CASES[(M, basis_kind)]


def _outputs(M, basis_kind, op):
    """name -> CPU tensor, every output of `op` on the configuration"""
    case, o, d = _case(M, basis_kind)
    if op == "decode":
        return {"logits": _run(case)}
    if op == "grad":
        out = dict(zip(("logits", "grad", "projected"), _run_grad(case, project=True, max_step=MAX_STEP)))
        for i, seg in enumerate(SEGMENTS):
            got = _run_grad(case, segments=list(seg), project=True, max_step=MAX_STEP)
            out.update({f"ragged{i}_{name}": v for name, v in zip(("logits", "grad", "projected"), got)})
        return out
    return dict(zip(("t", "logit", "step", "points"), _cast(_dev(case), o, d, S, N_REFINE)))


def _bits(t):
    return t.contiguous().numpy().view(np.int32)


@gpu
@pytest.mark.parametrize("op", ["decode", "grad", "rays"])
@pytest.mark.parametrize("M,basis_kind", CONFIGS)
def test_outputs_equal_the_recorded_bits(M, basis_kind, op):
    """Every output of the op, as int32 bits, equals the recording; the gradient entry's logits are also the plain entry's."""
    gold = np.load(os.path.join(GOLDEN, FIXTURE), allow_pickle=False)
    got = _outputs(M, basis_kind, op)
    for name, v in got.items():
        want = gold[f"{op}_{M}_{basis_kind}_{name}"]
        have = _bits(v)
        assert have.shape == want.shape, (name, have.shape, want.shape)
        assert np.array_equal(have, want), (name, int((have != want).sum()), np.argwhere(have != want)[:4].tolist())
    if op == "grad":
        assert np.array_equal(_bits(got["logits"]), gold[f"decode_{M}_{basis_kind}_logits"])


if __name__ == "__main__":
    rec = {}
    for M, basis_kind in CONFIGS:
        for op in ("decode", "grad", "rays"):
            for name, v in _outputs(M, basis_kind, op).items():
                assert not bool(torch.isnan(v).any()) or op == "rays", (M, basis_kind, op, name)
                rec[f"{op}_{M}_{basis_kind}_{name}"] = _bits(v).copy()
        step = _outputs(M, basis_kind, "rays")["step"]
        shares = [int((step == 0).sum()), int((step >= 1).sum()), int((step < 0).sum())]
        print(M, basis_kind, "c0", _case(M, basis_kind)[0]["c0"], "rays hit at 0 / later / miss", shares)
        assert min(shares) >= 5, shares
        assert np.array_equal(rec[f"grad_{M}_{basis_kind}_logits"], rec[f"decode_{M}_{basis_kind}_logits"])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, FIXTURE)
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes,", len(rec), "arrays")
