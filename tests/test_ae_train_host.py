"""CPU tests of the autoencoder training route's host logic: the scratch-size queries of csrc/ae_train.hip (pure host arithmetic),
KLAutoEncoder.forward's route selection and its NotImplementedErrors (stubs stand in for the GPU paths), and the drop-path draw
order against timm's DropPath calls."""
import pytest
import torch


def test_scratch_size_queries_are_host_arithmetic():
    from rald_amd._lib import lib
    L = lib()
    assert L.rald_op_ln_affine_bwd_scratch_bytes(0) == 0
    assert L.rald_op_ln_affine_bwd_scratch_bytes(1) == 1024 * 4                       # one workgroup of 64 rows: gamma + beta partials
    assert L.rald_op_ln_affine_bwd_scratch_bytes(40000) == 625 * 1024 * 4
    assert L.rald_op_ln_affine_bwd_scratch_bytes(40001) == 626 * 1024 * 4
    assert L.rald_op_pe_wgrad_scratch_bytes(0) == 0
    assert L.rald_op_pe_wgrad_scratch_bytes(512) == 512 * 52 * 4                       # one workgroup of 512 rows: [512 x (51 + bias)]
    assert L.rald_op_pe_wgrad_scratch_bytes(80192) == 157 * 512 * 52 * 4


def _model(**kw):
    from rald_amd import models_ae as A
    args = dict(depth=1, dim=512, queries_dim=512, output_dim=1, num_inputs=64, num_latents=512, latent_dim=32, heads=8, dim_head=64,
                query_type="mix")
    args.update(kw)
    return A.KLAutoEncoder(**args)


def test_route_selection(monkeypatch):
    from rald_amd import models_ae as A
    m = _model()
    calls = []
    monkeypatch.setattr(A.KLAutoEncoder, "_train_forward", lambda self, pc, q: calls.append("train") or {"logits": None, "kl": None})
    monkeypatch.setattr(A.KLAutoEncoder, "encode", lambda self, pc: (calls.append("encode") or torch.zeros(1), torch.zeros(1, 512, 32)))
    monkeypatch.setattr(A.KLAutoEncoder, "decode", lambda self, x, q: calls.append("decode") or torch.zeros(1, 4, 1))
    pc, q = torch.zeros(1, 64, 3), torch.zeros(1, 4, 3)
    m.train()
    m(pc, q)
    assert calls == ["train"]
    calls.clear()
    with torch.no_grad():
        m(pc, q)
    assert calls == ["encode", "decode"]
    calls.clear()
    m.eval()
    m(pc, q)
    assert calls == ["encode", "decode"]
    calls.clear()
    m.train()
    for p in m.parameters():
        p.requires_grad_(False)
    m(pc, q)
    assert calls == ["encode", "decode"]


def test_out_of_scope_raises_not_implemented():
    pc, q = torch.zeros(1, 64, 3), torch.zeros(1, 4, 3)
    m = _model().train()
    with pytest.raises(NotImplementedError):
        m(pc.clone().requires_grad_(True), q)
    with pytest.raises(NotImplementedError):
        m(pc, q.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        _model(latent_dim=16).train()(pc, q)
    with pytest.raises(NotImplementedError):
        _model(num_latents=256).train()(pc, q)
    with pytest.raises(NotImplementedError):
        _model(query_type="learnable", latent_dim=8).train()(pc, q)


def test_trainer_refuses_cpu_parameters():
    from rald_amd.train_ae import AeTrainer
    m = _model()
    with pytest.raises(RuntimeError):
        AeTrainer(dict(m.named_parameters()), m.point_embed.basis, 1, 32, "mix")
    with pytest.raises(NotImplementedError):
        AeTrainer(dict(m.named_parameters()), m.point_embed.basis, 1, 32, "point")


def test_drop_path_masks_follow_timm_draw_order():
    """timm's DropPath (rate 0.1, scale_by_keep): x.new_empty((B, 1, 1)).bernoulli_(0.9).div_(0.9), one call per branch in the
    reference's forward order - mix_attn_layer, then layers.i attention and FF."""
    from rald_amd.train_ae import drop_path_masks
    B, depth = 5, 3
    torch.manual_seed(11)
    got = drop_path_masks(B, 1 + 2 * depth, "cpu")
    torch.manual_seed(11)
    x = torch.zeros(B, 7, 512)
    want = [x.new_empty((B, 1, 1)).bernoulli_(0.9).div_(0.9).reshape(B) for _ in range(1 + 2 * depth)]
    assert len(got) == 1 + 2 * depth
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(set(t.tolist()) <= {0.0, 1 / 0.9} or torch.allclose(t[t > 0], torch.full_like(t[t > 0], 1 / 0.9)) for t in got)
