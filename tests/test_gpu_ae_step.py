"""The native stage-1 training step on a real MI355X: ``train_ops.ae_loss`` (csrc/ae_train.hip) against torch in float64,
``train_ae.AeStepTrainer`` against the autograd route bit for bit and against the oracle under fp32 autograd, ``train_ae.GraphedAeStep``
against the eager step bit for bit, and three iterations on a LiDAR batch.

Bounds.  The loss op: its terms are non-negative and summed in double, so the error of a loss is at most the per-term error of expf /
log1pf, a few fp32 ulp; 16 ulp = 1.9e-6 -> 2e-6 for the four losses (relative) and for dlogits / dkl (rel-L2).  Counts are integers:
exact.  The step route against the oracle: the bounds tests/test_gpu_ae_train.py states for this arithmetic (bf16 MFMA operands, fp32
accumulation).  Everything else is bit equality: the routes run the same kernels on the same bits."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

LOSS_OP_TOL = 2e-6       # the four losses, relative; dlogits and dkl, rel-L2
LOSS_TOL = 5e-4          # step route against the oracle: loss, relative
LOGIT_TOL = 1e-2         # logits rel-L2
KL_TOL = 2e-4            # kl rel-L2
GRAD_TOL = 1e-2          # whole-gradient rel-L2
PARAM_TOL = 2.8e-2       # worst parameter rel-L2 where the reference gradient is not numerically zero
KEEP = 1 / 0.9
W = dict(vol_weight=0.7, near_weight=0.1, kl_weight=1e-3)


# ------------------------------------------------------------------------------------------------------------------ the loss op
def _loss_inputs(B, Q, seed=0):
    """logits ~ N(0, 3) with +-100, +-1e4 and exactly 0 planted under both labels, away from the two ends (with n = 1 or Q - 1 a span
    holds one term; a planted 100 under label 1 is a subnormal term there, which says nothing about the formulation)."""
    g = torch.Generator().manual_seed(seed + 1000 * B + Q)
    x = torch.randn(B, Q, generator=g) * 3
    y = (torch.rand(B, Q, generator=g) < 0.3).float()
    if Q >= 63:
        planted = torch.tensor([100.0, -100.0, 1e4, -1e4, 0.0])
        x[0, 5:10], y[0, 5:10] = planted, 0.0
        x[0, 12:17], y[0, 12:17] = planted, 1.0
        x[-1, Q - 20:Q - 15], y[-1, Q - 20:Q - 15] = planted, 1.0
        x[-1, Q - 12:Q - 7], y[-1, Q - 12:Q - 7] = planted, 0.0
    kl = torch.rand(B, generator=g) * 5 + 0.1
    return x, y, kl


def _loss_ref(x, y, kl, n, grad_scale, vol_weight, near_weight, kl_weight):
    """engine_ae.py:70-101 with torch in float64 on the CPU: BCEWithLogitsLoss per span, the reference's sums, autograd for the gradients
    of grad_scale * total; an empty span is left out of the backward pass (its loss is NaN, its gradient has no elements)."""
    x64, k64, y64 = x.double().requires_grad_(True), kl.double().requires_grad_(True), y.double()
    crit = torch.nn.BCEWithLogitsLoss()
    B, Q = x.shape
    vol, near = crit(x64[:, :n], y64[:, :n]), crit(x64[:, n:], y64[:, n:])
    klm = torch.sum(k64) / B
    total = vol_weight * vol + near_weight * near + kl_weight * klm
    live = kl_weight * klm + (vol_weight * vol if n > 0 else 0.0) + (near_weight * near if n < Q else 0.0)
    (grad_scale * live).backward()
    pred = (x >= 0).float()
    counts = torch.stack([(pred == y).sum(1), (pred * y).sum(1), (pred + y).gt(0).sum(1)], 1).to(torch.int32)
    return torch.stack([total, vol, near, klm]).detach(), counts, x64.grad, k64.grad


def _close(got, want, tol):
    return bool(((got - want).abs() <= tol * want.abs()).all())


@pytest.mark.parametrize("B,Q,n", [(2, 1500, 1), (2, 1500, 900), (3, 1500, 1499), (3, 1500, 900), (2, 63, 1), (3, 63, 62)])
def test_ae_loss_against_torch_float64(B, Q, n):
    """Measured on an MI355X over the six cases: the total at most 1.7e-8 (its weights are passed as fp32: 0.1 and 0.7 round at 2^-25),
    vol / near at most 2.7e-8, kl 0; dlogits at most 6.3e-8, dkl at most 7.7e-8 (one fp32 rounding)."""
    from rald_amd import train_ops as TO
    x, y, kl = _loss_inputs(B, Q)
    gs = 0.5
    losses, counts, dlogits, dkl = TO.ae_loss(x.cuda(), y.cuda(), kl.cuda(), n, grad_scale=gs, **W)
    l_ref, c_ref, dx_ref, dk_ref = _loss_ref(x, y, kl, n, gs, **W)
    losses, counts = losses.cpu(), counts.cpu()
    e = ((losses - l_ref).abs() / l_ref.abs()).tolist()
    print(f"ae_loss B={B} Q={Q} n={n}: losses rel {['%.1e' % v for v in e]} (bound {LOSS_OP_TOL}) dlogits {rel_l2(dlogits, dx_ref):.1e} "
          f"dkl {rel_l2(dkl, dk_ref):.1e}")
    assert losses.dtype == torch.float64 and counts.dtype == torch.int32
    assert _close(losses, l_ref, LOSS_OP_TOL)
    assert torch.equal(counts, c_ref)
    assert rel_l2(dlogits, dx_ref) <= LOSS_OP_TOL and rel_l2(dkl, dk_ref) <= LOSS_OP_TOL
    # a forward-only call (evaluation) gives the same losses and counts and no gradients
    l2, c2, d2, k2 = TO.ae_loss(x.cuda(), y.cuda(), kl.cuda(), n, grad_scale=gs, want_grad=False, **W)
    assert d2 is None and k2 is None and torch.equal(l2.cpu(), losses) and torch.equal(c2.cpu(), counts)


@pytest.mark.parametrize("B,Q", [(2, 1500), (2, 63), (3, 1)])
@pytest.mark.parametrize("empty", ["vol", "near"])
def test_ae_loss_empty_span_is_nan_and_the_other_gradient_is_written(B, Q, empty):
    from rald_amd import train_ops as TO
    x, y, kl = _loss_inputs(B, Q)
    n = 0 if empty == "vol" else Q
    losses, counts, dlogits, dkl = TO.ae_loss(x.cuda(), y.cuda(), kl.cuda(), n, **W)
    l_ref, c_ref, dx_ref, dk_ref = _loss_ref(x, y, kl, n, 1.0, **W)
    losses = losses.cpu()
    nan_at, live_at = (1, 2) if empty == "vol" else (2, 1)
    assert torch.isnan(losses[0]) and torch.isnan(losses[nan_at]) and torch.isnan(l_ref[0]) and torch.isnan(l_ref[nan_at])
    assert _close(losses[[live_at, 3]], l_ref[[live_at, 3]], LOSS_OP_TOL)
    assert torch.equal(counts.cpu(), c_ref)
    assert bool(torch.isfinite(dlogits).all()) and bool(torch.isfinite(dkl).all())
    assert rel_l2(dlogits, dx_ref) <= LOSS_OP_TOL and rel_l2(dkl, dk_ref) <= LOSS_OP_TOL


@pytest.mark.parametrize("Q,n", [(1500, 900), (10000, 9375)])
def test_ae_loss_is_bit_reproducible_and_batch_independent(Q, n):
    """Two calls give the same bits; sample 0's counts and dlogits row are the same bits alone (grad_scale 1) and inside a batch of 3
    (grad_scale 3: the 1 / B factor matches).  Q = 10 000 is the shipped shape: not a multiple of 64, ten workgroups per sample."""
    from rald_amd import train_ops as TO
    x, y, kl = (t.cuda() for t in _loss_inputs(3, Q))
    a = TO.ae_loss(x, y, kl, n, grad_scale=3.0, **W)
    b = TO.ae_loss(x, y, kl, n, grad_scale=3.0, **W)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    one = TO.ae_loss(x[:1].contiguous(), y[:1].contiguous(), kl[:1].contiguous(), n, grad_scale=1.0, **W)
    assert torch.equal(one[1][0], a[1][0])
    assert torch.equal(one[2][0], a[2][0])
    assert float(one[2].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ the step routes
def _ae(depth=2, N=1000, query_type="mix", seed=0):
    from rald_amd import models_ae as A, weights
    m = A.KLAutoEncoder(depth=depth, dim=512, queries_dim=512, output_dim=1, num_inputs=N, num_latents=512, latent_dim=32, heads=8,
                        dim_head=64, query_type=query_type)
    spec = weights.spec_of_state_dict(m.state_dict())
    m.load_state_dict(weights.make_state_dict(spec, seed), strict=True)
    return m.cuda().train()


def _stepper(m, lr=1e-4, reducer=False):
    from rald_amd.train_ae import AeStepTrainer
    from rald_amd.train_utils import FlatAdamW, GradReducer
    opt = FlatAdamW(m.parameters(), lr=lr, ema=True)
    return AeStepTrainer(m, opt, reducer=GradReducer(opt.flat_g) if reducer else None), opt


def _oracle_forward(sd, pc, q, eps, masks, depth, mix):
    """KLAutoEncoder.forward (:351-432) in training mode with explicit drop-path scales and posterior noise (the recipe of
    tests/test_gpu_ae_train.py)."""
    from oracle import rald_oracle as O
    B = pc.shape[0]
    emb = O.point_embed(sd, pc)
    if mix:
        d_q = O.ae_attention(sd, "mix_attn_layer.", sd["d_latents.weight"][None].expand(B, -1, -1), emb, 8) * masks[0].view(B, 1, 1)
        x = O._lin(sd, "query_proj", sd["s_latents.weight"][None].expand(B, -1, -1) + d_q)
        off = 1
    else:
        x = sd["latents.weight"][None].expand(B, -1, -1)
        off = 0
    x = O.ae_attention(sd, "cross_attend_blocks.0.", x, emb, heads=1) + x
    x = O.ae_ff(sd, "cross_attend_blocks.1.", x) + x
    z, kl = O.diag_gaussian(O._lin(sd, "mean_fc", x), O._lin(sd, "logvar_fc", x), eps)
    x = O._lin(sd, "proj", z)
    for i in range(depth):
        x = O.ae_attention(sd, f"layers.{i}.0.", x, None, 8) * masks[off + 2 * i].view(B, 1, 1) + x
        x = O.ae_ff(sd, f"layers.{i}.1.", x) * masks[off + 2 * i + 1].view(B, 1, 1) + x
    return O.ae_decode_queries(sd, x, q).squeeze(-1), kl


def _loss(logits, kl, labels, in_voxel_num, vol_weight=1.0, near_weight=0.1):
    """engine_ae.py:73-87 (the shipped ae config's weights)."""
    criterion = torch.nn.BCEWithLogitsLoss()
    loss_vol = criterion(logits[:, :in_voxel_num], labels[:, :in_voxel_num])
    loss_near = criterion(logits[:, in_voxel_num:], labels[:, in_voxel_num:])
    return vol_weight * loss_vol + near_weight * loss_near + 1e-3 * torch.sum(kl) / kl.shape[0]


def _inputs(B, N, Q, seed=7):
    from rald_amd import synth
    pc, q = synth.point_cloud(B, N, seed=seed), synth.queries(B, Q, seed=seed + 1)
    labels = (torch.rand(B, Q, generator=torch.Generator().manual_seed(seed + 2)) < 0.3).float()
    eps = torch.randn(B, 512, 32, generator=torch.Generator().manual_seed(seed + 3))
    return pc, q, labels, eps


B_, N_, Q_, N_IN = 2, 1000, 1500, 900
MASKS = [torch.tensor([KEEP, KEEP]), torch.tensor([KEEP, 0.0]), torch.tensor([KEEP, KEEP]), torch.tensor([0.0, KEEP]), torch.tensor([KEEP, KEEP])]


@pytest.fixture(scope="module")
def step_route():
    """One forward_backward of the step route on FlatAdamW storage (one sample's layers.0 FF branch and the other's layers.0 attention
    branch dropped): what the two parity tests below compare against."""
    from rald_amd import train_ops as TO
    m = _ae()
    st, opt = _stepper(m)
    pc, q, labels, eps = _inputs(B_, N_, Q_)
    losses, counts = st.forward_backward(pc.cuda(), q.cuda(), labels.cuda(), N_IN, eps=eps, masks=MASKS)
    _, _, dlogits, dkl = TO.ae_loss(st.logits, labels.cuda(), st.kl, N_IN)              # bit-reproducible: the gradients the step used
    return dict(m=m, losses=losses.cpu(), counts=counts.cpu(), logits=st.logits.clone(), kl=st.kl.clone(), dlogits=dlogits, dkl=dkl,
                grads={n: p.grad.clone() for n, p in m.named_parameters()}, flat_g=opt.flat_g.clone())


def test_step_route_equals_autograd_route(step_route):
    """(a) AeStepTrainer.forward_backward on FlatAdamW storage, (b) the autograd node fed the gradients ae_loss produced: the same kernels
    on the same bits."""
    m = _ae()
    pc, q, _, eps = _inputs(B_, N_, Q_)
    out = m._train_forward(pc.cuda(), q.cuda(), masks=[s.cuda() for s in MASKS], eps=eps)
    assert torch.equal(out["logits"], step_route["logits"]) and torch.equal(out["kl"], step_route["kl"])
    torch.autograd.backward([out["logits"], out["kl"]], [step_route["dlogits"], step_route["dkl"]])
    bad = [n for n, p in m.named_parameters() if not torch.equal(p.grad, step_route["grads"][n])]
    assert not bad, bad
    # the step wrote through the parameters' .grad views straight into the flat gradient
    g = step_route["flat_g"]
    assert float(g.abs().max()) > 0 and all(bool((step_route["grads"][n] != 0).any()) for n, _ in m.named_parameters())


def test_step_route_against_the_oracle(step_route):
    """Measured on an MI355X: loss 1.2e-5, logits 2.6e-3, kl 8.4e-5, whole gradient 4.0e-3, worst parameter 1.14e-2
    (mix_attn_layer.norm.weight)."""
    m = step_route["m"]
    pc, q, labels, eps = _inputs(B_, N_, Q_)
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    logits_r, kl_r = _oracle_forward(sd, pc, q, eps, MASKS, m.depth, True)
    loss_r = _loss(logits_r, kl_r, labels, N_IN)
    loss_r.backward()
    e_loss = abs(float(step_route["losses"][0]) - float(loss_r.detach())) / abs(float(loss_r.detach()))
    e_log, e_kl = rel_l2(step_route["logits"].cpu(), logits_r.detach()), rel_l2(step_route["kl"].cpu(), kl_r.detach())
    names = [n for n, _ in m.named_parameters()]
    g = {n: step_route["grads"][n].cpu() for n in names}
    gr = {n: sd[n].grad for n in names}
    cat = lambda d: torch.cat([d[n].flatten() for n in names])
    whole = float((cat(g) - cat(gr)).norm() / cat(gr).norm())
    gmax = max(float(gr[n].norm()) for n in names)
    per = {n: rel_l2(g[n], gr[n]) for n in names if float(gr[n].norm()) > 1e-4 * gmax}
    worst = max(per, key=per.get)
    print(f"step route vs oracle: loss {e_loss:.2e} (bound {LOSS_TOL}) logits {e_log:.2e} ({LOGIT_TOL}) kl {e_kl:.2e} ({KL_TOL}) "
          f"grad {whole:.2e} ({GRAD_TOL}) worst param {worst} {per[worst]:.2e} ({PARAM_TOL})")
    assert e_loss < LOSS_TOL and e_log < LOGIT_TOL and e_kl < KL_TOL
    assert whole < GRAD_TOL
    assert per[worst] < PARAM_TOL, (worst, per[worst])
    # the counts of the same logits, as the reference forms them (:92-99)
    pred = (step_route["logits"].cpu() >= 0).float()
    want = torch.stack([(pred == labels).sum(1), (pred * labels).sum(1), (pred + labels).gt(0).sum(1)], 1).to(torch.int32)
    assert torch.equal(step_route["counts"], want)


@pytest.mark.parametrize("accum_iter,n_iter", [(1, 3), (2, 4)])
def test_graphed_step_equals_eager_step(accum_iter, n_iter):
    """GraphedAeStep and AeStepTrainer.step from identical states on the same per-iteration inputs, masks and noise, with a different
    in_voxel_num each iteration (the graph reads it from device memory).  The accum_iter = 2 case hooks a GradReducer into the graphed
    step (world 1: it exchanges nothing and hands back pre_scale 1)."""
    from rald_amd.train_ae import GraphedAeStep, drop_path_masks
    me, mg = _ae(), _ae()
    (se, oe), (sg, og) = _stepper(me), _stepper(mg, reducer=accum_iter == 2)
    graphed = GraphedAeStep(sg, B_, N_, Q_, accum_iter=accum_iter)
    assert torch.equal(oe.flat_p, og.flat_p) and float(og.flat_g.abs().max()) == 0.0       # capture left parameters and gradient alone
    n_ins = [900, 700, 1100, 1300]
    torch.manual_seed(3)
    for i in range(n_iter):
        pc, q, labels, eps = _inputs(B_, N_, Q_, seed=7 + 10 * i)
        masks = drop_path_masks(B_, 5, "cuda")
        kw = dict(eps=eps, masks=masks, update=(i + 1) % accum_iter == 0, accum_iter=accum_iter, max_norm=10.0)
        le, ce, ne = se.step(pc.cuda(), q.cuda(), labels.cuda(), n_ins[i], **kw)
        lg, cg, ng = graphed(pc.cuda(), q.cuda(), labels.cuda(), n_ins[i], **kw)
        assert bool(torch.isfinite(le).all())
        assert torch.equal(le, lg) and torch.equal(ce, cg), (i, le, lg)
        assert (ne is None) == (ng is None) == (not kw["update"])
        assert torch.equal(oe.flat_g, og.flat_g), i
        for name in ("flat_p", "flat_ema", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(oe, name), getattr(og, name)), (i, name)
    assert oe.step_count == og.step_count == n_iter // accum_iter
    assert not torch.equal(oe.flat_p, oe.flat_ema)
    with pytest.raises(ValueError):
        graphed(pc.cuda(), q.cuda(), labels.cuda(), 900, accum_iter=accum_iter + 1)


def test_step_trains_on_a_lidar_batch():
    """Three AeStepTrainer.step iterations on the LidarFrames 'train' batch of test_reference_training_loop_on_a_lidar_batch (same config,
    lr 1e-4): the loss falls; eval() + no_grad encode then sees the new weights (FlatAdamW.mark_params_changed); with the same torch
    seed an autograd-route forward draws the masks the step drew."""
    from rald_amd import synth
    from rald_amd.lidar import LidarFrames, load_lidar_config
    cfg = load_lidar_config({"dataset": {"lidar": dict(pc_range=[0, -90, -20, 15.8, 90, 20], num_point_features=3, voxel_size=[0.05, 0.25, 0.5],
                                                       max_points_per_voxel=10, max_number_of_voxels=50000, sampling=True, num_samples=2048,
                                                       query_ratio=0.0625, norm_isotropy=False, norm_anisotropy=True, cache_voxel=False,
                                                       view_cone_mode=True)}})
    d = LidarFrames(cfg).batch(synth.lidar_scan(2, n=20000), "train", rng=torch.Generator("cuda").manual_seed(5), crop=True)
    surface, points, labels = d["lidar_points"], d["query_points"], d["query_labels"].float()
    m = _ae(depth=2, N=2048)
    st, opt = _stepper(m, lr=1e-4)
    torch.manual_seed(0)
    losses, first_masks = [], None
    for _ in range(3):
        l, counts, norm = st.step(surface, points, labels, d["in_voxel_num"][0], max_norm=10.0)
        losses.append(l)
        first_masks = first_masks or [t.clone() for t in st.masks]
    losses = [float(l[0]) for l in losses]
    print("losses", losses, "grad norm", float(norm))
    assert losses[-1] < losses[0]
    assert opt.step_count == 3
    twin = _ae(depth=2, N=2048)
    torch.manual_seed(0)
    twin(surface, points)
    assert len(first_masks) == 5 and all(torch.equal(a, b) for a, b in zip(first_masks, twin._last_drop_path_masks))
    m.eval()
    with torch.no_grad():
        torch.manual_seed(1)
        kl1, _ = m.encode(surface)
    from oracle import rald_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    torch.manual_seed(1)
    eps = torch.randn(2, 512, 32)
    kl_ref, _, _, _ = O.ae_encode(sd, surface.cpu(), eps)
    assert rel_l2(kl1.cpu(), kl_ref) < 1e-2, "the inference handle did not reload the trained weights"
    # the evaluation use of the loss op on the trained weights: BCE over all queries, the evaluation IoU (engine_ae.py:211-222)
    from rald_amd import engine_ae
    with torch.no_grad():
        out = m(surface, points)
    ev = engine_ae.evaluate_losses(lambda s, p: out, surface, points, labels)               # the same logits on both sides
    x, y = out["logits"].double().cpu(), labels.double().cpu()
    ref = float(torch.nn.BCEWithLogitsLoss()(x, y))
    pred = (x >= 0).double()
    iou = float(((pred * y).sum(1) / (pred + y).gt(0).sum(1) + 1e-5).mean())
    assert abs(ev["loss"] - ref) <= LOSS_OP_TOL * ref
    assert abs(ev["iou"] - iou) <= 1e-12 and abs(ev["accuracy"] - float((pred == y).double().mean())) <= 1e-12
    assert abs(ev["loss_kl"] - float(out["kl"].double().mean())) <= LOSS_OP_TOL * abs(ev["loss_kl"])
